// Device code of libatacom_point_vec.so: k_point_step_masked for {float, double} x {2, 4} obstacles and k_point_snapshot_copy
// for the two directions.
#include <algorithm>

#include "atacom_point_vec.h"
#include "atacom_point_vec_ops.h"

namespace atacom_point {
namespace {

constexpr int kCopyBlocks = 2048;        // 256 CUs x 8 workgroups: the copy strides over the rest

template <typename T, int N>
void launch_step(const atacom_point_config& c, void* f, int* ip, const uint8_t* mask, const void* action, const void* draws,
                 void* obs, void* reward, uint8_t* absorbing, uint8_t* last, hipStream_t s) {
    hipLaunchKernelGGL((k_point_step_masked<T, N>), dim3((c.batch + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, params<T>(c), (T*)f,
                       ip, mask, (const T*)action, (const T*)draws, (T*)obs, (T*)reward, absorbing, last);
}

}  // namespace

int point_vec_values_per_env(int n_objects) {
    switch (n_objects) {
        case 2: return Layout<2>::VALUES_PER_ENV;
        case 4: return Layout<4>::VALUES_PER_ENV;
        default: return 0;
    }
}

int point_vec_step_launch(const atacom_point_config& c, void* f, int* ip, const uint8_t* mask, const void* action,
                          const void* draws, void* obs, void* reward, uint8_t* absorbing, uint8_t* last, hipStream_t s) {
    const bool f64 = c.dtype == ATACOM_POINT_F64;
    if (!f64 && c.dtype != ATACOM_POINT_F32) return ATACOM_POINT_E_UNSUPPORTED;
#define POINT_VEC_GO(T, N) launch_step<T, N>(c, f, ip, mask, action, draws, obs, reward, absorbing, last, s)
    switch (c.n_objects) {
        case 2: if (f64) POINT_VEC_GO(double, 2); else POINT_VEC_GO(float, 2); break;
        case 4: if (f64) POINT_VEC_GO(double, 4); else POINT_VEC_GO(float, 4); break;
        default: return ATACOM_POINT_E_UNSUPPORTED;
    }
#undef POINT_VEC_GO
    return ATACOM_POINT_OK;
}

void point_vec_snapshot_launch(const atacom_point_config& c, bool save, void* f, size_t f_bytes, int* ip, size_t i_bytes,
                               void* image, hipStream_t s) {
    SnapHeader hdr{};
    hdr.magic = kSnapMagic; hdr.format = kSnapFormat;
    hdr.dtype = c.dtype; hdr.n_objects = c.n_objects; hdr.batch = c.batch; hdr.seed = c.seed;
    const size_t nf = f_bytes / sizeof(Item), ni = i_bytes / sizeof(Item);
    const dim3 grid((unsigned)std::min<size_t>(kCopyBlocks, (nf + ni + BLOCK - 1) / BLOCK));
    if (save) hipLaunchKernelGGL((k_point_snapshot_copy<true>), grid, dim3(BLOCK), 0, s, hdr, (Item*)f, nf, (Item*)ip, ni, (Item*)image);
    else hipLaunchKernelGGL((k_point_snapshot_copy<false>), grid, dim3(BLOCK), 0, s, hdr, (Item*)f, nf, (Item*)ip, ni, (Item*)image);
}

}  // namespace atacom_point
