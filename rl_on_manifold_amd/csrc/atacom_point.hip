// Device code of libatacom_point.so: the collision-avoidance kernels for {float, double} x {2, 4} obstacles.
#include "atacom_point.h"
#include "atacom_point_ops.h"

namespace atacom_point {
namespace {

template <typename T, int N>
struct Ops {
    static dim3 grid(int B) { return dim3((B + BLOCK - 1) / BLOCK); }
    static void reset(const atacom_point_config& c, void* f, int* ip, const uint8_t* mask, const void* draws, void* obs,
                      hipStream_t s) {
        hipLaunchKernelGGL((k_point_reset<T, N>), grid(c.batch), dim3(BLOCK), 0, s, params<T>(c), (T*)f, ip, mask,
                           (const T*)draws, (T*)obs);
    }
    static void step(const atacom_point_config& c, void* f, int* ip, const void* act, const void* draws, void* obs,
                     void* rew, uint8_t* ab, uint8_t* last, hipStream_t s) {
        hipLaunchKernelGGL((k_point_step<T, N>), grid(c.batch), dim3(BLOCK), 0, s, params<T>(c), (T*)f, ip, (const T*)act,
                           (const T*)draws, (T*)obs, (T*)rew, ab, last);
    }
    static void rollout(const atacom_point_config& c, int n_steps, void* f, int* ip, const void* acts, const void* draws,
                        void* obs, void* nobs, void* rew, uint8_t* ab, uint8_t* last, hipStream_t s) {
        hipLaunchKernelGGL((k_point_rollout<T, N>), grid(c.batch), dim3(BLOCK), 0, s, params<T>(c), n_steps, (T*)f, ip,
                           (const T*)acts, (const T*)draws, (T*)obs, (T*)nobs, (T*)rew, ab, last);
    }
    static void stats(const atacom_point_config& c, void* f, int* ip, double* partial, int nblocks, int clear,
                      hipStream_t s) {
        hipLaunchKernelGGL((k_point_stats<T, N>), dim3(nblocks), dim3(256), 0, s, c.batch, (T*)f, ip, partial, clear);
    }
    static void state_io(const atacom_point_config& c, void* f, int* ip, void* buf, int set, hipStream_t s) {
        hipLaunchKernelGGL((k_point_state_io<T, N>), dim3((c.batch + 255) / 256), dim3(256), 0, s, c.batch, (T*)f, ip,
                           (T*)buf, set);
    }
    static const PointOps* table() {
        static const PointOps t = {Layout<N>::VALUES_PER_ENV, Layout<N>::OBS, Layout<N>::STATE_DIM, sizeof(T),
                                   &reset, &step, &rollout, &stats, &state_io};
        return &t;
    }
};

}  // namespace

const PointOps* point_ops(int dtype, int n_objects) {
    const bool f64 = dtype == ATACOM_POINT_F64;
    if (!f64 && dtype != ATACOM_POINT_F32) return nullptr;
    switch (n_objects) {
        case 2: return f64 ? Ops<double, 2>::table() : Ops<float, 2>::table();
        case 4: return f64 ? Ops<double, 4>::table() : Ops<float, 4>::table();
        default: return nullptr;
    }
}

}  // namespace atacom_point
