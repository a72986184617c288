// Device code of libatacom_point_compact.so: k_point_rollout_compact for {float, double} x {2, 4} obstacles x {actions, policy}.
#include "atacom_mlp_host.h"
#include "atacom_point_compact.h"
#include "atacom_point_compact_ops.h"

namespace atacom_point {
namespace {

template <typename T, int N, bool POLICY>
void launch(const atacom_point_config& c, int n_steps, const atacom_mlp* net, void* f, int* ip, const void* acts_in,
            const void* noise, const void* draws, void* rec, int rec_ld, void* ends, int* n_ends, int ends_cap, hipStream_t s) {
    size_t lds_bytes = 0;
    MlpArgs<T> args{};
    if constexpr (POLICY) {
        lds_bytes = PolicyLds<T, N>::bytes(net->sW1 != nullptr);
        args = atacom::mlp_args<T>(*net);
    }
    hipLaunchKernelGGL((k_point_rollout_compact<T, N, POLICY>), dim3((c.batch + BLOCK - 1) / BLOCK), dim3(BLOCK), lds_bytes, s,
                       params<T>(c), args, n_steps, (T*)f, ip, (const T*)acts_in, (const T*)noise, (const T*)draws, (T*)rec,
                       rec_ld, CompactEnds<T>{(T*)ends, n_ends, ends_cap});
}

template <typename T, int N>
void launch(const atacom_point_config& c, int n_steps, const atacom_mlp* net, void* f, int* ip, const void* acts_in,
            const void* noise, const void* draws, void* rec, int rec_ld, void* ends, int* n_ends, int ends_cap, hipStream_t s) {
    if (net) launch<T, N, true>(c, n_steps, net, f, ip, acts_in, noise, draws, rec, rec_ld, ends, n_ends, ends_cap, s);
    else launch<T, N, false>(c, n_steps, net, f, ip, acts_in, noise, draws, rec, rec_ld, ends, n_ends, ends_cap, s);
}

}  // namespace

int point_compact_launch(const atacom_point_config& c, int n_steps, const atacom_mlp* net, void* f, int* ip,
                         const void* acts_in, const void* noise, const void* draws, void* rec, int rec_ld, void* ends,
                         int* n_ends, int ends_cap, hipStream_t s) {
    const bool f64 = c.dtype == ATACOM_POINT_F64;
    if (!f64 && c.dtype != ATACOM_POINT_F32) return ATACOM_POINT_E_UNSUPPORTED;
#define POINT_COMPACT_GO(T, N) launch<T, N>(c, n_steps, net, f, ip, acts_in, noise, draws, rec, rec_ld, ends, n_ends, ends_cap, s)
    switch (c.n_objects) {
        case 2: if (f64) POINT_COMPACT_GO(double, 2); else POINT_COMPACT_GO(float, 2); break;
        case 4: if (f64) POINT_COMPACT_GO(double, 4); else POINT_COMPACT_GO(float, 4); break;
        default: return ATACOM_POINT_E_UNSUPPORTED;
    }
#undef POINT_COMPACT_GO
    return ATACOM_POINT_OK;
}

}  // namespace atacom_point
