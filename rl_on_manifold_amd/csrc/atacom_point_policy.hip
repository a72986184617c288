// Device code of libatacom_point_policy.so: k_point_rollout_mlp for {float, double} x {2, 4} obstacles.
#include "atacom_mlp_host.h"
#include "atacom_point_policy.h"
#include "atacom_point_policy_ops.h"

namespace atacom_point {
namespace {

template <typename T, int N>
void launch(const atacom_point_config& c, int n_steps, const atacom_mlp* net, void* f, int* ip, const void* acts_in,
            const void* noise, const void* draws, void* obs, void* nobs, void* acts_out, void* rew, uint8_t* ab,
            uint8_t* last, void* rec, int rec_ld, hipStream_t s) {
    // pre-generated actions: nothing is staged, no dynamic LDS
    const size_t lds_bytes = net ? PolicyLds<T, N>::bytes(net->sW1 != nullptr) : 0;
    hipLaunchKernelGGL((k_point_rollout_mlp<T, N>), dim3((c.batch + BLOCK - 1) / BLOCK), dim3(BLOCK), lds_bytes, s,
                       params<T>(c), net ? atacom::mlp_args<T>(*net) : MlpArgs<T>{}, n_steps, (T*)f, ip, (const T*)acts_in, (const T*)noise,
                       (const T*)draws, (T*)obs, (T*)nobs, (T*)acts_out, (T*)rew, ab, last, (T*)rec, rec_ld);
}

}  // namespace

int point_policy_launch(const atacom_point_config& c, int n_steps, const atacom_mlp* net, void* f, int* ip,
                        const void* acts_in, const void* noise, const void* draws, void* obs, void* nobs, void* acts_out,
                        void* rew, uint8_t* ab, uint8_t* last, void* rec, int rec_ld, hipStream_t s) {
    const bool f64 = c.dtype == ATACOM_POINT_F64;
    if (!f64 && c.dtype != ATACOM_POINT_F32) return ATACOM_POINT_E_UNSUPPORTED;
#define POINT_POLICY_GO(T, N) \
    launch<T, N>(c, n_steps, net, f, ip, acts_in, noise, draws, obs, nobs, acts_out, rew, ab, last, rec, rec_ld, s)
    switch (c.n_objects) {
        case 2: if (f64) POINT_POLICY_GO(double, 2); else POINT_POLICY_GO(float, 2); break;
        case 4: if (f64) POINT_POLICY_GO(double, 4); else POINT_POLICY_GO(float, 4); break;
        default: return ATACOM_POINT_E_UNSUPPORTED;
    }
#undef POINT_POLICY_GO
    return ATACOM_POINT_OK;
}

}  // namespace atacom_point
