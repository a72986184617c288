// Device code of libatacom_point_policy.so: k_point_rollout_mlp for {float, double} x {2, 4} obstacles.
#include <cmath>

#include "atacom_point_policy.h"
#include "atacom_point_policy_ops.h"

namespace atacom_point {
namespace {

// the launch parameters atacom_point.hip forms from the same config
template <typename T>
PParams<T> params(const atacom_point_config& c) {
    PParams<T> P;
    P.batch = c.batch; P.horizon = c.horizon; P.auto_reset = c.auto_reset; P.random_walk = c.random_walk;
    P.seed = (unsigned int)c.seed;
    P.dt = (T)c.dt;
    return P;
}

template <typename T>
MlpArgs<T> mlp_args(const atacom_mlp* net) {
    MlpArgs<T> a{};
    if (!net) return a;
    a.W1 = (const T*)net->W1; a.b1 = (const T*)net->b1; a.W2 = (const T*)net->W2; a.b2 = (const T*)net->b2;
    a.W3 = (const T*)net->W3; a.b3 = (const T*)net->b3; a.obs_shift = (const T*)net->obs_shift;
    a.obs_scale = (const T*)net->obs_scale; a.std = (const T*)net->std;
    a.sW1 = (const T*)net->sW1; a.sb1 = (const T*)net->sb1; a.sW2 = (const T*)net->sW2; a.sb2 = (const T*)net->sb2;
    a.sW3 = (const T*)net->sW3; a.sb3 = (const T*)net->sb3;
    a.log_std_min = (T)net->log_std_min; a.log_std_max = (T)net->log_std_max; a.squash = net->squash;
    a.n_in = net->n_in; a.n_out = net->n_out; a.activation = net->activation;
    a.mean_mode = net->mean_mode; a.explore = net->explore;
    a.act_scale = (const T*)net->act_scale; a.act_low = (const T*)net->act_low; a.act_high = (const T*)net->act_high;
    a.ou_x0 = (const T*)net->ou_x0; a.ou_state = (T*)net->ou_state;
    // x <- x - (theta dt) x + (sqrt(dt) std) eps: the two products of constants formed once, in double (atacom_ops_impl.h)
    a.ou_theta_dt = (T)(net->ou_theta * net->ou_dt);
    a.ou_sqrt_dt = (T)(net->explore == 2 ? std::sqrt(net->ou_dt) : 0.0);
    return a;
}

template <typename T, int N>
void launch(const atacom_point_config& c, int n_steps, const atacom_mlp* net, void* f, int* ip, const void* acts_in,
            const void* noise, const void* draws, void* obs, void* nobs, void* acts_out, void* rew, uint8_t* ab,
            uint8_t* last, void* rec, int rec_ld, hipStream_t s) {
    // pre-generated actions: nothing is staged, no dynamic LDS
    const size_t lds_bytes = net ? PolicyLds<T, N>::bytes(net->sW1 != nullptr) : 0;
    hipLaunchKernelGGL((k_point_rollout_mlp<T, N>), dim3((c.batch + BLOCK - 1) / BLOCK), dim3(BLOCK), lds_bytes, s,
                       params<T>(c), mlp_args<T>(net), n_steps, (T*)f, ip, (const T*)acts_in, (const T*)noise,
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
