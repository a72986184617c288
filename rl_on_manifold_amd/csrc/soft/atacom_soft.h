// Launchers of libatacom_soft.so (include/atacom_soft_hip.h): what the C-ABI file calls after it has validated a call, and the
// sizes both sides agree on.  The kernels are in atacom_soft.hip; nothing here touches the device.  The workgroup and tile
// constants, tiles() and effective_blocks() are those of ../mlp/atacom_mlp_backward.h, RowView is that of
// ../mlp/atacom_mlp_forward.h.
#pragma once
#include "../../../include/atacom_soft_hip.h"
#include "../mlp/atacom_mlp_forward.h"

namespace atacom_soft {

using namespace atacom_mlp_backward;

constexpr int kStats = ATACOM_SOFT_STATS;
static_assert(H == ATACOM_SOFT_HIDDEN && NK == ATACOM_SOFT_MAX_ACT, "the shared backward pass is this library's network");

// values of a gradient: W1, b1, W2, b2, W3, b3 -- and of a partial
__host__ __device__ inline int64_t grad_size(int n_in, int n_out) { return net_size(n_in, n_out); }
__host__ __device__ inline int64_t partial_size(int n_in, int n_out) { return grad_size(n_in, n_out) + kStats; }

// One network of a launch: mu or sigma (n1 = D, n_out = k) or a critic (n1 = D + k, n_out = 1).
struct NetDesc {
    const void *W1, *b1, *W2, *b2, *W3, *b3, *shift, *scale;
    int n1, n_out, activation;
};

// what the three row kernels share
struct RowCall {
    int dtype, n_obs, n_act;
    int64_t n_rows, n_inner;
    const int64_t* idx;
    RowView obs;
};

struct TargetCall : RowCall {
    NetDesc mu, sigma, critic[2];
    RowView reward, absorbing;
    const void *eps, *act_scale, *act_shift, *log_alpha;
    int64_t eps_stride;
    double log_std_min, log_std_max, gamma;
    void *y, *action_out, *logp_out;
    int64_t y_stride, action_out_stride, logp_out_stride;
};

struct CriticCall : RowCall {
    int n_nets;
    NetDesc net[2];
    RowView action;
    const void* target;
    int64_t target_stride;
    void* grad[2];
    void* stats[2];
    void* workspace;
};

struct ActorCall : RowCall {
    NetDesc mu, sigma, critic[2];
    const void *eps, *act_scale, *act_shift, *log_alpha;
    int64_t eps_stride;
    double log_std_min, log_std_max, target_entropy;
    void *grad_mu, *grad_sigma, *stats, *action_out, *logp_out, *q_out, *dqda_out, *workspace;
    int64_t action_out_stride, logp_out_stride, q_out_stride, dqda_out_stride;
};

struct AlphaCall {
    int dtype;
    void* log_alpha;
    const void* grad;
    void* state;
    double lr, beta1, beta2, eps;
};

// Enqueue only; everything has passed every check, `blocks` >= 1.  Non-zero when there is no kernel for the dtype or width.
int target_launch(const TargetCall& c, int blocks, hipStream_t s);
int critic_launch(const CriticCall& c, int blocks, hipStream_t s);
int actor_launch(const ActorCall& c, int blocks, hipStream_t s);
int alpha_launch(const AlphaCall& c, hipStream_t s);

}  // namespace atacom_soft
