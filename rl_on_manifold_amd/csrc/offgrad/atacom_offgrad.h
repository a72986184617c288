// Launchers of libatacom_offgrad.so (include/atacom_offgrad_hip.h): what the C-ABI file calls after it has validated a call,
// and the sizes both sides agree on.  The kernels are in atacom_offgrad.hip; nothing here touches the device.  The workgroup and
// tile constants, tiles() and effective_blocks() are those of ../mlp/atacom_mlp_backward.h, RowView is that of
// ../mlp/atacom_mlp_forward.h.
#pragma once
#include "../../../include/atacom_offgrad_hip.h"
#include "../mlp/atacom_mlp_forward.h"

namespace atacom_offgrad {

using namespace atacom_mlp_backward;

constexpr int kStats = ATACOM_OFFGRAD_STATS;
static_assert(H == ATACOM_OFFGRAD_HIDDEN && NK == ATACOM_OFFGRAD_MAX_ACT, "the shared backward pass is this library's network");

// values of a gradient: the network's (W1, b1, W2, b2, W3, b3) and, for a critic, W2a behind them (n_act = k; 0 for the actor)
// -- and of a partial
__host__ __device__ inline int64_t grad_size(int n_in, int n_out, int n_act) { return net_size(n_in, n_out) + 64 * n_act; }
__host__ __device__ inline int64_t partial_size(int n_in, int n_out, int n_act) { return grad_size(n_in, n_out, n_act) + kStats; }

// One network of a launch: a critic (n_out = 1, n_act = k) or the actor (W2a = null, n_act = 0; act_scale only with mean_mode).
struct NetDesc {
    const void *W1, *b1, *W2, *b2, *W2a, *W3, *b3, *shift, *scale, *act_scale;
    int n1, n_out, activation, mean_mode;
};

// A validated critic call: n_nets critics on the same rows.
struct CriticCall {
    int dtype, n_nets, kind, n_obs, n_act;
    NetDesc net[2];
    int64_t n_rows, n_inner;
    const int64_t* idx;
    RowView obs, action;
    const void* target;
    int64_t target_stride;
    void* grad[2];
    void* stats[2];
    void* workspace;
};

// A validated actor call.
struct ActorCall {
    int dtype, kind, n_obs, n_act;
    NetDesc actor, critic;
    int64_t n_rows, n_inner;
    const int64_t* idx;
    RowView obs;
    void *grad, *stats, *action_out, *dqda_out, *workspace;
    int64_t action_out_stride, dqda_out_stride;
};

// Enqueue only; everything has passed every check, `blocks` >= 1.  Non-zero when there is no kernel for the dtype or width.
int critic_launch(const CriticCall& c, int blocks, hipStream_t s);
int actor_launch(const ActorCall& c, int blocks, hipStream_t s);

}  // namespace atacom_offgrad
