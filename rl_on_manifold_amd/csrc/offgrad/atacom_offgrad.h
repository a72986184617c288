// Launchers of libatacom_offgrad.so (include/atacom_offgrad_hip.h): what the C-ABI file calls after it has validated a call,
// and the sizes both sides agree on.  The kernels are in atacom_offgrad.hip; nothing here touches the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/atacom_offgrad_hip.h"

namespace atacom_offgrad {

constexpr int kBlock = 256;                 // threads per workgroup: four wavefronts share one staged copy of a network
constexpr int kWaves = kBlock / 64;
constexpr int kRowsF32 = 64;                // rows per wavefront and tile (four blocks of 16): the matrix-core form
constexpr int kRowsF64 = 16;                // rows per WORKGROUP and tile: the vector form
constexpr int kDefaultBlocks = 512;         // ceiling of the library's own choice of n_blocks
constexpr int kReduceBlock = 256;           // threads of a reduce workgroup: kReduceSlices slices of kReduceValues values
constexpr int kReduceValues = 32;
constexpr int kReduceSlices = kReduceBlock / kReduceValues;
constexpr int H = ATACOM_OFFGRAD_HIDDEN, NK = ATACOM_OFFGRAD_MAX_ACT, kStats = ATACOM_OFFGRAD_STATS;

// values of a gradient: W1, b1, W2, b2, W3, b3 and, for a critic, W2a (n_act = k; 0 for the actor) -- and of a partial
__host__ __device__ inline int64_t grad_size(int n_in, int n_out, int n_act) {
    return 64 * (int64_t)n_in + 64 + 4096 + 64 + 64 * n_out + n_out + 64 * n_act;
}
__host__ __device__ inline int64_t partial_size(int n_in, int n_out, int n_act) { return grad_size(n_in, n_out, n_act) + kStats; }

inline int64_t tiles(int64_t rows, bool f64) {
    const int per = f64 ? kRowsF64 : kWaves * kRowsF32;
    return (rows + per - 1) / per;
}

inline int64_t effective_blocks(int n_blocks, int64_t rows, bool f64) {
    if (n_blocks > 0) return n_blocks;
    const int64_t need = tiles(rows, f64);
    return need < kDefaultBlocks ? need : kDefaultBlocks;
}

// One network of a launch: a critic (n_out = 1, n_act = k) or the actor (W2a = null, n_act = 0; act_scale only with mean_mode).
struct NetDesc {
    const void *W1, *b1, *W2, *b2, *W2a, *W3, *b3, *shift, *scale, *act_scale;
    int n1, n_out, activation, mean_mode;
};

struct RowView {
    const void* ptr;
    int64_t so, si;
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
