// Launchers of libatacom_soft.so (include/atacom_soft_hip.h): what the C-ABI file calls after it has validated a call, and the
// sizes both sides agree on.  The kernels are in atacom_soft.hip; nothing here touches the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/atacom_soft_hip.h"

namespace atacom_soft {

constexpr int kBlock = 256;                 // threads per workgroup: four wavefronts share one staged copy of a network
constexpr int kWaves = kBlock / 64;
constexpr int kRowsF32 = 64;                // rows per wavefront and tile (four blocks of 16): the matrix-core form
constexpr int kRowsF64 = 16;                // rows per WORKGROUP and tile: the vector form
constexpr int kDefaultBlocks = 512;         // ceiling of the library's own choice of n_blocks
constexpr int kReduceBlock = 256;           // threads of a reduce workgroup: kReduceSlices slices of kReduceValues values
constexpr int kReduceValues = 32;
constexpr int kReduceSlices = kReduceBlock / kReduceValues;
constexpr int H = ATACOM_SOFT_HIDDEN, NK = ATACOM_SOFT_MAX_ACT, kStats = ATACOM_SOFT_STATS;

// values of a gradient: W1, b1, W2, b2, W3, b3 -- and of a partial
__host__ __device__ inline int64_t grad_size(int n_in, int n_out) { return 64 * (int64_t)n_in + 64 + 4096 + 64 + 64 * n_out + n_out; }
__host__ __device__ inline int64_t partial_size(int n_in, int n_out) { return grad_size(n_in, n_out) + kStats; }

inline int64_t tiles(int64_t rows, bool f64) {
    const int per = f64 ? kRowsF64 : kWaves * kRowsF32;
    return (rows + per - 1) / per;
}

inline int64_t effective_blocks(int n_blocks, int64_t rows, bool f64) {
    if (n_blocks > 0) return n_blocks;
    const int64_t need = tiles(rows, f64);
    return need < kDefaultBlocks ? need : kDefaultBlocks;
}

// One network of a launch: mu or sigma (n1 = D, n_out = k) or a critic (n1 = D + k, n_out = 1).
struct NetDesc {
    const void *W1, *b1, *W2, *b2, *W3, *b3, *shift, *scale;
    int n1, n_out, activation;
};

struct RowView {
    const void* ptr;
    int64_t so, si;
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
