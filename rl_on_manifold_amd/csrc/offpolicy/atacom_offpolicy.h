// Launchers of libatacom_offpolicy.so (include/atacom_offpolicy_hip.h): what the C-ABI file calls after it has validated a
// call.  The kernels are in atacom_offpolicy.hip; nothing here touches the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/atacom_offpolicy_hip.h"

namespace atacom_offpolicy {

constexpr int kBlock = 256;                 // threads per workgroup: four wavefronts share one staged copy of a network
constexpr int kWaves = kBlock / 64;
constexpr int kRowsF32 = 64;                // rows per wavefront and tile: the matrix-core form, one row per lane
constexpr int kRowsF64 = 16;                // the vector form, four lanes per row
constexpr int kResident = 2;                // float32 workgroups a compute unit holds (62.3 KB of LDS, <= 256 registers)
constexpr int kSoftBlock = 256;

inline int64_t tiles(int64_t rows, bool f64) {
    const int per = kWaves * (f64 ? kRowsF64 : kRowsF32);
    return (rows + per - 1) / per;
}

// One network of a launch: the actor (W2a = null, n_act_in = 0) or a critic (n_out = 1).
struct NetDesc {
    const void *W1, *b1, *W2, *b2, *W2a, *W3, *b3, *shift, *scale, *act_scale;
    int n1, n_out, activation, mean_mode;
};

// A validated call of either entry point: `has_actor` = the target (net[0] is the actor, then n_critics critics), else q
// (net[0] is the critic, `action` is read and `y` receives q).
struct Call {
    int dtype, has_actor, n_nets, kind, n_obs, n_act;
    NetDesc net[3];
    int64_t n_rows, n_inner;
    const int64_t* idx;
    atacom_evaluate_view obs, action, reward, absorbing;
    const void* eps;
    int64_t eps_stride;
    const void *low, *high;
    double noise_std, noise_clip, gamma;
    void* y;
    int64_t y_stride;
    void* action_out;
    int64_t action_out_stride;
};

// Enqueue only; everything has passed every check, `blocks` >= 1.  Non-zero when there is no kernel for the dtype or width.
int net_launch(const Call& c, int blocks, hipStream_t s);
void soft_update_launch(const atacom_offpolicy_soft_update_args& a, hipStream_t s);

// the values of each tensor of a pair, in the header's order
inline void pair_sizes(const atacom_offpolicy_pair& p, int (&n)[ATACOM_OFFPOLICY_TENSORS]) {
    const int H = ATACOM_OFFPOLICY_HIDDEN;
    n[0] = H * p.n_in, n[1] = H, n[2] = H * H, n[3] = H, n[4] = p.n_out * H, n[5] = p.n_out, n[6] = H * p.n_act;
}

}  // namespace atacom_offpolicy
