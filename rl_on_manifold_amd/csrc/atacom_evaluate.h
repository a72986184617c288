// Launcher of libatacom_evaluate.so (include/atacom_evaluate_hip.h): what the C-ABI file calls after it has validated a call.
// The kernels are in atacom_evaluate.hip; nothing here touches the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/atacom_evaluate_hip.h"

namespace atacom_evaluate {

constexpr int kBlock = 256;                 // threads per workgroup: four wavefronts, one per SIMD, share one staged copy of the weights
constexpr int kWaves = kBlock / 64;
constexpr int kRowsF32 = 64;                // rows per wavefront and tile: the matrix-core form, one row per lane
constexpr int kRowsF64 = 16;                // the vector form, four lanes per row
// Workgroups a compute unit holds.  Float32: 62.3 KB of LDS each, two in 160 KB, and at most 256 registers a lane (__launch_bounds__), two wavefronts per
// SIMD -- eight wavefronts per CU, so that one's loads, LDS exchanges and activations run under another's MFMAs.  (Workgroups
// of two wavefronts were measured first: the dispatcher stacks two of them on the same pair of SIMDs and leaves the other pair
// idle, profiles/evaluate.md.)  Float64 holds 350 to 370 registers: one workgroup.
constexpr int kResident = 2;

inline int64_t tiles(int64_t rows, bool f64) {
    const int per = kWaves * (f64 ? kRowsF64 : kRowsF32);
    return (rows + per - 1) / per;
}

// Enqueue only; `net` has passed every check, `blocks` >= 1.  Returns non-zero when there is no kernel for the dtype.
int evaluate_launch(const atacom_evaluate_args& a, const atacom_mlp& net, int blocks, hipStream_t s);

}  // namespace atacom_evaluate
