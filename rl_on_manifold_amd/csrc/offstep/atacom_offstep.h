// Launcher of libatacom_offstep.so (include/atacom_offstep_hip.h): what the C-ABI file calls after it has validated a call, and
// the sizes both sides agree on.  The kernels are in atacom_offstep.hip; nothing here touches the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/atacom_offstep_hip.h"

namespace atacom_offstep {

constexpr int kBlock = 1024;                          // threads of the one workgroup that updates a group
constexpr int kSegments = ATACOM_OFFSTEP_TENSORS;     // W1, b1, W2, b2, W3, b3, W2a (length 0 for a plain network)

// the values of each segment in the order of grad; -> N, their sum
__host__ __device__ inline int segments(int n_in, int n_out, int n_act, int n[kSegments]) {
    n[0] = 64 * n_in, n[1] = 64, n[2] = 4096, n[3] = 64, n[4] = 64 * n_out, n[5] = n_out, n[6] = 64 * n_act;
    int N = 0;
    for (int s = 0; s < kSegments; ++s) N += n[s];
    return N;
}

inline int64_t state_bytes(int n_in, int n_out, int n_act, bool f64) {
    int n[kSegments];
    return ATACOM_OFFSTEP_HEAD + 2 * (int64_t)segments(n_in, n_out, n_act, n) * (f64 ? 8 : 4);
}

// Enqueue only; `a` has passed every check.
void init_launch(const atacom_offstep_args& a, hipStream_t s);
void step_launch(const atacom_offstep_args& a, hipStream_t s);

}  // namespace atacom_offstep
