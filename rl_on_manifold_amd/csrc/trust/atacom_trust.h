// Launcher of libatacom_trust.so (include/atacom_trust_hip.h): what the C-ABI file calls after it has validated a call, and the
// sizes both sides agree on.  The kernels are in atacom_trust.hip; nothing here touches the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/atacom_trust_hip.h"

namespace atacom_trust {

constexpr int kBlock = 256;                 // threads per workgroup: four wavefronts share one staged copy of weights and direction
constexpr int kWaves = kBlock / 64;
constexpr int kRowsF32 = 64;                // rows per wavefront and tile (four blocks of 16): the matrix-core form
constexpr int kRowsF64 = 16;                // rows per WORKGROUP and tile: the vector form
constexpr int kDefaultBlocks = 512;         // ceiling of the library's own choice of n_blocks
constexpr int kReduceBlock = 256;           // threads of a k_trust_reduce workgroup: kReduceSlices slices of kReduceValues values
constexpr int kReduceValues = 32;
constexpr int kReduceSlices = kReduceBlock / kReduceValues;

// values of the network part of a direction = of one workgroup's partial
__host__ __device__ inline int64_t net_size(int n_in, int n_out) { return 64 * (int64_t)n_in + 64 + 4096 + 64 + 64 * n_out + n_out; }

inline int64_t tiles(int64_t rows, bool f64) {
    const int per = f64 ? kRowsF64 : kWaves * kRowsF32;
    return (rows + per - 1) / per;
}

inline int64_t effective_blocks(int n_blocks, int64_t rows, bool f64) {
    if (n_blocks > 0) return n_blocks;
    const int64_t need = tiles(rows, f64);
    return need < kDefaultBlocks ? need : kDefaultBlocks;
}

// Enqueue only; `net` has passed every check, `blocks` >= 1, `rows` = M.  Returns non-zero when there is no kernel.
int trust_launch(const atacom_trust_args& a, const atacom_mlp& net, int blocks, int64_t rows, hipStream_t s);

}  // namespace atacom_trust
