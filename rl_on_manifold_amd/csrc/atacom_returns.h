// Launchers of libatacom_returns.so (include/atacom_returns_hip.h): what the C-ABI file calls after it has validated a call.
// The kernels are in atacom_returns.hip; nothing here touches the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/atacom_returns_hip.h"

namespace atacom_returns {

// Steps whose loads a scan lane has in flight ahead of the step it computes (two buffers of kDepth steps each).  Chosen by
// measurement on the MI355X: profiles/returns.md.
#ifndef ATACOM_RETURNS_DEPTH
#define ATACOM_RETURNS_DEPTH 8
#endif
constexpr int kDepth = ATACOM_RETURNS_DEPTH;

constexpr int kScanBlock = 64;     // lanes per block of the scan kernels: one wave, so that 8192 environments reach 128 CUs
constexpr int kReduceBlock = 256;  // threads per block of the reduction stage, and its largest number of first-stage blocks
constexpr int kMaxGridYZ = 65535;

// first-stage blocks of the reduction over `lanes` per-environment partial sums
inline int reduce_blocks(int64_t lanes) {
    int64_t p = (lanes + kReduceBlock - 1) / kReduceBlock;
    return (int)(p < kReduceBlock ? p : kReduceBlock);
}

// Each returns non-zero when there is no kernel for (dtype, flag_dtype).  Enqueue only.
int gae_launch(const atacom_returns_gae_args& a, hipStream_t s);
int normalize_launch(const atacom_returns_shape& sh, const atacom_returns_view& adv, double* ws, double* stats, hipStream_t s);
int episodes_launch(const atacom_returns_episodes_args& a, hipStream_t s);

}  // namespace atacom_returns
