// Launcher of libatacom_fit.so (include/atacom_fit_hip.h): what the C-ABI file calls after it has validated a call, and the
// sizes both sides agree on.  The kernels are in atacom_fit.hip; nothing here touches the device.  The workgroup and tile
// constants, tiles() and effective_blocks() are those of ../mlp/atacom_mlp_backward.h.
#pragma once
#include "../../../include/atacom_fit_hip.h"
#include "../mlp/atacom_mlp_backward.h"

namespace atacom_fit {

using namespace atacom_mlp_backward;

// values of a gradient, and of one workgroup's partial (the d log std slots and the statistics are always there)
__host__ __device__ inline int64_t grad_size(int n_in, int n_out) { return net_size(n_in, n_out); }
__host__ __device__ inline int64_t partial_size(int n_in, int n_out) { return grad_size(n_in, n_out) + n_out + ATACOM_FIT_STATS; }

// Enqueue only; `net` has passed every check, `blocks` >= 1, `rows` = M.  Returns non-zero when there is no kernel.
int fit_launch(const atacom_fit_args& a, const atacom_mlp& net, int blocks, int64_t rows, hipStream_t s);

}  // namespace atacom_fit
