// Launcher of libatacom_trust.so (include/atacom_trust_hip.h): what the C-ABI file calls after it has validated a call, and the
// sizes both sides agree on.  The kernels are in atacom_trust.hip; nothing here touches the device.  The workgroup and tile
// constants, tiles(), effective_blocks() and net_size() -- the values of the network part of a direction = of one workgroup's
// partial -- are those of ../mlp/atacom_mlp_backward.h.
#pragma once
#include "../../../include/atacom_trust_hip.h"
#include "../mlp/atacom_mlp_backward.h"

namespace atacom_trust {

using namespace atacom_mlp_backward;

// Enqueue only; `net` has passed every check, `blocks` >= 1, `rows` = M.  Returns non-zero when there is no kernel.
int trust_launch(const atacom_trust_args& a, const atacom_mlp& net, int blocks, int64_t rows, hipStream_t s);

}  // namespace atacom_trust
