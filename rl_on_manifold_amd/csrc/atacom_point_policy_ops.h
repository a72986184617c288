// Type-erased launcher of libatacom_point_policy.so: defined in atacom_point_policy.hip, consumed by the C-ABI host code
// (atacom_point_policy_capi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/atacom_point_policy_hip.h"

namespace atacom_point {

// One launch of k_point_rollout_mlp<T, N> for the (dtype, n_objects) of `c`.  net == nullptr: pre-generated actions `acts_in`
// (records only).  rec != nullptr: packed records with the env-axis stride rec_ld, the six array pointers unused.
// Returns ATACOM_POINT_E_UNSUPPORTED for a combination that is not compiled in, else ATACOM_POINT_OK (the launch itself
// is checked by the caller through hipGetLastError).
int point_policy_launch(const atacom_point_config& c, int n_steps, const atacom_mlp* net, void* f, int* ip,
                        const void* acts_in, const void* noise, const void* draws, void* obs, void* nobs, void* acts_out,
                        void* rew, uint8_t* ab, uint8_t* last, void* rec, int rec_ld, hipStream_t s);

}  // namespace atacom_point
