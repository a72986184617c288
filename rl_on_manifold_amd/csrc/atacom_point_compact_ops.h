// Type-erased launcher of libatacom_point_compact.so: defined in atacom_point_compact.hip, consumed by the C-ABI host code
// (atacom_point_compact_capi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/atacom_point_compact_hip.h"

namespace atacom_point {

// One launch of k_point_rollout_compact<T, N, POLICY> for the (dtype, n_objects) of `c`; POLICY = (net != nullptr), else the
// pre-generated actions `acts_in`.  rec [n_steps + 1, rec_ld, 4 (1 + N) + 5]; ends / n_ends / ends_cap: the exception list
// (n_ends zeroed by the caller on the same stream).  Returns ATACOM_POINT_E_UNSUPPORTED for a combination that is not compiled
// in, else ATACOM_POINT_OK (the launch itself is checked by the caller through hipGetLastError).
int point_compact_launch(const atacom_point_config& c, int n_steps, const atacom_mlp* net, void* f, int* ip,
                         const void* acts_in, const void* noise, const void* draws, void* rec, int rec_ld, void* ends,
                         int* n_ends, int ends_cap, hipStream_t s);

}  // namespace atacom_point
