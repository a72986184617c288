// The handle of libatacom_point.so, shared by the two host files that work on it: atacom_point_capi.cpp (which creates and
// destroys it) and atacom_point_policy_capi.cpp (libatacom_point_policy.so, which only borrows it).  Private: not installed,
// not part of include/atacom_point_hip.h.  Both libraries are built from one tree by one build.py; the magic number below
// carries the layout version, and a library that is handed a handle without it refuses the handle instead of reading on.
#pragma once
#include <stdint.h>
#include "../../include/atacom_point_hip.h"

namespace atacom_point {
struct PointOps;
// 'APT' with the layout number in the low byte: bump it with any change to the struct below
constexpr uint32_t kHandleMagic = 0x41505401u;
}  // namespace atacom_point

struct atacom_point_handle {
    uint32_t magic;              // atacom_point::kHandleMagic while the handle lives, 0 once destroyed
    atacom_point_config cfg;
    const atacom_point::PointOps* ops;   // launch table of libatacom_point.so (not dereferenced by the policy library)
    int device;
    void* f;                     // [groups][batch][4] of the handle's scalar type (atacom_point.h: Layout)
    int* ip;                     // [batch][4]
    double* partial_dev;
    double* partial_host;
};
