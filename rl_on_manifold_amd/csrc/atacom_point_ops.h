// Type-erased launch table of libatacom_point.so: one per (scalar type, number of obstacles); defined in atacom_point.hip,
// consumed by the C-ABI host code (atacom_point_capi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/atacom_point_hip.h"

namespace atacom_point {

struct PointOps {
    int values_per_env;          // elements of the float buffer per environment (groups of four); the int buffer holds 4
    int obs_dim, state_dim;
    size_t elem;
    void (*reset)(const atacom_point_config&, void* f, int* ip, const uint8_t* mask, const void* draws, void* obs,
                  hipStream_t s);
    void (*step)(const atacom_point_config&, void* f, int* ip, const void* act, const void* draws, void* obs, void* rew,
                 uint8_t* ab, uint8_t* last, hipStream_t s);
    void (*rollout)(const atacom_point_config&, int n_steps, void* f, int* ip, const void* acts, const void* draws,
                    void* obs, void* nobs, void* rew, uint8_t* ab, uint8_t* last, hipStream_t s);
    void (*stats)(const atacom_point_config&, void* f, int* ip, double* partial, int nblocks, int clear, hipStream_t s);
    void (*state_io)(const atacom_point_config&, void* f, int* ip, void* buf, int set, hipStream_t s);
};

// nullptr for a combination that is not compiled in (n_objects other than 2 and 4)
const PointOps* point_ops(int dtype, int n_objects);

}  // namespace atacom_point
