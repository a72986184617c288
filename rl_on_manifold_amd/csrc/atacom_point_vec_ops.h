// Type-erased launchers of libatacom_point_vec.so: defined in atacom_point_vec.hip, consumed by the C-ABI host code
// (atacom_point_vec_capi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/atacom_point_vec_hip.h"

namespace atacom_point {

// What a checkpoint image starts with: enough of the configuration to refuse an image of another handle shape instead of
// mis-reading it.  Four 16-byte items; everything after `seed` is zero.
struct SnapHeader {
    uint32_t magic, format;
    int32_t dtype, n_objects, batch, seed;
    uint32_t pad[10];
};
static_assert(sizeof(SnapHeader) == 64, "the image header is 64 bytes");
constexpr uint32_t kSnapMagic = 0x56535041u;      // "APSV"
constexpr uint32_t kSnapFormat = 1;

// Values per environment in the handle's float buffer (atacom_point.h: Layout<N>::VALUES_PER_ENV) for an obstacle count that
// is compiled in, else 0.
int point_vec_values_per_env(int n_objects);

// One launch of k_point_step_masked<T, N> for the (dtype, n_objects) of `c`.  Returns ATACOM_POINT_E_UNSUPPORTED for a
// combination that is not compiled in, else ATACOM_POINT_OK (the launch itself is checked by the caller through
// hipGetLastError).
int point_vec_step_launch(const atacom_point_config& c, void* f, int* ip, const uint8_t* mask, const void* action,
                          const void* draws, void* obs, void* reward, uint8_t* absorbing, uint8_t* last, hipStream_t s);

// One launch of k_point_snapshot_copy<save>: f_bytes / i_bytes are the sizes of the handle's two buffers (multiples of 16).
// save: the header is made from `c` and written by the kernel.
void point_vec_snapshot_launch(const atacom_point_config& c, bool save, void* f, size_t f_bytes, int* ip, size_t i_bytes,
                               void* image, hipStream_t s);

}  // namespace atacom_point
