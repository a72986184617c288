// C-ABI host side of libatacom_point_compact.so (see include/atacom_point_compact_hip.h).  Borrows the handles of
// libatacom_point.so (atacom_point_handle.h) and the argument checks of libatacom_point_policy.so
// (atacom_point_policy_ops.h); validates, then dispatches to the launcher; contains no numerics.
#include <hip/hip_runtime.h>

#include <string>

#include "atacom_point_compact_ops.h"
#include "atacom_point_handle.h"
#include "atacom_point_policy_ops.h"
#define ATACOM_CAPI_E_HIP ATACOM_POINT_E_HIP
#include "atacom_capi_common.h"      // g_err, fail, HIP_TRY, DeviceGuard, ON_DEVICE

namespace {

using atacom_point::dec;

// a check of atacom_point_policy_ops.h: its message becomes this library's last error
int keep(const atacom_point::Refusal& r) { return r.code ? fail(r.code, r.msg) : ATACOM_POINT_OK; }

}  // namespace

extern "C" {

const char* atacom_point_compact_last_error(void) { return g_err.c_str(); }
const char* atacom_point_compact_version(void) { return "atacom_point_compact 1.0 (gfx950)"; }

int atacom_point_compact_rollout(atacom_point_handle* h, int32_t n_steps, const void* d_actions, const atacom_mlp* net,
                                 const void* d_noise, const void* d_draws, void* d_records, int32_t record_batch_stride,
                                 void* d_ends, int32_t ends_capacity, int32_t* d_n_ends, void* stream) {
    const std::string w = "atacom_point_compact_rollout";
    if (!h || !d_records) return fail(ATACOM_POINT_E_INVALID, w + ": null argument");
    if ((d_actions != nullptr) == (net != nullptr))
        return fail(ATACOM_POINT_E_INVALID, w + ": exactly one of d_actions and net must be given");
    atacom_mlp m;
    if (net) {
        if (int rc = keep(atacom_point::check_mlp(net, w, &m))) return rc;
    }
    if (n_steps <= 0) return fail(ATACOM_POINT_E_INVALID, w + ": n_steps must be positive");
    // (t, b) of an exception row are stored in the handle's float type: exact integers below 2^24 in float32
    if (n_steps >= (1 << 24) || record_batch_stride >= (1 << 24))
        return fail(ATACOM_POINT_E_INVALID, w + ": n_steps and record_batch_stride must be < 2^24");
    if (!d_n_ends) return fail(ATACOM_POINT_E_INVALID, w + ": d_n_ends is required");
    if (ends_capacity < 0 || (ends_capacity > 0 && !d_ends))
        return fail(ATACOM_POINT_E_INVALID, w + ": ends_capacity must be >= 0, and d_ends given when it is positive");
    if (int rc = keep(atacom_point::check_handle(h, w))) return rc;
    if (net) {
        if (int rc = keep(atacom_point::check_net_fits(h, &m, w))) return rc;
    }
    if (record_batch_stride < h->cfg.batch)
        return fail(ATACOM_POINT_E_INVALID, w + ": record_batch_stride = " + dec(record_batch_stride) + " is smaller than the batch " + dec(h->cfg.batch));
    const uintptr_t mask = (h->cfg.dtype == ATACOM_POINT_F64 ? 8 : 4) - 1;
    if (((uintptr_t)d_records & mask) || ((uintptr_t)d_ends & mask))
        return fail(ATACOM_POINT_E_INVALID, w + ": d_records and d_ends must be aligned to one element");
    if ((uintptr_t)d_n_ends & 3) return fail(ATACOM_POINT_E_INVALID, w + ": d_n_ends must be aligned to four bytes");
    ON_DEVICE(h);
    HIP_TRY(hipMemsetAsync(d_n_ends, 0, sizeof(int32_t), (hipStream_t)stream));
    if (atacom_point::point_compact_launch(h->cfg, n_steps, net ? &m : nullptr, h->f, h->ip, d_actions, d_noise, d_draws, d_records,
                                           record_batch_stride, d_ends, d_n_ends, ends_capacity, (hipStream_t)stream))
        return fail(ATACOM_POINT_E_UNSUPPORTED, w + ": no kernel for dtype " + dec(h->cfg.dtype) + ", n_objects = " + dec(h->cfg.n_objects));
    HIP_TRY(hipGetLastError());
    return ATACOM_POINT_OK;
}

}  // extern "C"
