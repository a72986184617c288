// C-ABI host side of libatacom_point_policy.so (see include/atacom_point_policy_hip.h).  Borrows the handles of
// libatacom_point.so (atacom_point_handle.h); validates, then dispatches to the launcher; contains no numerics.
#include <hip/hip_runtime.h>

#include <string>

#include "atacom_mlp_host.h"
#include "atacom_point_handle.h"
#include "atacom_point_policy_ops.h"
#define ATACOM_CAPI_E_HIP ATACOM_POINT_E_HIP
#include "atacom_capi_common.h"      // g_err, fail, HIP_TRY, DeviceGuard, ON_DEVICE

namespace {

std::string num(long long v) { return atacom_point::dec(v); }

// a check of atacom_point_policy_ops.h: its message becomes this library's last error
int keep(const atacom_point::Refusal& r) { return r.code ? fail(r.code, r.msg) : ATACOM_POINT_OK; }

size_t elem_size(const atacom_point_handle* h) { return h->cfg.dtype == ATACOM_POINT_F64 ? 8 : 4; }

}  // namespace

extern "C" {

const char* atacom_point_policy_last_error(void) { return g_err.c_str(); }
const char* atacom_point_policy_version(void) { return "atacom_point_policy 1.0 (gfx950)"; }

int atacom_point_policy_rollout(atacom_point_handle* h, int32_t n_steps, const atacom_mlp* net, const void* d_noise,
                                const void* d_draws, void* d_obs, void* d_next_obs, void* d_actions, void* d_reward,
                                uint8_t* d_absorbing, uint8_t* d_last, void* stream) {
    const std::string w = "atacom_point_policy_rollout";
    if (!h || !net || !d_obs || !d_actions || !d_reward || !d_absorbing || !d_last)
        return fail(ATACOM_POINT_E_INVALID, w + ": null argument");
    atacom_mlp m;
    if (int rc = keep(atacom_point::check_mlp(net, w, &m))) return rc;
    if (n_steps <= 0) return fail(ATACOM_POINT_E_INVALID, w + ": n_steps must be positive");
    if (int rc = keep(atacom_point::check_handle(h, w))) return rc;
    if (int rc = keep(atacom_point::check_net_fits(h, &m, w))) return rc;
    const uintptr_t mask = 4 * elem_size(h) - 1;             // observation rows are written four elements at a time
    if (((uintptr_t)d_obs & mask) || ((uintptr_t)d_next_obs & mask))
        return fail(ATACOM_POINT_E_INVALID, w + ": d_obs / d_next_obs must be aligned to four elements");
    ON_DEVICE(h);
    if (atacom_point::point_policy_launch(h->cfg, n_steps, &m, h->f, h->ip, nullptr, d_noise, d_draws, d_obs, d_next_obs,
                                          d_actions, d_reward, d_absorbing, d_last, nullptr, 0, (hipStream_t)stream))
        return fail(ATACOM_POINT_E_UNSUPPORTED, w + ": no kernel for dtype " + num(h->cfg.dtype) + ", n_objects = " + num(h->cfg.n_objects));
    HIP_TRY(hipGetLastError());
    return ATACOM_POINT_OK;
}

int atacom_point_policy_rollout_packed(atacom_point_handle* h, int32_t n_steps, const void* d_actions, const atacom_mlp* net,
                                       const void* d_noise, const void* d_draws, void* d_records,
                                       int32_t record_batch_stride, void* stream) {
    const std::string w = "atacom_point_policy_rollout_packed";
    if (!h || !d_records) return fail(ATACOM_POINT_E_INVALID, w + ": null argument");
    if ((d_actions != nullptr) == (net != nullptr))
        return fail(ATACOM_POINT_E_INVALID, w + ": exactly one of d_actions and net must be given");
    atacom_mlp m;
    if (net) {
        if (int rc = keep(atacom_point::check_mlp(net, w, &m))) return rc;
    }
    if (n_steps <= 0) return fail(ATACOM_POINT_E_INVALID, w + ": n_steps must be positive");
    if (int rc = keep(atacom_point::check_handle(h, w))) return rc;
    if (net) {
        if (int rc = keep(atacom_point::check_net_fits(h, &m, w))) return rc;
    }
    if (record_batch_stride < h->cfg.batch)
        return fail(ATACOM_POINT_E_INVALID, w + ": record_batch_stride = " + num(record_batch_stride) + " is smaller than the batch " + num(h->cfg.batch));
    if ((uintptr_t)d_records & (elem_size(h) - 1))
        return fail(ATACOM_POINT_E_INVALID, w + ": d_records must be aligned to one element");
    ON_DEVICE(h);
    if (atacom_point::point_policy_launch(h->cfg, n_steps, net ? &m : nullptr, h->f, h->ip, d_actions, d_noise, d_draws, nullptr,
                                          nullptr, nullptr, nullptr, nullptr, nullptr, d_records, record_batch_stride,
                                          (hipStream_t)stream))
        return fail(ATACOM_POINT_E_UNSUPPORTED, w + ": no kernel for dtype " + num(h->cfg.dtype) + ", n_objects = " + num(h->cfg.n_objects));
    HIP_TRY(hipGetLastError());
    return ATACOM_POINT_OK;
}

}  // extern "C"
