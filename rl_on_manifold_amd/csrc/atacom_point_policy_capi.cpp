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

std::string num(long long v) { return std::to_string(v); }

// Everything about *in that can be judged without a handle.  Copies it to *net by the ABI-size rule of
// atacom_mlp_host.h: mlp_abi_copy.
int check_mlp(const atacom_mlp* in, const std::string& w, atacom_mlp* net) {
    if (!atacom::mlp_abi_copy(in, net))
        return fail(ATACOM_POINT_E_INVALID, w + ": atacom_mlp.struct_size = " + num(in->struct_size) + " is neither sizeof(atacom_mlp) = " +
                                                num((long long)sizeof(atacom_mlp)) + " nor ATACOM_MLP_SIZE_V1 (ABI)");
    if (net->hidden != 64)
        return fail(ATACOM_POINT_E_UNSUPPORTED, w + ": hidden = " + num(net->hidden) + " is not compiled in (64 hidden units)");
    if (net->n_out != 2)
        return fail(ATACOM_POINT_E_UNSUPPORTED, w + ": n_out = " + num(net->n_out) + " (the task's action has 2 components)");
    if (net->n_in != 12 && net->n_in != 20)
        return fail(ATACOM_POINT_E_UNSUPPORTED, w + ": n_in = " + num(net->n_in) + " (the observation has 4 (1 + n_objects) = 12 or 20 components)");
    if (net->activation != 0 && net->activation != 1)
        return fail(ATACOM_POINT_E_UNSUPPORTED, w + ": activation = " + num(net->activation) + " (0 = ReLU, 1 = tanh)");
    if (net->mean_mode != 0 && net->mean_mode != 1)
        return fail(ATACOM_POINT_E_UNSUPPORTED, w + ": mean_mode = " + num(net->mean_mode) + " (0 = linear, 1 = act_scale * tanh)");
    if (net->explore < 0 || net->explore > 2)
        return fail(ATACOM_POINT_E_UNSUPPORTED, w + ": explore = " + num(net->explore) + " (0 = Gaussian, 1 = clipped Gaussian, 2 = Ornstein-Uhlenbeck)");
    if (net->squash != 0 && net->squash != 1)
        return fail(ATACOM_POINT_E_UNSUPPORTED, w + ": squash = " + num(net->squash) + " (0 or 1)");
    if (!net->W1 || !net->b1 || !net->W2 || !net->b2 || !net->W3 || !net->b3)
        return fail(ATACOM_POINT_E_INVALID, w + ": null weight pointer");
    const int n_sig = (net->sW1 != nullptr) + (net->sb1 != nullptr) + (net->sW2 != nullptr) + (net->sb2 != nullptr) +
                      (net->sW3 != nullptr) + (net->sb3 != nullptr);
    if (n_sig != 0 && n_sig != 6)
        return fail(ATACOM_POINT_E_INVALID, w + ": the sigma network needs all six weight pointers (or none)");
    if (net->explore != 0 && (net->squash || n_sig != 0))
        return fail(ATACOM_POINT_E_INVALID, w + ": explore = 1 / 2 does not combine with squash or a sigma network");
    if (net->explore == 1 && (!net->act_low || !net->act_high))
        return fail(ATACOM_POINT_E_INVALID, w + ": explore = 1 (clipped Gaussian) needs act_low and act_high");
    if (net->explore == 2 && !net->ou_state)
        return fail(ATACOM_POINT_E_INVALID, w + ": explore = 2 (Ornstein-Uhlenbeck) needs ou_state");
    if (net->explore == 2 && !(net->ou_dt > 0.0))
        return fail(ATACOM_POINT_E_INVALID, w + ": explore = 2 (Ornstein-Uhlenbeck) needs ou_dt > 0");
    return ATACOM_POINT_OK;
}

int check_handle(const atacom_point_handle* h, const std::string& w) {
    if (h->magic != atacom_point::kHandleMagic)
        return fail(ATACOM_POINT_E_INVALID, w + ": not a live handle of the libatacom_point.so this library was built with "
                                                "(layout number mismatch, or the handle was destroyed)");
    return ATACOM_POINT_OK;
}

int check_net_fits(const atacom_point_handle* h, const atacom_mlp* net, const std::string& w) {
    const int obs_dim = 4 * (1 + h->cfg.n_objects);
    if (net->n_in != obs_dim)
        return fail(ATACOM_POINT_E_UNSUPPORTED, w + ": n_in = " + num(net->n_in) + " but the handle's observation has " + num(obs_dim) +
                                                    " components (n_objects = " + num(h->cfg.n_objects) + ")");
    return ATACOM_POINT_OK;
}

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
    if (int rc = check_mlp(net, w, &m)) return rc;
    if (n_steps <= 0) return fail(ATACOM_POINT_E_INVALID, w + ": n_steps must be positive");
    if (int rc = check_handle(h, w)) return rc;
    if (int rc = check_net_fits(h, &m, w)) return rc;
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
        if (int rc = check_mlp(net, w, &m)) return rc;
    }
    if (n_steps <= 0) return fail(ATACOM_POINT_E_INVALID, w + ": n_steps must be positive");
    if (int rc = check_handle(h, w)) return rc;
    if (net) {
        if (int rc = check_net_fits(h, &m, w)) return rc;
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
