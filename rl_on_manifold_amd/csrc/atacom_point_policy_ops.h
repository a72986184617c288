// Host interface of libatacom_point_policy.so: the argument checks of its entry points, which libatacom_point_compact.so
// (atacom_point_compact_capi.cpp) applies as they are, and the type-erased launcher defined in atacom_point_policy.hip and
// consumed by the C-ABI host code (atacom_point_policy_capi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/atacom_point_policy_hip.h"
#include "atacom_mlp_host.h"
#include "atacom_point_handle.h"

namespace atacom_point {

// ------------------------------------------------------------------ argument checks
// What the entry points of the task's libraries that take a network (libatacom_point_policy.so, libatacom_point_compact.so)
// refuse, with one wording.  Internal linkage, no error state: a check returns its verdict, and the calling C-ABI file keeps
// the message as its own library's last error.  `w` is the name of the entry point.
struct Refusal {
    int code;                    // ATACOM_POINT_OK or the ATACOM_POINT_E_* to return
    std::string msg;
};

static Refusal refuse(int code, const std::string& msg) { return Refusal{code, msg}; }
static std::string dec(long long v) { return std::to_string(v); }

// Everything about *in that can be judged without a handle.  Copies it to *net by the ABI-size rule of
// atacom_mlp_host.h: mlp_abi_copy.
static Refusal check_mlp(const atacom_mlp* in, const std::string& w, atacom_mlp* net) {
    if (!atacom::mlp_abi_copy(in, net))
        return refuse(ATACOM_POINT_E_INVALID, w + ": atacom_mlp.struct_size = " + dec(in->struct_size) + " is neither sizeof(atacom_mlp) = " +
                                                dec((long long)sizeof(atacom_mlp)) + " nor ATACOM_MLP_SIZE_V1 (ABI)");
    if (net->hidden != 64)
        return refuse(ATACOM_POINT_E_UNSUPPORTED, w + ": hidden = " + dec(net->hidden) + " is not compiled in (64 hidden units)");
    if (net->n_out != 2)
        return refuse(ATACOM_POINT_E_UNSUPPORTED, w + ": n_out = " + dec(net->n_out) + " (the task's action has 2 components)");
    if (net->n_in != 12 && net->n_in != 20)
        return refuse(ATACOM_POINT_E_UNSUPPORTED, w + ": n_in = " + dec(net->n_in) + " (the observation has 4 (1 + n_objects) = 12 or 20 components)");
    if (net->activation != 0 && net->activation != 1)
        return refuse(ATACOM_POINT_E_UNSUPPORTED, w + ": activation = " + dec(net->activation) + " (0 = ReLU, 1 = tanh)");
    if (net->mean_mode != 0 && net->mean_mode != 1)
        return refuse(ATACOM_POINT_E_UNSUPPORTED, w + ": mean_mode = " + dec(net->mean_mode) + " (0 = linear, 1 = act_scale * tanh)");
    if (net->explore < 0 || net->explore > 2)
        return refuse(ATACOM_POINT_E_UNSUPPORTED, w + ": explore = " + dec(net->explore) + " (0 = Gaussian, 1 = clipped Gaussian, 2 = Ornstein-Uhlenbeck)");
    if (net->squash != 0 && net->squash != 1)
        return refuse(ATACOM_POINT_E_UNSUPPORTED, w + ": squash = " + dec(net->squash) + " (0 or 1)");
    if (!net->W1 || !net->b1 || !net->W2 || !net->b2 || !net->W3 || !net->b3)
        return refuse(ATACOM_POINT_E_INVALID, w + ": null weight pointer");
    const int n_sig = (net->sW1 != nullptr) + (net->sb1 != nullptr) + (net->sW2 != nullptr) + (net->sb2 != nullptr) +
                      (net->sW3 != nullptr) + (net->sb3 != nullptr);
    if (n_sig != 0 && n_sig != 6)
        return refuse(ATACOM_POINT_E_INVALID, w + ": the sigma network needs all six weight pointers (or none)");
    if (net->explore != 0 && (net->squash || n_sig != 0))
        return refuse(ATACOM_POINT_E_INVALID, w + ": explore = 1 / 2 does not combine with squash or a sigma network");
    if (net->explore == 1 && (!net->act_low || !net->act_high))
        return refuse(ATACOM_POINT_E_INVALID, w + ": explore = 1 (clipped Gaussian) needs act_low and act_high");
    if (net->explore == 2 && !net->ou_state)
        return refuse(ATACOM_POINT_E_INVALID, w + ": explore = 2 (Ornstein-Uhlenbeck) needs ou_state");
    if (net->explore == 2 && !(net->ou_dt > 0.0))
        return refuse(ATACOM_POINT_E_INVALID, w + ": explore = 2 (Ornstein-Uhlenbeck) needs ou_dt > 0");
    return Refusal{ATACOM_POINT_OK, std::string()};
}

static Refusal check_handle(const atacom_point_handle* h, const std::string& w) {
    if (h->magic != atacom_point::kHandleMagic)
        return refuse(ATACOM_POINT_E_INVALID, w + ": not a live handle of the libatacom_point.so this library was built with "
                                                "(layout number mismatch, or the handle was destroyed)");
    return Refusal{ATACOM_POINT_OK, std::string()};
}

static Refusal check_net_fits(const atacom_point_handle* h, const atacom_mlp* net, const std::string& w) {
    const int obs_dim = 4 * (1 + h->cfg.n_objects);
    if (net->n_in != obs_dim)
        return refuse(ATACOM_POINT_E_UNSUPPORTED, w + ": n_in = " + dec(net->n_in) + " but the handle's observation has " + dec(obs_dim) +
                                                    " components (n_objects = " + dec(h->cfg.n_objects) + ")");
    return Refusal{ATACOM_POINT_OK, std::string()};
}

// ------------------------------------------------------------------ launcher
// One launch of k_point_rollout_mlp<T, N> for the (dtype, n_objects) of `c`.  net == nullptr: pre-generated actions `acts_in`
// (records only).  rec != nullptr: packed records with the env-axis stride rec_ld, the six array pointers unused.
// Returns ATACOM_POINT_E_UNSUPPORTED for a combination that is not compiled in, else ATACOM_POINT_OK (the launch itself
// is checked by the caller through hipGetLastError).
int point_policy_launch(const atacom_point_config& c, int n_steps, const atacom_mlp* net, void* f, int* ip,
                        const void* acts_in, const void* noise, const void* draws, void* obs, void* nobs, void* acts_out,
                        void* rew, uint8_t* ab, uint8_t* last, void* rec, int rec_ld, hipStream_t s);

}  // namespace atacom_point
