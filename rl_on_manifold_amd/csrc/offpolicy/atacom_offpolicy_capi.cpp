// C-ABI host side of libatacom_offpolicy.so (see include/atacom_offpolicy_hip.h).  No handle: the device index travels in the
// call's argument struct.  Validates, then dispatches to the launchers; contains no numerics.  The words of a refusal are those
// of atacom_fit_capi.cpp wherever the two libraries ask the same thing.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <string>
#include <vector>

#include "atacom_offpolicy.h"
#define ATACOM_CAPI_E_HIP ATACOM_OFFPOLICY_E_HIP
#include "../atacom_capi_common.h"        // g_err, fail, HIP_TRY, DeviceGuard, ON_DEVICE
#include "../atacom_mlp_host.h"           // mlp_abi_copy
#define ATACOM_CAPI_E_INVALID ATACOM_OFFPOLICY_E_INVALID
#define ATACOM_CAPI_LIB(X) ATACOM_OFFPOLICY_##X
#include "../mlp/atacom_view_checks.h"   // dec, Extent, Named, extent, strided, flat, overlap, check_strides, check_row_stride, check_aligned,
                                          // check_overlaps, check_workspace, check_head

namespace {

constexpr int INVALID = ATACOM_OFFPOLICY_E_INVALID, UNSUPPORTED = ATACOM_OFFPOLICY_E_UNSUPPORTED;

int check_critic(const atacom_offpolicy_critic& c, const std::string& w, atacom_offpolicy::NetDesc* d) {
    if (c.kind != ATACOM_OFFPOLICY_DDPG && c.kind != ATACOM_OFFPOLICY_TD3)
        return fail(UNSUPPORTED, w + ": kind = " + dec(c.kind) + " (0 = DDPG, 1 = TD3)");
    if (c.n_obs < 1 || c.n_obs > ATACOM_OFFPOLICY_MAX_IN)
        return fail(UNSUPPORTED, w + ": n_obs = " + dec(c.n_obs) + " is outside 1 .. " + dec(ATACOM_OFFPOLICY_MAX_IN));
    if (c.n_act < 1 || c.n_act > ATACOM_OFFPOLICY_MAX_ACT)
        return fail(UNSUPPORTED, w + ": n_act = " + dec(c.n_act) + " is outside 1 .. " + dec(ATACOM_OFFPOLICY_MAX_ACT));
    const int n1 = c.kind == ATACOM_OFFPOLICY_TD3 ? c.n_obs + c.n_act : c.n_obs;
    if (n1 > ATACOM_OFFPOLICY_MAX_IN)
        return fail(UNSUPPORTED, w + ": n1 = n_obs + n_act = " + dec(n1) + " first-layer inputs exceed " + dec(ATACOM_OFFPOLICY_MAX_IN));
    if (c.activation != 0 && c.activation != 1) return fail(UNSUPPORTED, w + ": activation = " + dec(c.activation) + " (0 = ReLU, 1 = tanh)");
    if (!c.W1 || !c.b1 || !c.W2 || !c.b2 || !c.W2a || !c.W3 || !c.b3)
        return fail(INVALID, w + ": null argument (a weight or bias of the critic)");
    *d = atacom_offpolicy::NetDesc{c.W1, c.b1, c.W2, c.b2, c.W2a, c.W3, c.b3, c.obs_shift, c.obs_scale, c.act_scale, n1, 1, c.activation, 0};
    return 0;
}

// compute units of a device, asked once
int compute_units(int device) {
    static std::atomic<int> cache[64];
    if (device < 64 && cache[device].load() > 0) return cache[device].load();
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n < 1) n = 256;
    if (device < 64) cache[device].store(n);
    return n;
}

// a q call stages once and a workgroup walks its tiles; a target call restages per tile, so it takes a workgroup per tile
int64_t choose_blocks(int32_t n_blocks, int64_t rows, bool f64, bool target, int device) {
    int64_t blocks = n_blocks;
    if (blocks == 0) {
        blocks = atacom_offpolicy::tiles(rows, f64);
        const int64_t fit = (int64_t)compute_units(device) * (f64 ? 1 : atacom_offpolicy::kResident);
        if (!target && blocks > fit) blocks = fit;
        if (blocks > ATACOM_OFFPOLICY_MAX_BLOCKS) blocks = ATACOM_OFFPOLICY_MAX_BLOCKS;
    }
    return blocks;
}

}  // namespace

extern "C" {

const char* atacom_offpolicy_last_error(void) { return g_err.c_str(); }
const char* atacom_offpolicy_version(void) { return "atacom_offpolicy 1.0 (gfx950)"; }

int atacom_offpolicy_q(const atacom_offpolicy_q_args* a) {
    const std::string w = "atacom_offpolicy_q";
    if (!a) return fail(INVALID, w + ": null argument");
    if (a->struct_size != sizeof(atacom_offpolicy_q_args))
        return fail(INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " + dec(sizeof(atacom_offpolicy_q_args)));
    int64_t rows = 0;
    if (int rc = check_head(a->device, a->dtype, a->n_blocks, a->n_outer, a->n_inner, a->idx, a->n_idx, w, &rows)) return rc;
    atacom_offpolicy::Call c = {};
    if (int rc = check_critic(a->critic, w + ": critic", &c.net[0])) return rc;
    if (!a->obs.ptr) return fail(INVALID, w + ": null argument (obs)");
    if (!a->action.ptr) return fail(INVALID, w + ": null argument (action)");
    if (!a->q) return fail(INVALID, w + ": null argument (q)");
    const int64_t no = a->n_outer, ni = a->n_inner;
    const int esize = a->dtype == ATACOM_OFFPOLICY_F64 ? 8 : 4, D = a->critic.n_obs, k = a->critic.n_act;
    if (int rc = check_strides(a->obs, no, ni, D, "obs", w)) return rc;
    if (int rc = check_strides(a->action, no, ni, k, "action", w)) return rc;
    if (int rc = check_row_stride(rows, a->q_stride, 1, true, "q", w)) return rc;
    std::vector<Named> ins = {extent(a->obs, no, ni, D, esize, "obs"), extent(a->action, no, ni, k, esize, "action")};
    if (a->idx) ins.push_back(flat(a->idx, a->n_idx * 8, "idx"));
    if (int rc = check_overlaps({strided(a->q, rows, a->q_stride, 1, esize, "q")}, ins, w)) return rc;

    c.dtype = a->dtype, c.has_actor = 0, c.n_nets = 1, c.kind = a->critic.kind, c.n_obs = D, c.n_act = k;
    c.n_rows = rows, c.n_inner = ni, c.idx = a->idx, c.obs = a->obs, c.action = a->action;
    c.y = a->q, c.y_stride = a->q_stride;
    ON_DEVICE(a);
    const int64_t blocks = choose_blocks(a->n_blocks, rows, esize == 8, false, a->device);
    if (atacom_offpolicy::net_launch(c, (int)blocks, (hipStream_t)a->stream)) return fail(UNSUPPORTED, w + ": no kernel for this call");
    HIP_TRY(hipGetLastError());
    return ATACOM_OFFPOLICY_OK;
}

int atacom_offpolicy_target(const atacom_offpolicy_target_args* a) {
    const std::string w = "atacom_offpolicy_target";
    if (!a) return fail(INVALID, w + ": null argument");
    if (a->struct_size != sizeof(atacom_offpolicy_target_args))
        return fail(INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " + dec(sizeof(atacom_offpolicy_target_args)));
    int64_t rows = 0;
    if (int rc = check_head(a->device, a->dtype, a->n_blocks, a->n_outer, a->n_inner, a->idx, a->n_idx, w, &rows)) return rc;
    if (a->n_critics != 1 && a->n_critics != 2) return fail(INVALID, w + ": n_critics = " + dec(a->n_critics) + " (1 = DDPG, 2 = TD3)");
    atacom_offpolicy::Call c = {};
    for (int j = 0; j < a->n_critics; ++j)
        if (int rc = check_critic(a->critics[j], w + ": critics[" + dec(j) + "]", &c.net[1 + j])) return rc;
    const atacom_offpolicy_critic& c0 = a->critics[0];
    if (a->n_critics == 2) {
        const atacom_offpolicy_critic& c1 = a->critics[1];
        if (c1.kind != c0.kind || c1.n_obs != c0.n_obs || c1.n_act != c0.n_act)
            return fail(INVALID, w + ": the two critics differ in kind, n_obs or n_act");
    }
    // ---- the actor
    atacom_mlp net;
    if (!atacom::mlp_abi_copy(&a->actor, &net))
        return fail(INVALID, w + ": actor.struct_size = " + dec(a->actor.struct_size) + ", this library expects " + dec(sizeof(atacom_mlp)) +
                                 " or " + dec(ATACOM_MLP_SIZE_V1));
    if (net.hidden != ATACOM_OFFPOLICY_HIDDEN) return fail(UNSUPPORTED, w + ": actor: hidden = " + dec(net.hidden) + ", only 64 hidden units are supported");
    if (net.n_in != c0.n_obs || net.n_out != c0.n_act)
        return fail(INVALID, w + ": the actor maps " + dec(net.n_in) + " to " + dec(net.n_out) + " where the critics take n_obs = " +
                                 dec(c0.n_obs) + ", n_act = " + dec(c0.n_act));
    if (net.activation != 0 && net.activation != 1) return fail(UNSUPPORTED, w + ": actor: activation = " + dec(net.activation) + " (0 = ReLU, 1 = tanh)");
    if (!net.W1 || !net.b1 || !net.W2 || !net.b2 || !net.W3 || !net.b3) return fail(INVALID, w + ": null argument (a weight or bias of the actor)");
    if (net.sW1 || net.sb1 || net.sW2 || net.sb2 || net.sW3 || net.sb3) return fail(UNSUPPORTED, w + ": a sigma network is not supported");
    if (net.squash) return fail(UNSUPPORTED, w + ": squash is not supported (SAC's entropy target is out of scope)");
    if (net.mean_mode != 0 && net.mean_mode != 1) return fail(UNSUPPORTED, w + ": mean_mode = " + dec(net.mean_mode) + " is not supported");
    c.net[0] = atacom_offpolicy::NetDesc{net.W1, net.b1, net.W2, net.b2, nullptr, net.W3, net.b3, net.obs_shift, net.obs_scale,
                                         net.mean_mode ? net.act_scale : nullptr, net.n_in, net.n_out, net.activation, net.mean_mode};
    // ---- the scalars
    if (!(a->noise_std >= 0.0) || !std::isfinite(a->noise_std)) return fail(INVALID, w + ": noise_std must be >= 0 and finite, got " + std::to_string(a->noise_std));
    if (!(a->noise_clip >= 0.0) || !std::isfinite(a->noise_clip)) return fail(INVALID, w + ": noise_clip must be >= 0 and finite, got " + std::to_string(a->noise_clip));
    if (!std::isfinite(a->gamma)) return fail(INVALID, w + ": gamma must be finite, got " + std::to_string(a->gamma));
    if ((a->act_low == nullptr) != (a->act_high == nullptr)) return fail(INVALID, w + ": act_low and act_high are given together or not at all");
    // ---- the views
    if (!a->next_obs.ptr || !a->reward.ptr || !a->absorbing.ptr) return fail(INVALID, w + ": null argument (next_obs, reward or absorbing)");
    if (!a->y) return fail(INVALID, w + ": null argument (y)");
    const int64_t no = a->n_outer, ni = a->n_inner;
    const int esize = a->dtype == ATACOM_OFFPOLICY_F64 ? 8 : 4, D = c0.n_obs, k = c0.n_act;
    if (int rc = check_strides(a->next_obs, no, ni, D, "next_obs", w)) return rc;
    if (int rc = check_strides(a->reward, no, ni, 1, "reward", w)) return rc;
    if (int rc = check_strides(a->absorbing, no, ni, 1, "absorbing", w)) return rc;
    if (a->eps)
        if (int rc = check_row_stride(rows, a->eps_stride, k, false, "eps", w)) return rc;
    if (int rc = check_row_stride(rows, a->y_stride, 1, true, "y", w)) return rc;
    if (a->action_out)
        if (int rc = check_row_stride(rows, a->action_out_stride, k, true, "action_out", w)) return rc;
    std::vector<Named> ins = {extent(a->next_obs, no, ni, D, esize, "next_obs"), extent(a->reward, no, ni, 1, esize, "reward"),
                               extent(a->absorbing, no, ni, 1, esize, "absorbing")};
    if (a->eps) ins.push_back(strided(a->eps, rows, a->eps_stride, k, esize, "eps"));
    if (a->idx) ins.push_back(flat(a->idx, a->n_idx * 8, "idx"));
    std::vector<Named> outs = {strided(a->y, rows, a->y_stride, 1, esize, "y")};
    if (a->action_out) outs.push_back(strided(a->action_out, rows, a->action_out_stride, k, esize, "action_out"));
    if (int rc = check_overlaps(outs, ins, w)) return rc;

    c.dtype = a->dtype, c.has_actor = 1, c.n_nets = 1 + a->n_critics, c.kind = c0.kind, c.n_obs = D, c.n_act = k;
    c.n_rows = rows, c.n_inner = ni, c.idx = a->idx, c.obs = a->next_obs, c.reward = a->reward, c.absorbing = a->absorbing;
    c.eps = a->eps, c.eps_stride = a->eps_stride, c.low = a->act_low, c.high = a->act_high;
    c.noise_std = a->noise_std, c.noise_clip = a->noise_clip, c.gamma = a->gamma;
    c.y = a->y, c.y_stride = a->y_stride, c.action_out = a->action_out, c.action_out_stride = a->action_out_stride;
    ON_DEVICE(a);
    const int64_t blocks = choose_blocks(a->n_blocks, rows, esize == 8, true, a->device);
    if (atacom_offpolicy::net_launch(c, (int)blocks, (hipStream_t)a->stream)) return fail(UNSUPPORTED, w + ": no kernel for this call");
    HIP_TRY(hipGetLastError());
    return ATACOM_OFFPOLICY_OK;
}

int atacom_offpolicy_soft_update(const atacom_offpolicy_soft_update_args* a) {
    const std::string w = "atacom_offpolicy_soft_update";
    static const char* const names[ATACOM_OFFPOLICY_TENSORS] = {"W1", "b1", "W2", "b2", "W3", "b3", "W2a"};
    if (!a) return fail(INVALID, w + ": null argument");
    if (a->struct_size != sizeof(atacom_offpolicy_soft_update_args))
        return fail(INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " + dec(sizeof(atacom_offpolicy_soft_update_args)));
    if (a->device < 0) return fail(INVALID, w + ": device = " + dec(a->device));
    if (a->dtype != ATACOM_OFFPOLICY_F32 && a->dtype != ATACOM_OFFPOLICY_F64) return fail(UNSUPPORTED, w + ": no kernel for dtype " + dec(a->dtype));
    if (a->n_pairs < 1 || a->n_pairs > ATACOM_OFFPOLICY_MAX_PAIRS)
        return fail(INVALID, w + ": n_pairs = " + dec(a->n_pairs) + " is outside 1 .. " + dec(ATACOM_OFFPOLICY_MAX_PAIRS));
    if (!(a->tau >= 0.0 && a->tau <= 1.0)) return fail(INVALID, w + ": tau must be in [0, 1], got " + std::to_string(a->tau));
    const int esize = a->dtype == ATACOM_OFFPOLICY_F64 ? 8 : 4;
    std::vector<Named> targets, onlines;
    for (int k = 0; k < a->n_pairs; ++k) {
        const atacom_offpolicy_pair& p = a->pairs[k];
        const std::string pw = "pairs[" + dec(k) + "]";
        if (p.n_in < 1 || p.n_in > ATACOM_OFFPOLICY_MAX_IN)
            return fail(UNSUPPORTED, w + ": " + pw + ": n_in = " + dec(p.n_in) + " is outside 1 .. " + dec(ATACOM_OFFPOLICY_MAX_IN));
        if (p.n_out < 1 || p.n_out > ATACOM_OFFPOLICY_MAX_ACT)
            return fail(UNSUPPORTED, w + ": " + pw + ": n_out = " + dec(p.n_out) + " is outside 1 .. " + dec(ATACOM_OFFPOLICY_MAX_ACT));
        if (p.n_act < 0 || p.n_act > ATACOM_OFFPOLICY_MAX_ACT)
            return fail(UNSUPPORTED, w + ": " + pw + ": n_act = " + dec(p.n_act) + " is outside 0 .. " + dec(ATACOM_OFFPOLICY_MAX_ACT));
        int n[ATACOM_OFFPOLICY_TENSORS];
        atacom_offpolicy::pair_sizes(p, n);
        for (int i = 0; i < ATACOM_OFFPOLICY_TENSORS; ++i) {
            if (n[i] == 0) continue;
            if (!p.target[i] || !p.online[i]) return fail(INVALID, w + ": " + pw + ": null argument (" + names[i] + ")");
            if ((intptr_t)p.target[i] % esize || (intptr_t)p.online[i] % esize)
                return fail(INVALID, w + ": " + pw + ": " + names[i] + " must be aligned to the dtype");
            targets.push_back(flat(p.target[i], (int64_t)n[i] * esize, pw + ".target." + names[i]));
            onlines.push_back(flat(p.online[i], (int64_t)n[i] * esize, pw + ".online." + names[i]));
        }
    }
    if (int rc = check_overlaps(targets, onlines, w)) return rc;
    ON_DEVICE(a);
    atacom_offpolicy::soft_update_launch(*a, (hipStream_t)a->stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OFFPOLICY_OK;
}

}  // extern "C"
