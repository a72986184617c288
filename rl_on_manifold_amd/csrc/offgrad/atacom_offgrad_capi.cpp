// C-ABI host side of libatacom_offgrad.so (see include/atacom_offgrad_hip.h).  No handle: the device index travels in the
// call's argument struct.  Validates, then dispatches to the launchers; contains no numerics.  The words of a refusal are those
// of libatacom_offpolicy.so and libatacom_fit.so wherever the libraries ask the same thing.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "atacom_offgrad.h"
#define ATACOM_CAPI_E_HIP ATACOM_OFFGRAD_E_HIP
#include "../atacom_capi_common.h"        // g_err, fail, HIP_TRY, DeviceGuard, ON_DEVICE
#include "../atacom_mlp_host.h"           // mlp_abi_copy
#define ATACOM_CAPI_E_INVALID ATACOM_OFFGRAD_E_INVALID
#define ATACOM_CAPI_LIB(X) ATACOM_OFFGRAD_##X
#include "../mlp/atacom_view_checks.h"   // dec, Extent, Named, extent, strided, flat, overlap, check_strides, check_row_stride, check_aligned,
                                          // check_overlaps, check_workspace, check_head

namespace {

constexpr int INVALID = ATACOM_OFFGRAD_E_INVALID, UNSUPPORTED = ATACOM_OFFGRAD_E_UNSUPPORTED;

int check_critic(const atacom_offgrad_critic& c, int esize, const std::string& w, atacom_offgrad::NetDesc* d) {
    if (c.kind != ATACOM_OFFGRAD_DDPG && c.kind != ATACOM_OFFGRAD_TD3)
        return fail(UNSUPPORTED, w + ": kind = " + dec(c.kind) + " (0 = DDPG, 1 = TD3)");
    if (c.n_obs < 1 || c.n_obs > ATACOM_OFFGRAD_MAX_IN)
        return fail(UNSUPPORTED, w + ": n_obs = " + dec(c.n_obs) + " is outside 1 .. " + dec(ATACOM_OFFGRAD_MAX_IN));
    if (c.n_act < 1 || c.n_act > ATACOM_OFFGRAD_MAX_ACT)
        return fail(UNSUPPORTED, w + ": n_act = " + dec(c.n_act) + " is outside 1 .. " + dec(ATACOM_OFFGRAD_MAX_ACT));
    const int n1 = c.kind == ATACOM_OFFGRAD_TD3 ? c.n_obs + c.n_act : c.n_obs;
    if (n1 > ATACOM_OFFGRAD_MAX_IN)
        return fail(UNSUPPORTED, w + ": n1 = n_obs + n_act = " + dec(n1) + " first-layer inputs exceed " + dec(ATACOM_OFFGRAD_MAX_IN));
    if (c.activation != 0 && c.activation != 1) return fail(UNSUPPORTED, w + ": activation = " + dec(c.activation) + " (0 = ReLU, 1 = tanh)");
    if (!c.W1 || !c.b1 || !c.W2 || !c.b2 || !c.W2a || !c.W3 || !c.b3)
        return fail(INVALID, w + ": null argument (a weight or bias of the critic)");
    const struct { const void* p; const char* name; } ptrs[10] = {{c.W1, "W1"}, {c.b1, "b1"}, {c.W2, "W2"}, {c.b2, "b2"}, {c.W2a, "W2a"},
                                                                  {c.W3, "W3"}, {c.b3, "b3"}, {c.obs_shift, "obs_shift"},
                                                                  {c.obs_scale, "obs_scale"}, {c.act_scale, "act_scale"}};
    for (const auto& q : ptrs)
        if (int rc = check_aligned(q.p, esize, q.name, w)) return rc;
    *d = atacom_offgrad::NetDesc{c.W1, c.b1, c.W2, c.b2, c.W2a, c.W3, c.b3, c.obs_shift, c.obs_scale, c.act_scale, n1, 1, c.activation, 0};
    return 0;
}

size_t workspace_bytes(int esize, int n_nets, int64_t partial, int64_t blocks) {
    const size_t raw = (size_t)n_nets * (size_t)blocks * (size_t)partial * (size_t)esize;
    return (raw + 255) / 256 * 256;
}

}  // namespace

extern "C" {

const char* atacom_offgrad_last_error(void) { return g_err.c_str(); }
const char* atacom_offgrad_version(void) { return "atacom_offgrad 1.0 (gfx950)"; }

size_t atacom_offgrad_workspace_size(int32_t dtype, int32_t n_nets, int32_t n_in, int32_t n_out, int32_t n_act, int64_t rows,
                                     int32_t n_blocks) {
    const std::string w = "atacom_offgrad_workspace_size";
    const auto no = [&](int code, const std::string& m) { fail(code, w + ": " + m); return (size_t)0; };
    if (dtype != ATACOM_OFFGRAD_F32 && dtype != ATACOM_OFFGRAD_F64) return no(UNSUPPORTED, "no kernel for dtype " + dec(dtype));
    if (n_nets != 1 && n_nets != 2) return no(INVALID, "n_nets = " + dec(n_nets) + " (1 or 2)");
    if (n_in < 1 || n_in > ATACOM_OFFGRAD_MAX_IN) return no(UNSUPPORTED, "n_in = " + dec(n_in) + " is outside 1 .. " + dec(ATACOM_OFFGRAD_MAX_IN));
    if (n_out < 1 || n_out > ATACOM_OFFGRAD_MAX_ACT) return no(UNSUPPORTED, "n_out = " + dec(n_out) + " is outside 1 .. " + dec(ATACOM_OFFGRAD_MAX_ACT));
    if (n_act < 0 || n_act > ATACOM_OFFGRAD_MAX_ACT) return no(UNSUPPORTED, "n_act = " + dec(n_act) + " is outside 0 .. " + dec(ATACOM_OFFGRAD_MAX_ACT));
    if (rows < 1 || rows > ATACOM_OFFGRAD_MAX_ROWS) return no(INVALID, "rows = " + dec(rows) + " is outside 1 .. " + dec(ATACOM_OFFGRAD_MAX_ROWS));
    if (n_blocks < 0 || n_blocks > ATACOM_OFFGRAD_MAX_BLOCKS)
        return no(INVALID, "n_blocks = " + dec(n_blocks) + " is outside 0 .. " + dec(ATACOM_OFFGRAD_MAX_BLOCKS));
    const bool f64 = dtype == ATACOM_OFFGRAD_F64;
    return workspace_bytes(f64 ? 8 : 4, n_nets, atacom_offgrad::partial_size(n_in, n_out, n_act),
                           atacom_offgrad::effective_blocks(n_blocks, rows, f64));
}

int atacom_offgrad_critic_gradient(const atacom_offgrad_critic_args* a) {
    const std::string w = "atacom_offgrad_critic_gradient";
    if (!a) return fail(INVALID, w + ": null argument");
    if (a->struct_size != sizeof(atacom_offgrad_critic_args))
        return fail(INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " + dec(sizeof(atacom_offgrad_critic_args)));
    int64_t rows = 0;
    if (int rc = check_head(a->device, a->dtype, a->n_blocks, a->n_outer, a->n_inner, a->idx, a->n_idx, w, &rows)) return rc;
    if (a->n_critics != 1 && a->n_critics != 2) return fail(INVALID, w + ": n_critics = " + dec(a->n_critics) + " (1 = DDPG, 2 = TD3)");
    const bool f64 = a->dtype == ATACOM_OFFGRAD_F64;
    const int esize = f64 ? 8 : 4;
    atacom_offgrad::CriticCall c = {};
    for (int j = 0; j < a->n_critics; ++j)
        if (int rc = check_critic(a->critics[j], esize, w + ": critics[" + dec(j) + "]", &c.net[j])) return rc;
    const atacom_offgrad_critic& c0 = a->critics[0];
    if (a->n_critics == 2) {
        const atacom_offgrad_critic& c1 = a->critics[1];
        if (c1.kind != c0.kind || c1.n_obs != c0.n_obs || c1.n_act != c0.n_act)
            return fail(INVALID, w + ": the two critics differ in kind, n_obs or n_act");
    }
    if (!a->obs.ptr) return fail(INVALID, w + ": null argument (obs)");
    if (!a->action.ptr) return fail(INVALID, w + ": null argument (action)");
    if (!a->target) return fail(INVALID, w + ": null argument (target)");
    for (int j = 0; j < a->n_critics; ++j)
        if (!a->grad[j] || !a->stats[j]) return fail(INVALID, w + ": null argument (grad[" + dec(j) + "] or stats[" + dec(j) + "])");
    const int64_t no = a->n_outer, ni = a->n_inner;
    const int D = c0.n_obs, k = c0.n_act, n1 = c.net[0].n1;
    if (int rc = check_aligned(a->obs.ptr, esize, "obs", w)) return rc;
    if (int rc = check_aligned(a->action.ptr, esize, "action", w)) return rc;
    if (int rc = check_aligned(a->target, esize, "target", w)) return rc;
    if (int rc = check_aligned(a->idx, 8, "idx", w)) return rc;
    for (int j = 0; j < a->n_critics; ++j) {
        if (int rc = check_aligned(a->grad[j], esize, "grad", w)) return rc;
        if (int rc = check_aligned(a->stats[j], esize, "stats", w)) return rc;
    }
    if (int rc = check_strides(a->obs, no, ni, D, "obs", w)) return rc;
    if (int rc = check_strides(a->action, no, ni, k, "action", w)) return rc;
    if (int rc = check_row_stride(rows, a->target_stride, 1, false, "target", w)) return rc;
    const int64_t blocks = atacom_offgrad::effective_blocks(a->n_blocks, rows, f64);
    const int64_t n_grad = atacom_offgrad::grad_size(n1, 1, k);
    const size_t need = workspace_bytes(esize, a->n_critics, n_grad + ATACOM_OFFGRAD_STATS, blocks);
    if (int rc = check_workspace(a->workspace, a->workspace_bytes, need, "atacom_offgrad_workspace_size", w)) return rc;
    std::vector<Named> ins = {extent(a->obs, no, ni, D, esize, "obs"), extent(a->action, no, ni, k, esize, "action"),
                               strided(a->target, rows, a->target_stride, 1, esize, "target")};
    if (a->idx) ins.push_back(flat(a->idx, a->n_idx * 8, "idx"));
    std::vector<Named> outs;
    for (int j = 0; j < a->n_critics; ++j) {
        outs.push_back(flat(a->grad[j], n_grad * esize, "grad[" + dec(j) + "]"));
        outs.push_back(flat(a->stats[j], ATACOM_OFFGRAD_STATS * esize, "stats[" + dec(j) + "]"));
    }
    outs.push_back(flat(a->workspace, (int64_t)need, "workspace"));
    if (int rc = check_overlaps(outs, ins, w)) return rc;

    c.dtype = a->dtype, c.n_nets = a->n_critics, c.kind = c0.kind, c.n_obs = D, c.n_act = k;
    c.n_rows = rows, c.n_inner = ni, c.idx = a->idx;
    c.obs = {a->obs.ptr, a->obs.stride_outer, a->obs.stride_inner};
    c.action = {a->action.ptr, a->action.stride_outer, a->action.stride_inner};
    c.target = a->target, c.target_stride = a->target_stride, c.workspace = a->workspace;
    for (int j = 0; j < 2; ++j) c.grad[j] = a->grad[j < a->n_critics ? j : 0], c.stats[j] = a->stats[j < a->n_critics ? j : 0];
    ON_DEVICE(a);
    if (atacom_offgrad::critic_launch(c, (int)blocks, (hipStream_t)a->stream)) return fail(UNSUPPORTED, w + ": no kernel for this call");
    HIP_TRY(hipGetLastError());
    return ATACOM_OFFGRAD_OK;
}

int atacom_offgrad_actor_gradient(const atacom_offgrad_actor_args* a) {
    const std::string w = "atacom_offgrad_actor_gradient";
    if (!a) return fail(INVALID, w + ": null argument");
    if (a->struct_size != sizeof(atacom_offgrad_actor_args))
        return fail(INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " + dec(sizeof(atacom_offgrad_actor_args)));
    int64_t rows = 0;
    if (int rc = check_head(a->device, a->dtype, a->n_blocks, a->n_outer, a->n_inner, a->idx, a->n_idx, w, &rows)) return rc;
    const bool f64 = a->dtype == ATACOM_OFFGRAD_F64;
    const int esize = f64 ? 8 : 4;
    atacom_offgrad::ActorCall c = {};
    if (int rc = check_critic(a->critic, esize, w + ": critic", &c.critic)) return rc;
    const atacom_offgrad_critic& c0 = a->critic;
    // ---- the actor
    atacom_mlp net;
    if (!atacom::mlp_abi_copy(&a->actor, &net))
        return fail(INVALID, w + ": actor.struct_size = " + dec(a->actor.struct_size) + ", this library expects " + dec(sizeof(atacom_mlp)) +
                                 " or " + dec(ATACOM_MLP_SIZE_V1));
    if (net.hidden != ATACOM_OFFGRAD_HIDDEN) return fail(UNSUPPORTED, w + ": actor: hidden = " + dec(net.hidden) + ", only 64 hidden units are supported");
    if (net.n_in != c0.n_obs || net.n_out != c0.n_act)
        return fail(INVALID, w + ": the actor maps " + dec(net.n_in) + " to " + dec(net.n_out) + " where the critic takes n_obs = " +
                                 dec(c0.n_obs) + ", n_act = " + dec(c0.n_act));
    if (net.activation != 0 && net.activation != 1) return fail(UNSUPPORTED, w + ": actor: activation = " + dec(net.activation) + " (0 = ReLU, 1 = tanh)");
    if (!net.W1 || !net.b1 || !net.W2 || !net.b2 || !net.W3 || !net.b3) return fail(INVALID, w + ": null argument (a weight or bias of the actor)");
    if (net.sW1 || net.sb1 || net.sW2 || net.sb2 || net.sW3 || net.sb3) return fail(UNSUPPORTED, w + ": a sigma network is not supported");
    if (net.squash) return fail(UNSUPPORTED, w + ": squash is not supported (SAC is out of scope)");
    if (net.mean_mode != 0 && net.mean_mode != 1) return fail(UNSUPPORTED, w + ": mean_mode = " + dec(net.mean_mode) + " is not supported");
    const struct { const void* p; const char* name; } ptrs[9] = {{net.W1, "actor.W1"}, {net.b1, "actor.b1"}, {net.W2, "actor.W2"},
                                                                 {net.b2, "actor.b2"}, {net.W3, "actor.W3"}, {net.b3, "actor.b3"},
                                                                 {net.obs_shift, "actor.obs_shift"}, {net.obs_scale, "actor.obs_scale"},
                                                                 {net.mean_mode ? net.act_scale : nullptr, "actor.act_scale"}};
    for (const auto& q : ptrs)
        if (int rc = check_aligned(q.p, esize, q.name, w)) return rc;
    c.actor = atacom_offgrad::NetDesc{net.W1, net.b1, net.W2, net.b2, nullptr, net.W3, net.b3, net.obs_shift, net.obs_scale,
                                      net.mean_mode ? net.act_scale : nullptr, net.n_in, net.n_out, net.activation, net.mean_mode};
    // ---- the views and the outputs
    if (!a->obs.ptr) return fail(INVALID, w + ": null argument (obs)");
    if (!a->grad || !a->stats) return fail(INVALID, w + ": null argument (grad or stats)");
    const int64_t no = a->n_outer, ni = a->n_inner;
    const int D = c0.n_obs, k = c0.n_act;
    if (int rc = check_aligned(a->obs.ptr, esize, "obs", w)) return rc;
    if (int rc = check_aligned(a->idx, 8, "idx", w)) return rc;
    if (int rc = check_aligned(a->grad, esize, "grad", w)) return rc;
    if (int rc = check_aligned(a->stats, esize, "stats", w)) return rc;
    if (int rc = check_aligned(a->action_out, esize, "action_out", w)) return rc;
    if (int rc = check_aligned(a->dqda_out, esize, "dqda_out", w)) return rc;
    if (int rc = check_strides(a->obs, no, ni, D, "obs", w)) return rc;
    if (a->action_out)
        if (int rc = check_row_stride(rows, a->action_out_stride, k, true, "action_out", w)) return rc;
    if (a->dqda_out)
        if (int rc = check_row_stride(rows, a->dqda_out_stride, k, true, "dqda_out", w)) return rc;
    const int64_t blocks = atacom_offgrad::effective_blocks(a->n_blocks, rows, f64);
    const int64_t n_grad = atacom_offgrad::grad_size(D, k, 0);
    const size_t need = workspace_bytes(esize, 1, n_grad + ATACOM_OFFGRAD_STATS, blocks);
    if (int rc = check_workspace(a->workspace, a->workspace_bytes, need, "atacom_offgrad_workspace_size", w)) return rc;
    std::vector<Named> ins = {extent(a->obs, no, ni, D, esize, "obs")};
    if (a->idx) ins.push_back(flat(a->idx, a->n_idx * 8, "idx"));
    std::vector<Named> outs = {flat(a->grad, n_grad * esize, "grad"), flat(a->stats, ATACOM_OFFGRAD_STATS * esize, "stats")};
    if (a->action_out) outs.push_back(strided(a->action_out, rows, a->action_out_stride, k, esize, "action_out"));
    if (a->dqda_out) outs.push_back(strided(a->dqda_out, rows, a->dqda_out_stride, k, esize, "dqda_out"));
    outs.push_back(flat(a->workspace, (int64_t)need, "workspace"));
    if (int rc = check_overlaps(outs, ins, w)) return rc;

    c.dtype = a->dtype, c.kind = c0.kind, c.n_obs = D, c.n_act = k, c.n_rows = rows, c.n_inner = ni, c.idx = a->idx;
    c.obs = {a->obs.ptr, a->obs.stride_outer, a->obs.stride_inner};
    c.grad = a->grad, c.stats = a->stats, c.workspace = a->workspace;
    c.action_out = a->action_out, c.action_out_stride = a->action_out_stride;
    c.dqda_out = a->dqda_out, c.dqda_out_stride = a->dqda_out_stride;
    ON_DEVICE(a);
    if (atacom_offgrad::actor_launch(c, (int)blocks, (hipStream_t)a->stream)) return fail(UNSUPPORTED, w + ": no kernel for this call");
    HIP_TRY(hipGetLastError());
    return ATACOM_OFFGRAD_OK;
}

}  // extern "C"
