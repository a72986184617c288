// C-ABI host side of libatacom_soft.so (see include/atacom_soft_hip.h).  No handle: the device index travels in the call's
// argument struct.  Validates, then dispatches to the launchers; contains no numerics.  The words of a refusal are those of
// libatacom_offgrad.so wherever the libraries ask the same thing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "atacom_soft.h"
#define ATACOM_CAPI_E_HIP ATACOM_SOFT_E_HIP
#include "../atacom_capi_common.h"        // g_err, fail, HIP_TRY, DeviceGuard, ON_DEVICE
#include "../atacom_mlp_host.h"           // mlp_abi_copy
#define ATACOM_CAPI_E_INVALID ATACOM_SOFT_E_INVALID
#define ATACOM_CAPI_LIB(X) ATACOM_SOFT_##X
#include "../mlp/atacom_view_checks.h"   // dec, Extent, Named, extent, strided, flat, overlap, check_strides, check_row_stride, check_aligned,
                                          // check_overlaps, check_workspace, check_head

namespace {

constexpr int INVALID = ATACOM_SOFT_E_INVALID, UNSUPPORTED = ATACOM_SOFT_E_UNSUPPORTED;

// what every row call shares, and the alignment of idx.  *rows = M.
int check_row_head(int32_t device, int32_t dtype, int32_t n_blocks, int64_t n_outer, int64_t n_inner, const int64_t* idx, int64_t n_idx,
                   const std::string& w, int64_t* rows) {
    if (int rc = check_head(device, dtype, n_blocks, n_outer, n_inner, idx, n_idx, w, rows)) return rc;
    if ((intptr_t)idx % 8) return fail(INVALID, w + ": idx must be aligned to the dtype");
    return 0;
}

int check_critic(const atacom_soft_critic& c, int esize, const std::string& w, atacom_soft::NetDesc* d) {
    if (c.n_act < 1 || c.n_act > ATACOM_SOFT_MAX_ACT)
        return fail(UNSUPPORTED, w + ": n_act = " + dec(c.n_act) + " is outside 1 .. " + dec(ATACOM_SOFT_MAX_ACT));
    if (c.n_obs < 1 || c.n_obs > ATACOM_SOFT_MAX_IN)
        return fail(UNSUPPORTED, w + ": n_obs = " + dec(c.n_obs) + " is outside 1 .. " + dec(ATACOM_SOFT_MAX_IN));
    const int n1 = c.n_obs + c.n_act;
    if (n1 > ATACOM_SOFT_MAX_IN)
        return fail(UNSUPPORTED, w + ": n1 = n_obs + n_act = " + dec(n1) + " first-layer inputs exceed " + dec(ATACOM_SOFT_MAX_IN));
    if (c.activation != 0 && c.activation != 1) return fail(UNSUPPORTED, w + ": activation = " + dec(c.activation) + " (0 = ReLU, 1 = tanh)");
    if (!c.W1 || !c.b1 || !c.W2 || !c.b2 || !c.W3 || !c.b3) return fail(INVALID, w + ": null argument (a weight or bias of the critic)");
    const struct { const void* p; const char* name; } ptrs[8] = {{c.W1, "W1"}, {c.b1, "b1"}, {c.W2, "W2"}, {c.b2, "b2"}, {c.W3, "W3"},
                                                                 {c.b3, "b3"}, {c.obs_shift, "obs_shift"}, {c.obs_scale, "obs_scale"}};
    for (const auto& q : ptrs)
        if (int rc = check_aligned(q.p, esize, q.name, w)) return rc;
    *d = atacom_soft::NetDesc{c.W1, c.b1, c.W2, c.b2, c.W3, c.b3, c.obs_shift, c.obs_scale, n1, 1, c.activation};
    return 0;
}

int check_pair(const atacom_soft_critic (&cs)[2], int n, int esize, const std::string& w, atacom_soft::NetDesc* d) {
    for (int j = 0; j < n; ++j)
        if (int rc = check_critic(cs[j], esize, w + ": critics[" + dec(j) + "]", d + j)) return rc;
    if (n == 2 && (cs[1].n_obs != cs[0].n_obs || cs[1].n_act != cs[0].n_act)) return fail(INVALID, w + ": the two critics differ in n_obs or n_act");
    return 0;
}

// the squashed-Gaussian policy of a call against its critics: mu and sigma as NetDesc
int check_policy(const atacom_mlp& in, int D, int k, int esize, const std::string& w, atacom_soft::NetDesc* mu, atacom_soft::NetDesc* sigma,
                 double* lmin, double* lmax) {
    atacom_mlp net;
    if (!atacom::mlp_abi_copy(&in, &net))
        return fail(INVALID, w + ": policy.struct_size = " + dec(in.struct_size) + ", this library expects " + dec(sizeof(atacom_mlp)) + " or " +
                                 dec(ATACOM_MLP_SIZE_V1));
    if (net.hidden != ATACOM_SOFT_HIDDEN) return fail(UNSUPPORTED, w + ": policy: hidden = " + dec(net.hidden) + ", only 64 hidden units are supported");
    if (net.n_in != D || net.n_out != k)
        return fail(INVALID, w + ": the policy maps " + dec(net.n_in) + " to " + dec(net.n_out) + " where the critics take n_obs = " + dec(D) +
                                 ", n_act = " + dec(k));
    if (net.activation != 0 && net.activation != 1) return fail(UNSUPPORTED, w + ": policy: activation = " + dec(net.activation) + " (0 = ReLU, 1 = tanh)");
    if (!net.W1 || !net.b1 || !net.W2 || !net.b2 || !net.W3 || !net.b3) return fail(INVALID, w + ": null argument (a weight or bias of the mu network)");
    if (!net.sW1 || !net.sb1 || !net.sW2 || !net.sb2 || !net.sW3 || !net.sb3)
        return fail(UNSUPPORTED, w + ": a policy without a sigma network is not supported (SAC's squashed Gaussian needs one)");
    if (!net.squash) return fail(UNSUPPORTED, w + ": a policy without squash is not supported (SAC's squashed Gaussian needs squash = 1)");
    if (!(net.log_std_min < net.log_std_max)) return fail(INVALID, w + ": policy: log_std_min must be below log_std_max");
    const struct { const void* p; const char* name; } ptrs[14] = {
        {net.W1, "policy.W1"}, {net.b1, "policy.b1"}, {net.W2, "policy.W2"}, {net.b2, "policy.b2"}, {net.W3, "policy.W3"}, {net.b3, "policy.b3"},
        {net.sW1, "policy.sW1"}, {net.sb1, "policy.sb1"}, {net.sW2, "policy.sW2"}, {net.sb2, "policy.sb2"}, {net.sW3, "policy.sW3"},
        {net.sb3, "policy.sb3"}, {net.obs_shift, "policy.obs_shift"}, {net.obs_scale, "policy.obs_scale"}};
    for (const auto& q : ptrs)
        if (int rc = check_aligned(q.p, esize, q.name, w)) return rc;
    *mu = atacom_soft::NetDesc{net.W1, net.b1, net.W2, net.b2, net.W3, net.b3, net.obs_shift, net.obs_scale, D, k, net.activation};
    *sigma = atacom_soft::NetDesc{net.sW1, net.sb1, net.sW2, net.sb2, net.sW3, net.sb3, net.obs_shift, net.obs_scale, D, k, net.activation};
    *lmin = net.log_std_min, *lmax = net.log_std_max;
    return 0;
}

size_t workspace_bytes(int esize, int n_nets, int64_t partial, int64_t blocks) {
    const size_t raw = (size_t)n_nets * (size_t)blocks * (size_t)partial * (size_t)esize;
    return (raw + 255) / 256 * 256;
}

// an optional per-row output: alignment, stride, extent
int add_out(const void* p, int64_t rows, int64_t stride, int width, int esize, const char* name, const std::string& w, std::vector<Named>* outs) {
    if (!p) return 0;
    if (int rc = check_aligned(p, esize, name, w)) return rc;
    if (int rc = check_row_stride(rows, stride, width, true, name, w)) return rc;
    outs->push_back(strided(p, rows, stride, width, esize, name));
    return 0;
}

// eps, act_scale, act_shift, log_alpha of a call: presence, alignment and their extents as inputs
int check_squash(const void* eps, int64_t eps_stride, const void* act_scale, const void* act_shift, const void* log_alpha, int64_t rows, int k,
                 int esize, const std::string& w, std::vector<Named>* ins) {
    if (!eps) return fail(INVALID, w + ": null argument (eps)");
    if (!log_alpha) return fail(INVALID, w + ": null argument (log_alpha)");
    if (int rc = check_aligned(eps, esize, "eps", w)) return rc;
    if (int rc = check_aligned(act_scale, esize, "act_scale", w)) return rc;
    if (int rc = check_aligned(act_shift, esize, "act_shift", w)) return rc;
    if (int rc = check_aligned(log_alpha, esize, "log_alpha", w)) return rc;
    if (int rc = check_row_stride(rows, eps_stride, k, false, "eps", w)) return rc;
    ins->push_back(strided(eps, rows, eps_stride, k, esize, "eps"));
    ins->push_back(flat(log_alpha, esize, "log_alpha"));
    if (act_scale) ins->push_back(flat(act_scale, (int64_t)k * esize, "act_scale"));
    if (act_shift) ins->push_back(flat(act_shift, (int64_t)k * esize, "act_shift"));
    return 0;
}

atacom_soft::RowView view(const atacom_evaluate_view& v) { return {v.ptr, v.stride_outer, v.stride_inner}; }

}  // namespace

extern "C" {

const char* atacom_soft_last_error(void) { return g_err.c_str(); }
const char* atacom_soft_version(void) { return "atacom_soft 1.0 (gfx950)"; }

size_t atacom_soft_workspace_size(int32_t dtype, int32_t n_nets, int32_t n_in, int32_t n_out, int64_t rows, int32_t n_blocks) {
    const std::string w = "atacom_soft_workspace_size";
    const auto no = [&](int code, const std::string& m) { fail(code, w + ": " + m); return (size_t)0; };
    if (dtype != ATACOM_SOFT_F32 && dtype != ATACOM_SOFT_F64) return no(UNSUPPORTED, "no kernel for dtype " + dec(dtype));
    if (n_nets != 1 && n_nets != 2) return no(INVALID, "n_nets = " + dec(n_nets) + " (1 or 2)");
    if (n_in < 1 || n_in > ATACOM_SOFT_MAX_IN) return no(UNSUPPORTED, "n_in = " + dec(n_in) + " is outside 1 .. " + dec(ATACOM_SOFT_MAX_IN));
    if (n_out < 1 || n_out > ATACOM_SOFT_MAX_ACT) return no(UNSUPPORTED, "n_out = " + dec(n_out) + " is outside 1 .. " + dec(ATACOM_SOFT_MAX_ACT));
    if (rows < 1 || rows > ATACOM_SOFT_MAX_ROWS) return no(INVALID, "rows = " + dec(rows) + " is outside 1 .. " + dec(ATACOM_SOFT_MAX_ROWS));
    if (n_blocks < 0 || n_blocks > ATACOM_SOFT_MAX_BLOCKS)
        return no(INVALID, "n_blocks = " + dec(n_blocks) + " is outside 0 .. " + dec(ATACOM_SOFT_MAX_BLOCKS));
    const bool f64 = dtype == ATACOM_SOFT_F64;
    return workspace_bytes(f64 ? 8 : 4, n_nets, atacom_soft::partial_size(n_in, n_out), atacom_soft::effective_blocks(n_blocks, rows, f64));
}

int atacom_soft_target(const atacom_soft_target_args* a) {
    const std::string w = "atacom_soft_target";
    if (!a) return fail(INVALID, w + ": null argument");
    if (a->struct_size != sizeof(atacom_soft_target_args))
        return fail(INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " + dec(sizeof(atacom_soft_target_args)));
    int64_t rows = 0;
    if (int rc = check_row_head(a->device, a->dtype, a->n_blocks, a->n_outer, a->n_inner, a->idx, a->n_idx, w, &rows)) return rc;
    if (a->n_critics != 2) return fail(UNSUPPORTED, w + ": n_critics = " + dec(a->n_critics) + " (SAC has two critics)");
    const bool f64 = a->dtype == ATACOM_SOFT_F64;
    const int esize = f64 ? 8 : 4;
    atacom_soft::TargetCall c = {};
    if (int rc = check_pair(a->critics, 2, esize, w, c.critic)) return rc;
    const int D = a->critics[0].n_obs, k = a->critics[0].n_act;
    if (int rc = check_policy(a->policy, D, k, esize, w, &c.mu, &c.sigma, &c.log_std_min, &c.log_std_max)) return rc;
    if (!std::isfinite(a->gamma)) return fail(INVALID, w + ": gamma must be finite");
    if (!a->next_obs.ptr || !a->reward.ptr || !a->absorbing.ptr) return fail(INVALID, w + ": null argument (next_obs, reward or absorbing)");
    if (!a->y) return fail(INVALID, w + ": null argument (y)");
    const int64_t no = a->n_outer, ni = a->n_inner;
    if (int rc = check_aligned(a->next_obs.ptr, esize, "next_obs", w)) return rc;
    if (int rc = check_aligned(a->reward.ptr, esize, "reward", w)) return rc;
    if (int rc = check_aligned(a->absorbing.ptr, esize, "absorbing", w)) return rc;
    if (int rc = check_strides(a->next_obs, no, ni, D, "next_obs", w)) return rc;
    std::vector<Named> ins = {extent(a->next_obs, no, ni, D, esize, "next_obs"), extent(a->reward, no, ni, 1, esize, "reward"),
                               extent(a->absorbing, no, ni, 1, esize, "absorbing")};
    if (int rc = check_squash(a->eps, a->eps_stride, a->act_scale, a->act_shift, a->log_alpha, rows, k, esize, w, &ins)) return rc;
    if (a->idx) ins.push_back(flat(a->idx, a->n_idx * 8, "idx"));
    std::vector<Named> outs;
    if (int rc = add_out(a->y, rows, a->y_stride, 1, esize, "y", w, &outs)) return rc;
    if (int rc = add_out(a->action_out, rows, a->action_out_stride, k, esize, "action_out", w, &outs)) return rc;
    if (int rc = add_out(a->logp_out, rows, a->logp_out_stride, 1, esize, "logp_out", w, &outs)) return rc;
    if (int rc = check_overlaps(outs, ins, w)) return rc;
    const int64_t blocks = atacom_soft::effective_blocks(a->n_blocks, rows, f64);

    c.dtype = a->dtype, c.n_obs = D, c.n_act = k, c.n_rows = rows, c.n_inner = ni, c.idx = a->idx;
    c.obs = view(a->next_obs), c.reward = view(a->reward), c.absorbing = view(a->absorbing);
    c.eps = a->eps, c.eps_stride = a->eps_stride, c.act_scale = a->act_scale, c.act_shift = a->act_shift, c.log_alpha = a->log_alpha;
    c.gamma = a->gamma;
    c.y = a->y, c.y_stride = a->y_stride, c.action_out = a->action_out, c.action_out_stride = a->action_out_stride;
    c.logp_out = a->logp_out, c.logp_out_stride = a->logp_out_stride;
    ON_DEVICE(a);
    if (atacom_soft::target_launch(c, (int)blocks, (hipStream_t)a->stream)) return fail(UNSUPPORTED, w + ": no kernel for this call");
    HIP_TRY(hipGetLastError());
    return ATACOM_SOFT_OK;
}

int atacom_soft_critic_gradient(const atacom_soft_critic_args* a) {
    const std::string w = "atacom_soft_critic_gradient";
    if (!a) return fail(INVALID, w + ": null argument");
    if (a->struct_size != sizeof(atacom_soft_critic_args))
        return fail(INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " + dec(sizeof(atacom_soft_critic_args)));
    int64_t rows = 0;
    if (int rc = check_row_head(a->device, a->dtype, a->n_blocks, a->n_outer, a->n_inner, a->idx, a->n_idx, w, &rows)) return rc;
    if (a->n_critics != 1 && a->n_critics != 2) return fail(INVALID, w + ": n_critics = " + dec(a->n_critics) + " (1 or 2)");
    const bool f64 = a->dtype == ATACOM_SOFT_F64;
    const int esize = f64 ? 8 : 4;
    atacom_soft::CriticCall c = {};
    if (int rc = check_pair(a->critics, a->n_critics, esize, w, c.net)) return rc;
    if (!a->obs.ptr) return fail(INVALID, w + ": null argument (obs)");
    if (!a->action.ptr) return fail(INVALID, w + ": null argument (action)");
    if (!a->target) return fail(INVALID, w + ": null argument (target)");
    for (int j = 0; j < a->n_critics; ++j)
        if (!a->grad[j] || !a->stats[j]) return fail(INVALID, w + ": null argument (grad[" + dec(j) + "] or stats[" + dec(j) + "])");
    const int64_t no = a->n_outer, ni = a->n_inner;
    const int D = a->critics[0].n_obs, k = a->critics[0].n_act, n1 = D + k;
    if (int rc = check_aligned(a->obs.ptr, esize, "obs", w)) return rc;
    if (int rc = check_aligned(a->action.ptr, esize, "action", w)) return rc;
    if (int rc = check_aligned(a->target, esize, "target", w)) return rc;
    for (int j = 0; j < a->n_critics; ++j) {
        if (int rc = check_aligned(a->grad[j], esize, "grad", w)) return rc;
        if (int rc = check_aligned(a->stats[j], esize, "stats", w)) return rc;
    }
    if (int rc = check_strides(a->obs, no, ni, D, "obs", w)) return rc;
    if (int rc = check_strides(a->action, no, ni, k, "action", w)) return rc;
    if (int rc = check_row_stride(rows, a->target_stride, 1, false, "target", w)) return rc;
    const int64_t blocks = atacom_soft::effective_blocks(a->n_blocks, rows, f64);
    const int64_t n_grad = atacom_soft::grad_size(n1, 1);
    const size_t need = workspace_bytes(esize, a->n_critics, n_grad + ATACOM_SOFT_STATS, blocks);
    if (int rc = check_workspace(a->workspace, a->workspace_bytes, need, "atacom_soft_workspace_size", w)) return rc;
    std::vector<Named> ins = {extent(a->obs, no, ni, D, esize, "obs"), extent(a->action, no, ni, k, esize, "action"),
                               strided(a->target, rows, a->target_stride, 1, esize, "target")};
    if (a->idx) ins.push_back(flat(a->idx, a->n_idx * 8, "idx"));
    std::vector<Named> outs;
    for (int j = 0; j < a->n_critics; ++j) {
        outs.push_back(flat(a->grad[j], n_grad * esize, "grad[" + dec(j) + "]"));
        outs.push_back(flat(a->stats[j], ATACOM_SOFT_STATS * esize, "stats[" + dec(j) + "]"));
    }
    outs.push_back(flat(a->workspace, (int64_t)need, "workspace"));
    if (int rc = check_overlaps(outs, ins, w)) return rc;

    c.dtype = a->dtype, c.n_nets = a->n_critics, c.n_obs = D, c.n_act = k, c.n_rows = rows, c.n_inner = ni, c.idx = a->idx;
    c.obs = view(a->obs), c.action = view(a->action);
    c.target = a->target, c.target_stride = a->target_stride, c.workspace = a->workspace;
    for (int j = 0; j < 2; ++j) c.grad[j] = a->grad[j < a->n_critics ? j : 0], c.stats[j] = a->stats[j < a->n_critics ? j : 0];
    ON_DEVICE(a);
    if (atacom_soft::critic_launch(c, (int)blocks, (hipStream_t)a->stream)) return fail(UNSUPPORTED, w + ": no kernel for this call");
    HIP_TRY(hipGetLastError());
    return ATACOM_SOFT_OK;
}

int atacom_soft_actor_gradient(const atacom_soft_actor_args* a) {
    const std::string w = "atacom_soft_actor_gradient";
    if (!a) return fail(INVALID, w + ": null argument");
    if (a->struct_size != sizeof(atacom_soft_actor_args))
        return fail(INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " + dec(sizeof(atacom_soft_actor_args)));
    int64_t rows = 0;
    if (int rc = check_row_head(a->device, a->dtype, a->n_blocks, a->n_outer, a->n_inner, a->idx, a->n_idx, w, &rows)) return rc;
    const bool f64 = a->dtype == ATACOM_SOFT_F64;
    const int esize = f64 ? 8 : 4;
    atacom_soft::ActorCall c = {};
    if (int rc = check_pair(a->critics, 2, esize, w, c.critic)) return rc;
    const int D = a->critics[0].n_obs, k = a->critics[0].n_act;
    if (int rc = check_policy(a->policy, D, k, esize, w, &c.mu, &c.sigma, &c.log_std_min, &c.log_std_max)) return rc;
    if (!std::isfinite(a->target_entropy)) return fail(INVALID, w + ": target_entropy must be finite");
    if (!a->obs.ptr) return fail(INVALID, w + ": null argument (obs)");
    if (!a->grad_mu || !a->grad_sigma || !a->stats) return fail(INVALID, w + ": null argument (grad_mu, grad_sigma or stats)");
    const int64_t no = a->n_outer, ni = a->n_inner;
    if (int rc = check_aligned(a->obs.ptr, esize, "obs", w)) return rc;
    if (int rc = check_aligned(a->grad_mu, esize, "grad_mu", w)) return rc;
    if (int rc = check_aligned(a->grad_sigma, esize, "grad_sigma", w)) return rc;
    if (int rc = check_aligned(a->stats, esize, "stats", w)) return rc;
    if (int rc = check_strides(a->obs, no, ni, D, "obs", w)) return rc;
    std::vector<Named> ins = {extent(a->obs, no, ni, D, esize, "obs")};
    if (int rc = check_squash(a->eps, a->eps_stride, a->act_scale, a->act_shift, a->log_alpha, rows, k, esize, w, &ins)) return rc;
    if (a->idx) ins.push_back(flat(a->idx, a->n_idx * 8, "idx"));
    const int64_t blocks = atacom_soft::effective_blocks(a->n_blocks, rows, f64);
    const int64_t n_grad = atacom_soft::grad_size(D, k);
    const size_t need = workspace_bytes(esize, 2, n_grad + ATACOM_SOFT_STATS, blocks);
    if (int rc = check_workspace(a->workspace, a->workspace_bytes, need, "atacom_soft_workspace_size", w)) return rc;
    std::vector<Named> outs = {flat(a->grad_mu, n_grad * esize, "grad_mu"), flat(a->grad_sigma, n_grad * esize, "grad_sigma"),
                                flat(a->stats, ATACOM_SOFT_STATS * esize, "stats")};
    if (int rc = add_out(a->action_out, rows, a->action_out_stride, k, esize, "action_out", w, &outs)) return rc;
    if (int rc = add_out(a->logp_out, rows, a->logp_out_stride, 1, esize, "logp_out", w, &outs)) return rc;
    if (int rc = add_out(a->q_out, rows, a->q_out_stride, 2, esize, "q_out", w, &outs)) return rc;
    if (int rc = add_out(a->dqda_out, rows, a->dqda_out_stride, k, esize, "dqda_out", w, &outs)) return rc;
    outs.push_back(flat(a->workspace, (int64_t)need, "workspace"));
    if (int rc = check_overlaps(outs, ins, w)) return rc;

    c.dtype = a->dtype, c.n_obs = D, c.n_act = k, c.n_rows = rows, c.n_inner = ni, c.idx = a->idx;
    c.obs = view(a->obs);
    c.eps = a->eps, c.eps_stride = a->eps_stride, c.act_scale = a->act_scale, c.act_shift = a->act_shift, c.log_alpha = a->log_alpha;
    c.target_entropy = a->target_entropy;
    c.grad_mu = a->grad_mu, c.grad_sigma = a->grad_sigma, c.stats = a->stats, c.workspace = a->workspace;
    c.action_out = a->action_out, c.action_out_stride = a->action_out_stride, c.logp_out = a->logp_out, c.logp_out_stride = a->logp_out_stride;
    c.q_out = a->q_out, c.q_out_stride = a->q_out_stride, c.dqda_out = a->dqda_out, c.dqda_out_stride = a->dqda_out_stride;
    ON_DEVICE(a);
    if (atacom_soft::actor_launch(c, (int)blocks, (hipStream_t)a->stream)) return fail(UNSUPPORTED, w + ": no kernel for this call");
    HIP_TRY(hipGetLastError());
    return ATACOM_SOFT_OK;
}

int atacom_soft_alpha_step(const atacom_soft_alpha_args* a) {
    const std::string w = "atacom_soft_alpha_step";
    if (!a) return fail(INVALID, w + ": null argument");
    if (a->struct_size != sizeof(atacom_soft_alpha_args))
        return fail(INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " + dec(sizeof(atacom_soft_alpha_args)));
    if (a->device < 0) return fail(INVALID, w + ": device = " + dec(a->device));
    if (a->dtype != ATACOM_SOFT_F32 && a->dtype != ATACOM_SOFT_F64) return fail(UNSUPPORTED, w + ": no kernel for dtype " + dec(a->dtype));
    const int esize = a->dtype == ATACOM_SOFT_F64 ? 8 : 4;
    if (!a->log_alpha || !a->grad || !a->state) return fail(INVALID, w + ": null argument (log_alpha, grad or state)");
    if (int rc = check_aligned(a->log_alpha, esize, "log_alpha", w)) return rc;
    if (int rc = check_aligned(a->grad, esize, "grad", w)) return rc;
    if (int rc = check_aligned(a->state, 8, "state", w)) return rc;
    if (!(a->lr >= 0.0) || !std::isfinite(a->lr)) return fail(INVALID, w + ": lr must be >= 0 and finite");
    if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0)) return fail(INVALID, w + ": beta1 and beta2 must be in [0, 1)");
    if (!(a->eps > 0.0) || !std::isfinite(a->eps)) return fail(INVALID, w + ": eps must be > 0 and finite");
    const std::vector<Named> ins = {flat(a->grad, esize, "grad")};
    const std::vector<Named> outs = {flat(a->log_alpha, esize, "log_alpha"), flat(a->state, ATACOM_SOFT_ALPHA_STATE, "state")};
    if (int rc = check_overlaps(outs, ins, w)) return rc;
    atacom_soft::AlphaCall c = {a->dtype, a->log_alpha, a->grad, a->state, a->lr, a->beta1, a->beta2, a->eps};
    ON_DEVICE(a);
    if (atacom_soft::alpha_launch(c, (hipStream_t)a->stream)) return fail(UNSUPPORTED, w + ": no kernel for this call");
    HIP_TRY(hipGetLastError());
    return ATACOM_SOFT_OK;
}

}  // extern "C"
