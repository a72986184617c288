// C-ABI host side of libatacom_fit.so (see include/atacom_fit_hip.h).  No handle: the device index travels in the call's
// argument struct.  Validates, then dispatches to the launcher; contains no numerics.  The checks, their order and their words
// are those of atacom_evaluate_capi.cpp wherever the two libraries ask the same thing; the checks of the views are those of
// ../mlp/atacom_view_checks.h.
#include <hip/hip_runtime.h>

#include <string>

#include "atacom_fit.h"
#define ATACOM_CAPI_E_HIP ATACOM_FIT_E_HIP
#define ATACOM_CAPI_E_INVALID ATACOM_FIT_E_INVALID
#include "../atacom_capi_common.h"        // g_err, fail, HIP_TRY, DeviceGuard, ON_DEVICE
#include "../atacom_mlp_host.h"           // mlp_abi_copy
#include "../mlp/atacom_view_checks.h"    // dec, Extent, extent, flat, overlap, check_strides

namespace {

// Everything that decides the size of the workspace; *rows = M, *blocks = n_blocks_effective.
int check_sizes(const atacom_fit_args* a, const std::string& w, atacom_mlp* net, int64_t* rows, int64_t* blocks) {
    if (!a) return fail(ATACOM_FIT_E_INVALID, w + ": null argument");
    if (a->struct_size != sizeof(atacom_fit_args))
        return fail(ATACOM_FIT_E_INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " + dec(sizeof(atacom_fit_args)));
    if (a->device < 0) return fail(ATACOM_FIT_E_INVALID, w + ": device = " + dec(a->device));
    if (a->dtype != ATACOM_FIT_F32 && a->dtype != ATACOM_FIT_F64)
        return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": no kernel for dtype " + dec(a->dtype));
    if (a->head != ATACOM_FIT_VALUE && a->head != ATACOM_FIT_PPO_CLIP)
        return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": head = " + dec(a->head) + " (0 = value, 1 = PPO clip)");
    if (a->n_outer < 1) return fail(ATACOM_FIT_E_INVALID, w + ": n_outer must be >= 1, got " + dec(a->n_outer));
    if (a->n_inner < 1) return fail(ATACOM_FIT_E_INVALID, w + ": n_inner must be >= 1, got " + dec(a->n_inner));
    if (a->n_outer > ATACOM_FIT_MAX_ROWS / a->n_inner)
        return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": n_outer * n_inner = " + dec(a->n_outer) + " * " + dec(a->n_inner) +
                                                  " rows is too many (at most " + dec(ATACOM_FIT_MAX_ROWS) + " a call)");
    if (a->n_blocks < 0) return fail(ATACOM_FIT_E_INVALID, w + ": n_blocks must be >= 1, or 0 for the library's choice, got " + dec(a->n_blocks));
    if (a->n_blocks > ATACOM_FIT_MAX_BLOCKS)
        return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": n_blocks = " + dec(a->n_blocks) + " exceeds the launch grid (" + dec(ATACOM_FIT_MAX_BLOCKS) + ")");
    if (a->idx && a->n_idx < 1) return fail(ATACOM_FIT_E_INVALID, w + ": n_idx must be >= 1 with idx, got " + dec(a->n_idx));
    if (a->idx && a->n_idx > ATACOM_FIT_MAX_ROWS)
        return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": n_idx = " + dec(a->n_idx) + " rows is too many (at most " + dec(ATACOM_FIT_MAX_ROWS) + " a call)");
    // ---- the network
    if (!atacom::mlp_abi_copy(&a->net, net))
        return fail(ATACOM_FIT_E_INVALID, w + ": net.struct_size = " + dec(a->net.struct_size) + ", this library expects " +
                                              dec(sizeof(atacom_mlp)) + " or " + dec(ATACOM_MLP_SIZE_V1));
    if (net->hidden != ATACOM_FIT_HIDDEN)
        return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": hidden = " + dec(net->hidden) + ", only 64 hidden units are supported");
    if (net->n_in < 1 || net->n_in > ATACOM_FIT_MAX_IN)
        return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": n_in = " + dec(net->n_in) + " is outside 1 .. " + dec(ATACOM_FIT_MAX_IN));
    if (net->n_out < 1 || net->n_out > ATACOM_FIT_MAX_OUT)
        return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": n_out = " + dec(net->n_out) + " is outside 1 .. " + dec(ATACOM_FIT_MAX_OUT));
    if (a->head == ATACOM_FIT_VALUE && net->n_out != 1)
        return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": n_out = " + dec(net->n_out) + ", the value head fits a network of one output");
    *rows = a->idx ? a->n_idx : a->n_outer * a->n_inner;
    *blocks = atacom_fit::effective_blocks(a->n_blocks, *rows, a->dtype == ATACOM_FIT_F64);
    return ATACOM_FIT_OK;
}

size_t workspace_bytes(const atacom_fit_args* a, const atacom_mlp& net, int64_t blocks) {
    const size_t raw = (size_t)blocks * (size_t)atacom_fit::partial_size(net.n_in, net.n_out) * (a->dtype == ATACOM_FIT_F64 ? 8 : 4);
    return (raw + 255) / 256 * 256;
}

}  // namespace

extern "C" {

const char* atacom_fit_last_error(void) { return g_err.c_str(); }
const char* atacom_fit_version(void) { return "atacom_fit 1.0 (gfx950)"; }

size_t atacom_fit_workspace_size(const atacom_fit_args* a) {
    atacom_mlp net;
    int64_t rows = 0, blocks = 0;
    if (check_sizes(a, "atacom_fit_workspace_size", &net, &rows, &blocks)) return 0;
    return workspace_bytes(a, net, blocks);
}

int atacom_fit_gradient(const atacom_fit_args* a) {
    const std::string w = "atacom_fit_gradient";
    atacom_mlp net;
    int64_t rows = 0, blocks = 0;
    if (int rc = check_sizes(a, w, &net, &rows, &blocks)) return rc;
    const bool ppo = a->head == ATACOM_FIT_PPO_CLIP;
    if (net.activation != 0 && net.activation != 1)
        return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": activation = " + dec(net.activation) + " (0 = ReLU, 1 = tanh)");
    if (!net.W1 || !net.b1 || !net.W2 || !net.b2 || !net.W3 || !net.b3)
        return fail(ATACOM_FIT_E_INVALID, w + ": null argument (a weight or bias of the network)");
    if (net.sW1 || net.sb1 || net.sW2 || net.sb2 || net.sW3 || net.sb3)
        return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": a sigma network is not supported (the log-probability is that of a state-independent std)");
    if (net.squash) return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": squash is not supported (SAC's squashed log-probability is out of scope)");
    if (net.mean_mode) return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": mean_mode = " + dec(net.mean_mode) + " is not supported");
    if (net.explore) return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": explore = " + dec(net.explore) + " is not supported");
    // ---- the views
    if (!a->x.ptr) return fail(ATACOM_FIT_E_INVALID, w + ": null argument (x)");
    if (!a->weight.ptr) return fail(ATACOM_FIT_E_INVALID, w + ": null argument (weight)");
    if (!a->grad || !a->stats || !a->workspace) return fail(ATACOM_FIT_E_INVALID, w + ": null argument (grad, stats or workspace)");
    if (ppo && (!a->action.ptr || !a->logp_old.ptr || !net.std))
        return fail(ATACOM_FIT_E_INVALID, w + ": the PPO head needs action, logp_old and net.std");
    if (ppo && !(a->clip > 0.0)) return fail(ATACOM_FIT_E_INVALID, w + ": clip must be > 0, got " + std::to_string(a->clip));
    const int64_t no = a->n_outer, ni = a->n_inner;
    const int esize = a->dtype == ATACOM_FIT_F64 ? 8 : 4;
    if (int rc = check_strides(a->x, no, ni, net.n_in, "x", w)) return rc;
    if (int rc = check_strides(a->weight, no, ni, 1, "weight", w)) return rc;
    if (ppo) {
        if (int rc = check_strides(a->action, no, ni, net.n_out, "action", w)) return rc;
        if (int rc = check_strides(a->logp_old, no, ni, 1, "logp_old", w)) return rc;
    }
    const size_t need = workspace_bytes(a, net, blocks);
    if (a->workspace_bytes < need)
        return fail(ATACOM_FIT_E_INVALID, w + ": workspace_bytes = " + dec((long long)a->workspace_bytes) + " is below the " +
                                              dec((long long)need) + " that atacom_fit_workspace_size gives");
    const int64_t n_grad = atacom_fit::grad_size(net.n_in, net.n_out) + (ppo ? net.n_out : 0);
    const struct { const char* name; Extent e; } outs[3] = {{"grad", flat(a->grad, n_grad * esize)},
                                                            {"stats", flat(a->stats, ATACOM_FIT_STATS * esize)},
                                                            {"workspace", flat(a->workspace, (int64_t)need)}};
    const struct { const char* name; Extent e; bool used; } ins[5] = {
        {"x", extent(a->x, no, ni, net.n_in, esize), true},
        {"action", extent(a->action, no, ni, net.n_out, esize), ppo},
        {"weight", extent(a->weight, no, ni, 1, esize), true},
        {"logp_old", extent(a->logp_old, no, ni, 1, esize), ppo},
        {"idx", flat(a->idx, a->idx ? a->n_idx * 8 : 0), a->idx != nullptr}};
    for (int o = 0; o < 3; ++o) {
        for (const auto& in : ins)
            if (in.used && overlap(outs[o].e, in.e)) return fail(ATACOM_FIT_E_INVALID, w + ": " + outs[o].name + " overlaps " + in.name);
        for (int p = 0; p < o; ++p)
            if (overlap(outs[o].e, outs[p].e)) return fail(ATACOM_FIT_E_INVALID, w + ": " + outs[p].name + " overlaps " + outs[o].name);
    }

    ON_DEVICE(a);
    if (atacom_fit::fit_launch(*a, net, (int)blocks, rows, (hipStream_t)a->stream))
        return fail(ATACOM_FIT_E_UNSUPPORTED, w + ": no kernel for this call");
    HIP_TRY(hipGetLastError());
    return ATACOM_FIT_OK;
}

}  // extern "C"
