// C-ABI host side of libatacom_optim.so (see include/atacom_optim_hip.h).  No handle: the device index travels in the call's
// argument struct.  Validates, then dispatches to the launcher; contains no numerics.  The words of a refusal are those of
// atacom_fit_capi.cpp wherever the two libraries ask the same thing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "atacom_optim.h"
#define ATACOM_CAPI_E_HIP ATACOM_OPTIM_E_HIP
#include "../atacom_capi_common.h"   // g_err, fail, HIP_TRY, DeviceGuard, ON_DEVICE

namespace {

std::string dec(long long v) { return std::to_string(v); }

// [lo, hi) in bytes
struct Extent {
    intptr_t lo, hi;
    std::string name;
};

bool overlap(const Extent& a, const Extent& b) { return a.lo < b.hi && b.lo < a.hi; }

int check_shape(int32_t dtype, int32_t n_in, int32_t n_out, const std::string& w) {
    if (dtype != ATACOM_OPTIM_F32 && dtype != ATACOM_OPTIM_F64)
        return fail(ATACOM_OPTIM_E_UNSUPPORTED, w + ": no kernel for dtype " + dec(dtype));
    if (n_in < 1 || n_in > ATACOM_OPTIM_MAX_IN)
        return fail(ATACOM_OPTIM_E_UNSUPPORTED, w + ": n_in = " + dec(n_in) + " is outside 1 .. " + dec(ATACOM_OPTIM_MAX_IN));
    if (n_out < 1 || n_out > ATACOM_OPTIM_MAX_OUT)
        return fail(ATACOM_OPTIM_E_UNSUPPORTED, w + ": n_out = " + dec(n_out) + " is outside 1 .. " + dec(ATACOM_OPTIM_MAX_OUT));
    return ATACOM_OPTIM_OK;
}

// Everything a step asks of its arguments; init asks the same of the struct it shares with the steps, except a gradient.
int check(const atacom_optim_args* a, const std::string& w, bool need_grad) {
    if (!a) return fail(ATACOM_OPTIM_E_INVALID, w + ": null argument");
    if (a->struct_size != sizeof(atacom_optim_args))
        return fail(ATACOM_OPTIM_E_INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " + dec(sizeof(atacom_optim_args)));
    if (a->device < 0) return fail(ATACOM_OPTIM_E_INVALID, w + ": device = " + dec(a->device));
    if (a->n_groups < 1 || a->n_groups > ATACOM_OPTIM_MAX_GROUPS)
        return fail(ATACOM_OPTIM_E_INVALID, w + ": n_groups = " + dec(a->n_groups) + " is outside 1 .. " + dec(ATACOM_OPTIM_MAX_GROUPS));
    if (a->dtype != ATACOM_OPTIM_F32 && a->dtype != ATACOM_OPTIM_F64)
        return fail(ATACOM_OPTIM_E_UNSUPPORTED, w + ": no kernel for dtype " + dec(a->dtype));
    const struct { const char* name; double v; } betas[2] = {{"beta1", a->beta1}, {"beta2", a->beta2}};
    for (const auto& b : betas)
        if (!(b.v >= 0.0 && b.v < 1.0)) return fail(ATACOM_OPTIM_E_INVALID, w + ": " + b.name + " must be in [0, 1), got " + std::to_string(b.v));
    if (!(a->eps > 0.0) || !std::isfinite(a->eps)) return fail(ATACOM_OPTIM_E_INVALID, w + ": eps must be > 0 and finite, got " + std::to_string(a->eps));
    const int esize = a->dtype == ATACOM_OPTIM_F64 ? 8 : 4;
    std::vector<Extent> ext;
    for (int k = 0; k < a->n_groups; ++k) {
        const atacom_optim_group& g = a->groups[k];
        const std::string gw = w + ": groups[" + dec(k) + "]";
        if (int rc = check_shape(a->dtype, g.n_in, g.n_out, gw)) return rc;
        if (!g.W1 || !g.b1 || !g.W2 || !g.b2 || !g.W3 || !g.b3)
            return fail(ATACOM_OPTIM_E_INVALID, gw + ": null argument (a weight or bias of the network)");
        if ((need_grad && !g.grad) || !g.state) return fail(ATACOM_OPTIM_E_INVALID, gw + ": null argument (grad or state)");
        if (g.std && !g.log_std) return fail(ATACOM_OPTIM_E_INVALID, gw + ": std without log_std");
        if (!(g.lr >= 0.0) || !std::isfinite(g.lr)) return fail(ATACOM_OPTIM_E_INVALID, gw + ": lr must be >= 0 and finite, got " + std::to_string(g.lr));
        if (!std::isfinite(g.grad_scale)) return fail(ATACOM_OPTIM_E_INVALID, gw + ": grad_scale must be finite, got " + std::to_string(g.grad_scale));
        if ((intptr_t)g.state % 8) return fail(ATACOM_OPTIM_E_INVALID, gw + ": state must be aligned to 8 bytes");
        int n[atacom_optim::kSegments];
        const int64_t N = atacom_optim::segments(g.n_in, g.n_out, g.log_std != nullptr, n);
        const struct { const char* name; const void* p; int64_t bytes; } named[10] = {
            {"W1", g.W1, (int64_t)n[0] * esize}, {"b1", g.b1, (int64_t)n[1] * esize}, {"W2", g.W2, (int64_t)n[2] * esize},
            {"b2", g.b2, (int64_t)n[3] * esize}, {"W3", g.W3, (int64_t)n[4] * esize}, {"b3", g.b3, (int64_t)n[5] * esize},
            {"log_std", g.log_std, (int64_t)n[6] * esize}, {"std", g.std, (int64_t)g.n_out * esize}, {"grad", g.grad, N * esize},
            {"state", g.state, atacom_optim::state_bytes(g.n_in, g.n_out, g.log_std != nullptr, esize == 8)}};
        for (const auto& e : named) {
            if (!e.p) continue;
            if ((intptr_t)e.p % esize) return fail(ATACOM_OPTIM_E_INVALID, gw + ": " + e.name + " must be aligned to the dtype");
            ext.push_back({(intptr_t)e.p, (intptr_t)e.p + (intptr_t)e.bytes, "groups[" + dec(k) + "]." + e.name});
        }
    }
    for (size_t i = 0; i < ext.size(); ++i)
        for (size_t j = 0; j < i; ++j)
            if (overlap(ext[i], ext[j])) return fail(ATACOM_OPTIM_E_INVALID, w + ": " + ext[j].name + " overlaps " + ext[i].name);
    return ATACOM_OPTIM_OK;
}

}  // namespace

extern "C" {

const char* atacom_optim_last_error(void) { return g_err.c_str(); }
const char* atacom_optim_version(void) { return "atacom_optim 1.0 (gfx950)"; }

size_t atacom_optim_state_size(int32_t dtype, int32_t n_in, int32_t n_out, int32_t has_log_std) {
    if (check_shape(dtype, n_in, n_out, "atacom_optim_state_size")) return 0;
    return (size_t)atacom_optim::state_bytes(n_in, n_out, has_log_std != 0, dtype == ATACOM_OPTIM_F64);
}

int atacom_optim_adam_init(const atacom_optim_args* a) {
    if (int rc = check(a, "atacom_optim_adam_init", false)) return rc;
    ON_DEVICE(a);
    atacom_optim::init_launch(*a, (hipStream_t)a->stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OPTIM_OK;
}

int atacom_optim_adam_step(const atacom_optim_args* a) {
    if (int rc = check(a, "atacom_optim_adam_step", true)) return rc;
    ON_DEVICE(a);
    atacom_optim::step_launch(*a, (hipStream_t)a->stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OPTIM_OK;
}

}  // extern "C"
