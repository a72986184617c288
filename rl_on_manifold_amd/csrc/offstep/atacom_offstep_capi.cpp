// C-ABI host side of libatacom_offstep.so (see include/atacom_offstep_hip.h).  No handle: the device index travels in the call's
// argument struct.  Validates, then dispatches to the launcher; contains no numerics.  The words of a refusal are those of
// atacom_optim_capi.cpp wherever the two libraries ask the same thing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "atacom_offstep.h"
#define ATACOM_CAPI_E_HIP ATACOM_OFFSTEP_E_HIP
#include "../atacom_capi_common.h"   // g_err, fail, HIP_TRY, DeviceGuard, ON_DEVICE

namespace {

const int E_INVALID = ATACOM_OFFSTEP_E_INVALID;

std::string dec(long long v) { return std::to_string(v); }

// [lo, hi) in bytes; `written`: everything but a gradient
struct Extent {
    intptr_t lo, hi;
    bool written;
    std::string name;
};

bool overlap(const Extent& a, const Extent& b) { return a.lo < b.hi && b.lo < a.hi; }

int check_shape(int32_t dtype, int32_t n_in, int32_t n_out, int32_t n_act, const std::string& w) {
    if (dtype != ATACOM_OFFSTEP_F32 && dtype != ATACOM_OFFSTEP_F64) return fail(E_INVALID, w + ": no kernel for dtype " + dec(dtype));
    if (n_in < 1 || n_in > ATACOM_OFFSTEP_MAX_IN)
        return fail(E_INVALID, w + ": n_in = " + dec(n_in) + " is outside 1 .. " + dec(ATACOM_OFFSTEP_MAX_IN));
    if (n_out < 1 || n_out > ATACOM_OFFSTEP_MAX_OUT)
        return fail(E_INVALID, w + ": n_out = " + dec(n_out) + " is outside 1 .. " + dec(ATACOM_OFFSTEP_MAX_OUT));
    if (n_act < 0 || n_act > ATACOM_OFFSTEP_MAX_ACT)
        return fail(E_INVALID, w + ": n_act = " + dec(n_act) + " is outside 0 .. " + dec(ATACOM_OFFSTEP_MAX_ACT));
    return ATACOM_OFFSTEP_OK;
}

// Everything a step asks of its arguments; init takes the same struct and asks the same.
int check(const atacom_offstep_args* a, const std::string& w) {
    if (!a) return fail(E_INVALID, w + ": null argument");
    if (a->struct_size != sizeof(atacom_offstep_args))
        return fail(E_INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " + dec(sizeof(atacom_offstep_args)));
    if (a->device < 0) return fail(E_INVALID, w + ": device = " + dec(a->device));
    if (a->n_groups < 1 || a->n_groups > ATACOM_OFFSTEP_MAX_GROUPS)
        return fail(E_INVALID, w + ": n_groups = " + dec(a->n_groups) + " is outside 1 .. " + dec(ATACOM_OFFSTEP_MAX_GROUPS));
    if (a->dtype != ATACOM_OFFSTEP_F32 && a->dtype != ATACOM_OFFSTEP_F64) return fail(E_INVALID, w + ": no kernel for dtype " + dec(a->dtype));
    const struct { const char* name; double v; } betas[2] = {{"beta1", a->beta1}, {"beta2", a->beta2}};
    for (const auto& b : betas)
        if (!(b.v >= 0.0 && b.v < 1.0)) return fail(E_INVALID, w + ": " + b.name + " must be in [0, 1), got " + std::to_string(b.v));
    if (!(a->eps > 0.0) || !std::isfinite(a->eps)) return fail(E_INVALID, w + ": eps must be > 0 and finite, got " + std::to_string(a->eps));
    if (!(a->tau >= 0.0 && a->tau <= 1.0)) return fail(E_INVALID, w + ": tau must be in [0, 1], got " + std::to_string(a->tau));
    const int esize = a->dtype == ATACOM_OFFSTEP_F64 ? 8 : 4;
    static const char* const kNames[atacom_offstep::kSegments] = {"W1", "b1", "W2", "b2", "W3", "b3", "W2a"};
    std::vector<Extent> ext;
    for (int k = 0; k < a->n_groups; ++k) {
        const atacom_offstep_group& g = a->groups[k];
        const std::string gw = w + ": groups[" + dec(k) + "]", gn = "groups[" + dec(k) + "].";
        if (int rc = check_shape(a->dtype, g.n_in, g.n_out, g.n_act, gw)) return rc;
        int n[atacom_offstep::kSegments];
        const int64_t N = atacom_offstep::segments(g.n_in, g.n_out, g.n_act, n);
        const void* const p[atacom_offstep::kSegments] = {g.W1, g.b1, g.W2, g.b2, g.W3, g.b3, g.W2a};
        int set = 0, used = 0;
        for (int i = 0; i < atacom_offstep::kSegments; ++i) {
            if (n[i] == 0) continue;                         // W2a of a plain network: neither pointer is read
            if (!p[i]) return fail(E_INVALID, gw + ": null argument (a weight or bias of the network)");
            ++used;
            set += g.target[i] != nullptr;
        }
        if (set != 0 && set != used)
            return fail(E_INVALID, gw + ": target is partly set: " + dec(set) + " of its " + dec(used) + " tensors (all or none)");
        if (!g.state) return fail(E_INVALID, gw + ": null argument (state)");
        if (!(g.lr >= 0.0) || !std::isfinite(g.lr)) return fail(E_INVALID, gw + ": lr must be >= 0 and finite, got " + std::to_string(g.lr));
        if (!std::isfinite(g.grad_scale)) return fail(E_INVALID, gw + ": grad_scale must be finite, got " + std::to_string(g.grad_scale));
        if ((intptr_t)g.state % 8) return fail(E_INVALID, gw + ": state must be aligned to 8 bytes");
        for (int i = 0; i < atacom_offstep::kSegments; ++i) {
            if (n[i] == 0) continue;
            const intptr_t bytes = (intptr_t)n[i] * esize;
            if ((intptr_t)p[i] % esize) return fail(E_INVALID, gw + ": " + kNames[i] + " must be aligned to the dtype");
            ext.push_back({(intptr_t)p[i], (intptr_t)p[i] + bytes, true, gn + kNames[i]});
            if (!set) continue;
            const intptr_t t = (intptr_t)g.target[i];
            if (t % esize) return fail(E_INVALID, gw + ": target " + kNames[i] + " must be aligned to the dtype");
            ext.push_back({t, t + bytes, true, gn + "target." + kNames[i]});
        }
        if (g.grad) {
            if ((intptr_t)g.grad % esize) return fail(E_INVALID, gw + ": grad must be aligned to the dtype");
            ext.push_back({(intptr_t)g.grad, (intptr_t)g.grad + (intptr_t)(N * esize), false, gn + "grad"});
        }
        ext.push_back({(intptr_t)g.state, (intptr_t)g.state + (intptr_t)atacom_offstep::state_bytes(g.n_in, g.n_out, g.n_act, esize == 8),
                       true, gn + "state"});
    }
    for (size_t i = 0; i < ext.size(); ++i)
        for (size_t j = 0; j < i; ++j)
            if ((ext[i].written || ext[j].written) && overlap(ext[i], ext[j]))
                return fail(E_INVALID, w + ": " + ext[j].name + " overlaps " + ext[i].name);
    return ATACOM_OFFSTEP_OK;
}

}  // namespace

extern "C" {

const char* atacom_offstep_last_error(void) { return g_err.c_str(); }
const char* atacom_offstep_version(void) { return "atacom_offstep 1.0 (gfx950)"; }

size_t atacom_offstep_state_size(int32_t dtype, int32_t n_in, int32_t n_out, int32_t n_act) {
    if (check_shape(dtype, n_in, n_out, n_act, "atacom_offstep_state_size")) return 0;
    return (size_t)atacom_offstep::state_bytes(n_in, n_out, n_act, dtype == ATACOM_OFFSTEP_F64);
}

int atacom_offstep_adam_init(const atacom_offstep_args* a) {
    if (int rc = check(a, "atacom_offstep_adam_init")) return rc;
    ON_DEVICE(a);
    atacom_offstep::init_launch(*a, (hipStream_t)a->stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OFFSTEP_OK;
}

int atacom_offstep_adam_step(const atacom_offstep_args* a) {
    if (int rc = check(a, "atacom_offstep_adam_step")) return rc;
    ON_DEVICE(a);
    atacom_offstep::step_launch(*a, (hipStream_t)a->stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OFFSTEP_OK;
}

}  // extern "C"
