// C-ABI host side of libatacom_returns.so (see include/atacom_returns_hip.h).  No handle: the device index travels in the
// call's argument struct.  Validates, then dispatches to the launchers; contains no numerics.
#include <hip/hip_runtime.h>

#include <string>

#include "atacom_returns.h"
#define ATACOM_CAPI_E_HIP ATACOM_RETURNS_E_HIP
#include "atacom_capi_common.h"      // g_err, fail, HIP_TRY, DeviceGuard, ON_DEVICE

namespace {

std::string dec(long long v) { return std::to_string(v); }

int check_shape(const atacom_returns_shape& sh, const std::string& w, bool flags) {
    if (sh.device < 0) return fail(ATACOM_RETURNS_E_INVALID, w + ": device = " + dec(sh.device));
    if (sh.n_steps < 1) return fail(ATACOM_RETURNS_E_INVALID, w + ": n_steps must be >= 1, got " + dec(sh.n_steps));
    if (sh.batch < 1) return fail(ATACOM_RETURNS_E_INVALID, w + ": batch must be >= 1, got " + dec(sh.batch));
    if (sh.n_blocks < 1) return fail(ATACOM_RETURNS_E_INVALID, w + ": n_blocks must be >= 1, got " + dec(sh.n_blocks));
    if (sh.dtype != ATACOM_RETURNS_F32 && sh.dtype != ATACOM_RETURNS_F64)
        return fail(ATACOM_RETURNS_E_UNSUPPORTED, w + ": no kernel for dtype " + dec(sh.dtype));
    if (flags && sh.flag_dtype != ATACOM_RETURNS_FLAG_U8 && sh.flag_dtype != ATACOM_RETURNS_FLAG_VALUE)
        return fail(ATACOM_RETURNS_E_UNSUPPORTED, w + ": no kernel for flag_dtype " + dec(sh.flag_dtype));
    if (sh.n_blocks > atacom_returns::kMaxGridYZ)
        return fail(ATACOM_RETURNS_E_UNSUPPORTED, w + ": n_blocks = " + dec(sh.n_blocks) + " exceeds the launch grid (" +
                                                      dec(atacom_returns::kMaxGridYZ) + ")");
    return ATACOM_RETURNS_OK;
}

// the normalisation spreads the steps over a grid axis
int check_normalize_shape(const atacom_returns_shape& sh, const std::string& w) {
    if (sh.n_steps > atacom_returns::kMaxGridYZ)
        return fail(ATACOM_RETURNS_E_UNSUPPORTED, w + ": n_steps = " + dec(sh.n_steps) + " exceeds the launch grid of the normalisation (" +
                                                      dec(atacom_returns::kMaxGridYZ) + ")");
    return ATACOM_RETURNS_OK;
}

int check_unit(double x, const char* name, const std::string& w) {
    if (!(x >= 0.0 && x <= 1.0)) return fail(ATACOM_RETURNS_E_INVALID, w + ": " + name + " must be in [0, 1], got " + std::to_string(x));
    return ATACOM_RETURNS_OK;
}

template <typename A>
int check_size(const A* a, const std::string& w) {
    if (!a) return fail(ATACOM_RETURNS_E_INVALID, w + ": null argument");
    if (a->struct_size != sizeof(A))
        return fail(ATACOM_RETURNS_E_INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " + dec(sizeof(A)));
    return ATACOM_RETURNS_OK;
}

}  // namespace

extern "C" {

const char* atacom_returns_last_error(void) { return g_err.c_str(); }
const char* atacom_returns_version(void) { return "atacom_returns 1.0 (gfx950)"; }

int atacom_returns_gae(const atacom_returns_gae_args* a) {
    const std::string w = "atacom_returns_gae";
    if (int rc = check_size(a, w)) return rc;
    if (!a->reward.ptr || !a->absorbing.ptr || !a->last.ptr || !a->ret.ptr || !a->adv.ptr)
        return fail(ATACOM_RETURNS_E_INVALID, w + ": null argument");
    if ((a->v.ptr == nullptr) != (a->v_next.ptr == nullptr))
        return fail(ATACOM_RETURNS_E_INVALID, w + ": v and v_next must both be given or both be null");
    if (a->normalize && (!a->d_workspace || !a->d_stats))
        return fail(ATACOM_RETURNS_E_INVALID, w + ": null argument (normalize needs d_workspace and d_stats)");
    if (int rc = check_shape(a->shape, w, true)) return rc;
    if (int rc = check_unit(a->gamma, "gamma", w)) return rc;
    if (int rc = check_unit(a->lam, "lam", w)) return rc;
    if (a->normalize)
        if (int rc = check_normalize_shape(a->shape, w)) return rc;
    ON_DEVICE(&a->shape);
    atacom_returns::gae_launch(*a, (hipStream_t)a->stream);
    HIP_TRY(hipGetLastError());
    if (a->normalize) {
        atacom_returns::normalize_launch(a->shape, a->adv, a->d_workspace, a->d_stats, (hipStream_t)a->stream);
        HIP_TRY(hipGetLastError());
    }
    return ATACOM_RETURNS_OK;
}

int atacom_returns_normalize(const atacom_returns_normalize_args* a) {
    const std::string w = "atacom_returns_normalize";
    if (int rc = check_size(a, w)) return rc;
    if (!a->adv.ptr || !a->d_workspace || !a->d_stats) return fail(ATACOM_RETURNS_E_INVALID, w + ": null argument");
    if (int rc = check_shape(a->shape, w, false)) return rc;
    if (int rc = check_normalize_shape(a->shape, w)) return rc;
    ON_DEVICE(&a->shape);
    atacom_returns::normalize_launch(a->shape, a->adv, a->d_workspace, a->d_stats, (hipStream_t)a->stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_RETURNS_OK;
}

int atacom_returns_episodes(const atacom_returns_episodes_args* a) {
    const std::string w = "atacom_returns_episodes";
    if (int rc = check_size(a, w)) return rc;
    if (!a->reward.ptr || !a->last.ptr || !a->d_workspace || !a->d_result) return fail(ATACOM_RETURNS_E_INVALID, w + ": null argument");
    if (int rc = check_shape(a->shape, w, true)) return rc;
    if (int rc = check_unit(a->gamma, "gamma", w)) return rc;
    ON_DEVICE(&a->shape);
    atacom_returns::episodes_launch(*a, (hipStream_t)a->stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_RETURNS_OK;
}

}  // extern "C"
