// C-ABI host side of libatacom_evaluate.so (see include/atacom_evaluate_hip.h).  No handle: the device index travels in the
// call's argument struct.  Validates, then dispatches to the launcher; contains no numerics.
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

#include "atacom_evaluate.h"
#define ATACOM_CAPI_E_HIP ATACOM_EVALUATE_E_HIP
#include "atacom_capi_common.h"      // g_err, fail, HIP_TRY, DeviceGuard, ON_DEVICE
#include "atacom_mlp_host.h"         // mlp_abi_copy

namespace {

std::string dec(long long v) { return std::to_string(v); }

// [lo, hi) in bytes of the memory a view of rows of `width` elements touches
struct Extent {
    intptr_t lo, hi;
};

Extent extent(const atacom_evaluate_view& v, int64_t n_outer, int64_t n_inner, int width, int esize) {
    int64_t lo = 0, hi = width - 1;
    const int64_t so = n_outer > 1 ? v.stride_outer * (n_outer - 1) : 0, si = n_inner > 1 ? v.stride_inner * (n_inner - 1) : 0;
    (so < 0 ? lo : hi) += so;
    (si < 0 ? lo : hi) += si;
    const intptr_t base = (intptr_t)v.ptr;
    return {base + (intptr_t)(lo * esize), base + (intptr_t)((hi + 1) * esize)};
}

bool overlap(const Extent& a, const Extent& b) { return a.lo < b.hi && b.lo < a.hi; }

// rows must not run into each other: an input may repeat a row (stride 0), an output may not
int check_strides(const atacom_evaluate_view& v, int64_t n_outer, int64_t n_inner, int width, bool output, const char* name,
                  const std::string& w) {
    const struct { int64_t n, st; const char* dim; } dims[2] = {{n_outer, v.stride_outer, "stride_outer"}, {n_inner, v.stride_inner, "stride_inner"}};
    for (const auto& d : dims) {
        if (d.n <= 1) continue;
        const int64_t mag = d.st < 0 ? -d.st : d.st;
        if (mag >= width || (!output && d.st == 0)) continue;
        return fail(ATACOM_EVALUATE_E_INVALID, w + ": " + name + "." + d.dim + " = " + dec(d.st) + " is below the row width " + dec(width));
    }
    return ATACOM_EVALUATE_OK;
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

}  // namespace

extern "C" {

const char* atacom_evaluate_last_error(void) { return g_err.c_str(); }
const char* atacom_evaluate_version(void) { return "atacom_evaluate 1.0 (gfx950)"; }

int atacom_evaluate_mlp(const atacom_evaluate_args* a) {
    const std::string w = "atacom_evaluate_mlp";
    if (!a) return fail(ATACOM_EVALUATE_E_INVALID, w + ": null argument");
    if (a->struct_size != sizeof(atacom_evaluate_args))
        return fail(ATACOM_EVALUATE_E_INVALID, w + ": struct_size = " + dec(a->struct_size) + ", this library expects " +
                                                   dec(sizeof(atacom_evaluate_args)));
    if (a->device < 0) return fail(ATACOM_EVALUATE_E_INVALID, w + ": device = " + dec(a->device));
    if (a->dtype != ATACOM_EVALUATE_F32 && a->dtype != ATACOM_EVALUATE_F64)
        return fail(ATACOM_EVALUATE_E_UNSUPPORTED, w + ": no kernel for dtype " + dec(a->dtype));
    if (a->n_outer < 1) return fail(ATACOM_EVALUATE_E_INVALID, w + ": n_outer must be >= 1, got " + dec(a->n_outer));
    if (a->n_inner < 1) return fail(ATACOM_EVALUATE_E_INVALID, w + ": n_inner must be >= 1, got " + dec(a->n_inner));
    if (a->n_outer > ATACOM_EVALUATE_MAX_ROWS / a->n_inner)
        return fail(ATACOM_EVALUATE_E_UNSUPPORTED, w + ": n_outer * n_inner = " + dec(a->n_outer) + " * " + dec(a->n_inner) +
                                                       " rows is too many (at most " + dec(ATACOM_EVALUATE_MAX_ROWS) + " a call)");
    if (a->n_blocks < 0) return fail(ATACOM_EVALUATE_E_INVALID, w + ": n_blocks must be >= 1, or 0 for the library's choice, got " + dec(a->n_blocks));
    if (a->n_blocks > ATACOM_EVALUATE_MAX_BLOCKS)
        return fail(ATACOM_EVALUATE_E_UNSUPPORTED, w + ": n_blocks = " + dec(a->n_blocks) + " exceeds the launch grid (" +
                                                       dec(ATACOM_EVALUATE_MAX_BLOCKS) + ")");
    // ---- the network
    atacom_mlp net;
    if (!atacom::mlp_abi_copy(&a->net, &net))
        return fail(ATACOM_EVALUATE_E_INVALID, w + ": net.struct_size = " + dec(a->net.struct_size) + ", this library expects " +
                                                   dec(sizeof(atacom_mlp)) + " or " + dec(ATACOM_MLP_SIZE_V1));
    if (net.hidden != ATACOM_EVALUATE_HIDDEN)
        return fail(ATACOM_EVALUATE_E_UNSUPPORTED, w + ": hidden = " + dec(net.hidden) + ", only 64 hidden units are supported");
    if (net.n_in < 1 || net.n_in > ATACOM_EVALUATE_MAX_IN)
        return fail(ATACOM_EVALUATE_E_UNSUPPORTED, w + ": n_in = " + dec(net.n_in) + " is outside 1 .. " + dec(ATACOM_EVALUATE_MAX_IN));
    if (net.n_out < 1 || net.n_out > ATACOM_EVALUATE_MAX_OUT)
        return fail(ATACOM_EVALUATE_E_UNSUPPORTED, w + ": n_out = " + dec(net.n_out) + " is outside 1 .. " + dec(ATACOM_EVALUATE_MAX_OUT));
    if (net.activation != 0 && net.activation != 1)
        return fail(ATACOM_EVALUATE_E_UNSUPPORTED, w + ": activation = " + dec(net.activation) + " (0 = ReLU, 1 = tanh)");
    if (!net.W1 || !net.b1 || !net.W2 || !net.b2 || !net.W3 || !net.b3)
        return fail(ATACOM_EVALUATE_E_INVALID, w + ": null argument (a weight or bias of the network)");
    if (net.sW1 || net.sb1 || net.sW2 || net.sb2 || net.sW3 || net.sb3)
        return fail(ATACOM_EVALUATE_E_UNSUPPORTED, w + ": a sigma network is not supported (the log-probability is that of a state-independent std)");
    if (net.squash) return fail(ATACOM_EVALUATE_E_UNSUPPORTED, w + ": squash is not supported (SAC's squashed log-probability is out of scope)");
    if (net.mean_mode) return fail(ATACOM_EVALUATE_E_UNSUPPORTED, w + ": mean_mode = " + dec(net.mean_mode) + " is not supported");
    if (net.explore) return fail(ATACOM_EVALUATE_E_UNSUPPORTED, w + ": explore = " + dec(net.explore) + " is not supported");
    // ---- the views
    if (!a->x.ptr) return fail(ATACOM_EVALUATE_E_INVALID, w + ": null argument (x)");
    if (!a->y.ptr && !a->logp.ptr) return fail(ATACOM_EVALUATE_E_INVALID, w + ": neither y nor logp is requested");
    if (a->logp.ptr && (!a->action.ptr || !net.std))
        return fail(ATACOM_EVALUATE_E_INVALID, w + ": logp needs action and net.std");
    const int64_t no = a->n_outer, ni = a->n_inner;
    const int esize = a->dtype == ATACOM_EVALUATE_F64 ? 8 : 4;
    if (int rc = check_strides(a->x, no, ni, net.n_in, false, "x", w)) return rc;
    if (a->logp.ptr)
        if (int rc = check_strides(a->action, no, ni, net.n_out, false, "action", w)) return rc;
    if (a->y.ptr)
        if (int rc = check_strides(a->y, no, ni, net.n_out, true, "y", w)) return rc;
    if (a->logp.ptr)
        if (int rc = check_strides(a->logp, no, ni, 1, true, "logp", w)) return rc;
    const Extent ex = extent(a->x, no, ni, net.n_in, esize), ea = extent(a->action, no, ni, net.n_out, esize),
                 ey = extent(a->y, no, ni, net.n_out, esize), el = extent(a->logp, no, ni, 1, esize);
    if (a->y.ptr && overlap(ey, ex)) return fail(ATACOM_EVALUATE_E_INVALID, w + ": y overlaps x");
    if (a->y.ptr && a->logp.ptr && overlap(ey, ea)) return fail(ATACOM_EVALUATE_E_INVALID, w + ": y overlaps action");
    if (a->logp.ptr && overlap(el, ex)) return fail(ATACOM_EVALUATE_E_INVALID, w + ": logp overlaps x");
    if (a->logp.ptr && overlap(el, ea)) return fail(ATACOM_EVALUATE_E_INVALID, w + ": logp overlaps action");
    if (a->y.ptr && a->logp.ptr && overlap(ey, el)) return fail(ATACOM_EVALUATE_E_INVALID, w + ": y overlaps logp");

    ON_DEVICE(a);
    const bool f64 = a->dtype == ATACOM_EVALUATE_F64;
    int64_t blocks = a->n_blocks;
    if (blocks == 0) {
        const int64_t need = atacom_evaluate::tiles(no * ni, f64);
        const int64_t fit = (int64_t)compute_units(a->device) * atacom_evaluate::kResident;
        blocks = need < fit ? need : fit;
        if (blocks > ATACOM_EVALUATE_MAX_BLOCKS) blocks = ATACOM_EVALUATE_MAX_BLOCKS;
    }
    if (atacom_evaluate::evaluate_launch(*a, net, (int)blocks, (hipStream_t)a->stream))
        return fail(ATACOM_EVALUATE_E_UNSUPPORTED, w + ": no kernel for this call");
    HIP_TRY(hipGetLastError());
    return ATACOM_EVALUATE_OK;
}

}  // extern "C"
