// Host checks of the strided views (atacom_evaluate_view) of a call, shared by the C-ABI files of the libraries that walk the
// rows of a collection (../fit/atacom_fit_capi.cpp, ../trust/atacom_trust_capi.cpp, ../offpolicy/atacom_offpolicy_capi.cpp,
// ../offgrad/atacom_offgrad_capi.cpp, ../soft/atacom_soft_capi.cpp): the bytes a view or a flat buffer spans, whether two spans
// overlap, and that the rows of a view do not run into each other; for the off-policy libraries also spans that carry the name
// a refusal calls them by, the checks of a row stride, an alignment, a workspace and a list of outputs against the inputs, and
// the head every row call shares.  Internal linkage, like ../atacom_capi_common.h, whose fail() carries the message.  The
// including file defines ATACOM_CAPI_E_INVALID -- its library's code for "an invalid argument" -- before the include; success
// is 0 in every library.  check_head needs more of the library's constants: a file that wants it also defines
// ATACOM_CAPI_LIB(X), its name for the constant X (E_UNSUPPORTED, F32, F64, MAX_ROWS, MAX_BLOCKS).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../../include/atacom_evaluate_hip.h"   // atacom_evaluate_view
#include "../atacom_capi_common.h"                  // fail

#ifndef ATACOM_CAPI_E_INVALID
#error "define ATACOM_CAPI_E_INVALID (the library's invalid-argument code) before including atacom_view_checks.h"
#endif

namespace {

std::string dec(long long v) { return std::to_string(v); }

// [lo, hi) in bytes
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

Extent flat(const void* p, int64_t bytes) { return {(intptr_t)p, (intptr_t)p + (intptr_t)bytes}; }

bool overlap(const Extent& a, const Extent& b) { return a.lo < b.hi && b.lo < a.hi; }

// rows must not run into each other; every view here is an input and may repeat a row (stride 0)
int check_strides(const atacom_evaluate_view& v, int64_t n_outer, int64_t n_inner, int width, const char* name, const std::string& w) {
    const struct { int64_t n, st; const char* dim; } dims[2] = {{n_outer, v.stride_outer, "stride_outer"}, {n_inner, v.stride_inner, "stride_inner"}};
    for (const auto& d : dims) {
        if (d.n <= 1) continue;
        const int64_t mag = d.st < 0 ? -d.st : d.st;
        if (mag >= width || d.st == 0) continue;
        return fail(ATACOM_CAPI_E_INVALID, w + ": " + name + "." + d.dim + " = " + dec(d.st) + " is below the row width " + dec(width));
    }
    return 0;
}

// ---- with names: what the off-policy libraries' refusals quote
struct Named : Extent {
    std::string name;
};

Named extent(const atacom_evaluate_view& v, int64_t n_outer, int64_t n_inner, int width, int esize, const char* name) {
    return {extent(v, n_outer, n_inner, width, esize), name};
}

// M rows of `width` at ptr[r * stride]
Named strided(const void* p, int64_t rows, int64_t stride, int width, int esize, const char* name) {
    int64_t lo = 0, hi = width - 1;
    const int64_t s = rows > 1 ? stride * (rows - 1) : 0;
    (s < 0 ? lo : hi) += s;
    return {{(intptr_t)p + (intptr_t)(lo * esize), (intptr_t)p + (intptr_t)((hi + 1) * esize)}, name};
}

Named flat(const void* p, int64_t bytes, const std::string& name) { return {flat(p, bytes), name}; }

int check_row_stride(int64_t rows, int64_t stride, int width, bool output, const char* name, const std::string& w) {
    if (rows <= 1) return 0;
    const int64_t mag = stride < 0 ? -stride : stride;
    if (mag >= width || (!output && stride == 0)) return 0;
    return fail(ATACOM_CAPI_E_INVALID, w + ": " + name + "_stride = " + dec(stride) + " is below the row width " + dec(width));
}

int check_aligned(const void* p, int esize, const std::string& name, const std::string& w) {
    if ((intptr_t)p % esize == 0) return 0;
    return fail(ATACOM_CAPI_E_INVALID, w + ": " + name + " must be aligned to the dtype");
}

// an output against every input and the outputs before it
int check_overlaps(const std::vector<Named>& outs, const std::vector<Named>& ins, const std::string& w) {
    for (size_t o = 0; o < outs.size(); ++o) {
        for (const auto& in : ins)
            if (overlap(outs[o], in)) return fail(ATACOM_CAPI_E_INVALID, w + ": " + outs[o].name + " overlaps " + in.name);
        for (size_t p = 0; p < o; ++p)
            if (overlap(outs[o], outs[p])) return fail(ATACOM_CAPI_E_INVALID, w + ": " + outs[p].name + " overlaps " + outs[o].name);
    }
    return 0;
}

// `sizer`: the library's function that gives `need`
int check_workspace(const void* ws, size_t have, size_t need, const char* sizer, const std::string& w) {
    if (!ws) return fail(ATACOM_CAPI_E_INVALID, w + ": null argument (workspace)");
    if ((intptr_t)ws % 16) return fail(ATACOM_CAPI_E_INVALID, w + ": workspace must be aligned to 16 bytes");
    if (have < need)
        return fail(ATACOM_CAPI_E_INVALID, w + ": workspace_bytes = " + dec((long long)have) + " is below the " + dec((long long)need) +
                                               " that " + sizer + " gives");
    return 0;
}

#ifdef ATACOM_CAPI_LIB
// what every row call shares: sizes, idx.  *rows = M.
int check_head(int32_t device, int32_t dtype, int32_t n_blocks, int64_t n_outer, int64_t n_inner, const int64_t* idx, int64_t n_idx,
               const std::string& w, int64_t* rows) {
    constexpr int INVALID = ATACOM_CAPI_E_INVALID, UNSUPPORTED = ATACOM_CAPI_LIB(E_UNSUPPORTED);
    constexpr int64_t MAX_ROWS = ATACOM_CAPI_LIB(MAX_ROWS), MAX_BLOCKS = ATACOM_CAPI_LIB(MAX_BLOCKS);
    if (device < 0) return fail(INVALID, w + ": device = " + dec(device));
    if (dtype != ATACOM_CAPI_LIB(F32) && dtype != ATACOM_CAPI_LIB(F64)) return fail(UNSUPPORTED, w + ": no kernel for dtype " + dec(dtype));
    if (n_outer < 1) return fail(INVALID, w + ": n_outer must be >= 1, got " + dec(n_outer));
    if (n_inner < 1) return fail(INVALID, w + ": n_inner must be >= 1, got " + dec(n_inner));
    if (n_outer > MAX_ROWS / n_inner)
        return fail(UNSUPPORTED, w + ": n_outer * n_inner = " + dec(n_outer) + " * " + dec(n_inner) + " rows is too many (at most " +
                                     dec(MAX_ROWS) + " a call)");
    if (n_blocks < 0) return fail(INVALID, w + ": n_blocks must be >= 1, or 0 for the library's choice, got " + dec(n_blocks));
    if (n_blocks > MAX_BLOCKS) return fail(UNSUPPORTED, w + ": n_blocks = " + dec(n_blocks) + " exceeds the launch grid (" + dec(MAX_BLOCKS) + ")");
    if (idx && n_idx < 1) return fail(INVALID, w + ": n_idx must be >= 1 with idx, got " + dec(n_idx));
    if (idx && n_idx > MAX_ROWS) return fail(UNSUPPORTED, w + ": n_idx = " + dec(n_idx) + " rows is too many (at most " + dec(MAX_ROWS) + " a call)");
    *rows = idx ? n_idx : n_outer * n_inner;
    return 0;
}
#endif

}  // namespace
