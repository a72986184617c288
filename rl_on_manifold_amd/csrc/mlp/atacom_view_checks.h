// Host checks of the strided views (atacom_evaluate_view) of a call, shared by the C-ABI files of the libraries that walk the
// rows of a collection (../fit/atacom_fit_capi.cpp, ../trust/atacom_trust_capi.cpp): the bytes a view or a flat buffer spans,
// whether two spans overlap, and that the rows of a view do not run into each other.  Internal linkage, like
// ../atacom_capi_common.h, whose fail() carries the message.  The including file defines ATACOM_CAPI_E_INVALID -- its library's
// code for "an invalid argument" -- before the include; success is 0 in every library.
#pragma once
#include <stdint.h>

#include <string>

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

}  // namespace
