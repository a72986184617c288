// The forward half in front of atacom_mlp_backward.h, once: what the kernels of ../offgrad/atacom_offgrad.hip and
// ../soft/atacom_soft.hip share of a run-time-width 2 x 64 network before its dy exists -- the staging of its weights into one
// MlpLdsM<4 CH, 64, 8> block, the normalised observation and the float64 layers -- and the row views of their launchers.
// Same namespace, same rule as the backward header (every expression means the same with and without contraction), same WA
// flag: layer 2 of a DDPG / TD3 critic has the branch W2a as, and W2a [64][8] lives in rows 8 .. 15 of the block's W3 rows,
// whose outputs are never stored.
// A unit keeps its Net (any struct with W1, b1, W2, b2, W3, b3, shift, scale, n1, n_out, activation; W2a with WA), its AUX
// words, its first-layer input beyond the observation (x1_elem, as_elem), its head, and forward_block, the float32 forward
// pass of a block of 16 rows: in one function with either unit's layer 1 the other unit's kernels measured slower, and split
// into layer 1 and a shared rest neither unit's kernels stay the code they were (profiles/offpolicy_forward_shared.md).
// ../offpolicy/atacom_offpolicy.hip shares none of this: its forward runs four blocks at once in another rounding order, and
// its library does not include the backward header.
#pragma once
#include "atacom_mlp_backward.h"

namespace atacom_mlp_backward {

// ------------------------------------------------------------------------------------------------------------ launchers
struct RowView {
    const void* ptr;
    int64_t so, si;
};

template <typename T>
Rows<T> rows_of(const RowView& v) {
    return Rows<T>{(const T*)v.ptr, v.so, v.si};
}

// dst.f = second ? b.f : a.f for every member f named: a network of the kernel's argument block is selected field by field,
// not indexed -- a run-time index into the argument block would put it in scratch
template <typename N, typename... M>
__device__ __forceinline__ void pick_fields(N& dst, bool second, const N& a, const N& b, M N::*... f) {
    ((dst.*f = second ? b.*f : a.*f), ...);
}

// ------------------------------------------------------------------------------------------------------------ float32
template <int CH>
struct LdsM : atacom::MlpLdsM<4 * CH, H, NK> {
    using L = atacom::MlpLdsM<4 * CH, H, NK>;
    static constexpr int W2A = L::W3 + 8 * L::S2;      // [64][8], with WA
    static constexpr int AUX = L::EXPLORE;             // the unit's own words (act_scale, ...): 40 floats
    static_assert(H * 8 <= 8 * L::S2, "W2a fits the unread half of the W3 block");
};

// Every word of the block that a phase reads, but AUX, the padding as zero: the W1 slots at or past n1, the W3 rows and biases
// from n_out to 7 and, with WA, the W2a columns at or past n_act (all of them when W2a is null); without WA the W3 rows up to
// 15.  The observation's normalisation covers the first n_obs elements of the first layer's input.  No barrier: the caller
// has one before (the phase before has read its weights), writes its AUX words and has one after.
// The kernels stage inside their loop over the rounds.  Left visible, the per-thread source addresses of every staging
// iteration (they divide by n1) are hoisted out of that loop as 64-bit pairs and spill to scratch; an opaque thread index
// keeps them where they are used -- `tid` is the caller's, opaque for its AUX loop too.
template <int CH, bool WA, typename N>
__device__ __forceinline__ void stage_weights(const N& n, int n_obs, int n_act, float* lds, int& tid) {
    using L = LdsM<CH>;
    asm volatile("" : "+v"(tid));
    for (int i = tid; i < H * L::S1; i += kBlock) {      // [unit][g][8], slot s of group g = element CH g + s
        const int u = i / L::S1, g = (i % L::S1) / 8, s = i % 8, e = CH * g + s;
        lds[L::W1 + i] = (s < CH && e < n.n1) ? n.W1[u * n.n1 + e] : 0.0f;
    }
    for (int i = tid; i < H * H; i += kBlock) lds[L::W2 + (i / H) * L::S2 + (i % H)] = n.W2[i];
    for (int i = tid; i < (WA ? 8 : 16) * H; i += kBlock) lds[L::W3 + (i / H) * L::S2 + (i % H)] = i < n.n_out * H ? n.W3[i] : 0.0f;
    if constexpr (WA)
        for (int i = tid; i < 8 * L::S2; i += kBlock) {  // rows 8 .. 15 of the W3 block: W2a [64][8], then zeros
            const int u = i / 8, k = i % 8;
            lds[L::W2A + i] = (n.W2a && u < H && k < n_act) ? n.W2a[u * n_act + k] : 0.0f;
        }
    for (int i = tid; i < H; i += kBlock) { lds[L::B1 + i] = n.b1[i]; lds[L::B2 + i] = n.b2[i]; }
    for (int i = tid; i < 16; i += kBlock) lds[L::B3 + i] = i < n.n_out ? n.b3[i] : 0.0f;
    for (int i = tid; i < 32; i += kBlock) {             // [g][8] like W1; past the observation: shift 0, scale 1
        const int g = i / 8, s = i % 8, e = CH * g + s;
        const bool real = s < CH && e < n_obs;
        lds[L::SHIFT + i] = (real && n.shift) ? n.shift[e] : 0.0f;
        lds[L::SCALE + i] = (real && n.scale) ? n.scale[e] : 1.0f;
    }
}

// element e of the normalised observation of the row at xr; 0 at or past n_obs.  The load is under the full exec mask.
template <int CH>
__device__ __forceinline__ float obs_elem(const float* lds, const float* xr, int e, int n_obs) {
    using L = LdsM<CH>;
    const int ec = e < n_obs ? e : n_obs - 1;
    const int slot = 8 * (ec / CH) + ec % CH;
    const float v = (xr[ec] - lds[L::SHIFT + slot]) * lds[L::SCALE + slot];
    return e < n_obs ? v : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------ float64
// the normalised observation of the row at xr, elements c, c + 16, ... of D
template <typename N>
__device__ __forceinline__ void normalise_f64(const N& n, const double* xr, double* dst, int D, int c) {
    for (int e = c; e < D; e += 16) dst[e] = (xr[e] - (n.shift ? n.shift[e] : 0.0)) * (n.scale ? n.scale[e] : 1.0);
}

// two hidden layers of a network from the columns cx (n1 values) of the thread's record into the columns ch1, ch2; with WA and
// a W2a that is not null, layer 2 adds W2a as, as the n_act values at the columns cas.  All threads of the workgroup call it:
// two barriers.
template <bool WA, typename N>
__device__ __forceinline__ void hidden_f64(const N& n, double* me, int cx, int ch1, int ch2, int n_act, int cas, bool live, int c) {
    if (live)
        for (int j = c; j < H; j += 16) {
            double a = n.b1[j];
            for (int e = 0; e < n.n1; ++e) a = __builtin_fma(n.W1[j * n.n1 + e], me[cx + e], a);
            me[ch1 + j] = atacom::mlp_act(a, n.activation);
        }
    __syncthreads();
    if (live)
        for (int j = c; j < H; j += 16) {
            double a = n.b2[j];
            for (int i = 0; i < H; ++i) a = __builtin_fma(n.W2[j * H + i], me[ch1 + i], a);
            if constexpr (WA)
                if (n.W2a)
                    for (int k = 0; k < n_act; ++k) a = __builtin_fma(n.W2a[j * n_act + k], me[cas + k], a);
            me[ch2 + j] = atacom::mlp_act(a, n.activation);
        }
    __syncthreads();
}

// ... of a network without the second branch
template <typename N>
__device__ __forceinline__ void hidden_f64(const N& n, double* me, int cx, int ch1, int ch2, bool live, int c) {
    hidden_f64<false>(n, me, cx, ch1, ch2, 0, 0, live, c);
}

// output o of a network from the columns ch2
template <typename N>
__device__ __forceinline__ double head_f64(const N& n, const double* me, int ch2, int o) {
    double a = n.b3[o];
    for (int j = 0; j < H; ++j) a = __builtin_fma(n.W3[o * H + j], me[ch2 + j], a);
    return a;
}

}  // namespace atacom_mlp_backward
