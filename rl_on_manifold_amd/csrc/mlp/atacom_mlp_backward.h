// The backward pass of the 2 x 64 network of ../atacom_policy.h over the rows of a collection, once: what the kernels of
// ../fit/atacom_fit.hip (k_fit_gradient), ../trust/atacom_trust.hip (k_trust_fvp), ../offgrad/atacom_offgrad.hip
// (k_offgrad_critic, k_offgrad_actor) and ../soft/atacom_soft.hip (k_soft_critic, k_soft_actor) share, and the constants and
// sizes their launchers share.  Headers only: csrc/mlp/ is no library, and a unit that includes this file is rebuilt when it
// changes.  A unit keeps its Params, its staging where that differs, its forward (and tangent) layers 2 and 3, its head -- what
// dy is -- and its own tail of the hand-over, of the partial and of the reduction.
//
// THE RULE OF THIS FILE: every expression here means the same with and without floating-point contraction.  Two of the units
// compile with -ffp-contract=off and two with the compiler's default, and all four must get the same bits from the same grid,
// so a product followed by an addition is written as an explicit fma (__builtin_fma, __builtin_fmaf, the matrix-core builtin)
// or the two are kept apart by what lies between them (a subtraction BEFORE a product, a product alone, sums alone).
//
// WA: layer 2 of a DDPG / TD3 critic has a second branch, h2 = act(W2 h1 + W2a as + b2) with as the scaled action [n_act <= 8],
// so its gradient carries dW2a = sum_r delta2_r as_r^T.  Grads, backward, hand_over and store_net take the flag WA (default
// false: no such branch).  With it dW2a rides on dW2's A operands (one more accumulator, acc2a, handed over between acc2 and
// acc3) and is stored behind the network's values, at NetOffsets::end; net_columns takes n_act for its float64 column pairs.
//
// Float32, one wavefront, one block of 16 rows (lane = (n16, g) = (lane % 16, lane / 16)), on the LDS layout MlpLdsM, the operand
// mapping of mlp_forward_mfma and the wave-level fence of ../atacom_policy.h:
//   * transposed as there, H^T = W X^T, lane (n16, g) holds, in register v of tile t, unit 16 t + 4 g + v of row n16 -- for h1,
//     h2 and, computed the same way from W3^T and W2^T, for da2 and da1;
//   * the weight gradients dW = sum_r delta_r act_r^T have the ROW as the K index, so both operands are needed with
//     lane % 16 = unit, lane / 16 = row: the transposition of the above.  Each goes once through a [16 rows][64 units] buffer of
//     the wavefront's LDS staging area (put / get; the column is rotated by 16 (row % 4) so that the b128 writes and the b32 reads
//     are both free of bank conflicts without padding);
//   * the accumulators (Grads: 16 NT + 64 + 16 registers of dW1, dW2, dW3, NT = 1 or 2 tiles of inputs, 32 of db1, db2 and,
//     with WA, 16 of dW2a) stay in registers for the whole walk; at its end the bias sums are added across lanes (sum_biases),
//     wavefronts 1, 2, 3 hand their registers to wavefront 0 through LDS in that order (hand_over) and wavefront 0 stores the
//     partial (store_net).
// Float64: one record per row in LDS, sixteen threads a row; every thread owns the entries tid, tid + 256, ... of the partial,
// each the sum over rows of the product of two columns of the records (net_columns, accumulate_f64).  The record layout is the
// unit's own (C: columns H1, H2, D1, D2, X, DY, ONE).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../atacom_policy.h"

namespace atacom_mlp_backward {

// ------------------------------------------------------------------------------------------------------------ launchers
constexpr int kBlock = 256;                 // threads per workgroup: four wavefronts share one staged copy of the weights
constexpr int kWaves = kBlock / 64;
constexpr int kRowsF32 = 64;                // rows per wavefront and tile (four blocks of 16): the matrix-core form
constexpr int kRowsF64 = 16;                // rows per WORKGROUP and tile: the vector form
constexpr int kDefaultBlocks = 512;         // ceiling of a library's own choice of n_blocks (two workgroups per compute unit)
constexpr int kReduceBlock = 256;           // threads of a reduce workgroup: kReduceSlices slices of kReduceValues values
constexpr int kReduceValues = 32;
constexpr int kReduceSlices = kReduceBlock / kReduceValues;
constexpr int H = 64, NK = 8;               // hidden units; the most outputs
constexpr int kStage = 2048;                // floats of staging per wavefront: two [16][64] transposition buffers

// values of the network: W1, b1, W2, b2, W3, b3 in that order
__host__ __device__ inline int64_t net_size(int n_in, int n_out) { return 64 * (int64_t)n_in + 64 + 4096 + 64 + 64 * n_out + n_out; }

// where they begin in a partial
struct NetOffsets {
    int b1, W2, b2, W3, b3, end;
};

__device__ __forceinline__ NetOffsets net_offsets(int n_in, int n_out) {
    NetOffsets o;
    o.b1 = H * n_in; o.W2 = o.b1 + H; o.b2 = o.W2 + H * H; o.W3 = o.b2 + H; o.b3 = o.W3 + H * n_out; o.end = o.b3 + n_out;
    return o;
}

inline int64_t tiles(int64_t rows, bool f64) {
    const int per = f64 ? kRowsF64 : kWaves * kRowsF32;
    return (rows + per - 1) / per;
}

inline int64_t effective_blocks(int n_blocks, int64_t rows, bool f64) {
    if (n_blocks > 0) return n_blocks;
    const int64_t need = tiles(rows, f64);
    return need < kDefaultBlocks ? need : kDefaultBlocks;
}

// f(std::integral_constant<int, CH>) for CH = ceil(n_in / 4) = 1 .. 8; false when there is no such kernel
template <typename F>
bool with_ch(int n_in, F&& f) {
    switch ((n_in + 3) / 4) {
#define ATACOM_MLP_CH(CH) \
    case CH: f(std::integral_constant<int, CH>{}); return true
        ATACOM_MLP_CH(1); ATACOM_MLP_CH(2); ATACOM_MLP_CH(3); ATACOM_MLP_CH(4);
        ATACOM_MLP_CH(5); ATACOM_MLP_CH(6); ATACOM_MLP_CH(7); ATACOM_MLP_CH(8);
#undef ATACOM_MLP_CH
    }
    return false;
}

// ------------------------------------------------------------------------------------------------------------ the rows
template <typename T>
struct Rows {
    const T* p;
    int64_t so, si;
};

// the flat number of the call's row r (P: n_rows = M, idx); a row past the end is the last one again
template <typename P>
__device__ __forceinline__ int64_t flat_row(const P& p, int64_t r) {
    const int64_t last = p.n_rows - 1;
    r = r < last ? r : last;
    return p.idx ? p.idx[r] : r;
}

// the host admits at most 2^31 - 1 rows, so the row's (outer, inner) index is a 32-bit division; the offsets are 64-bit
template <typename T>
__device__ __forceinline__ const T* row_ptr(const Rows<T>& v, int64_t fr, int64_t n_inner) {
    const uint32_t o = (uint32_t)fr / (uint32_t)n_inner, i = (uint32_t)fr - o * (uint32_t)n_inner;
    return v.p + (int64_t)o * v.so + (int64_t)i * v.si;
}

// ------------------------------------------------------------------------------------------------------------ float32
typedef atacom::mfma_v4f V4;

// One MlpLdsM<4 CH, 64, 8> block with run-time n_in / n_out from six tensors; what is not written stays zero (padding of W1,
// rows >= n_out of W3).  The caller has zeroed the block.  per_output(i) runs beside the store of b3[i], i < n_out: what else a
// unit stages per output (the gradient kernel: std) shares that loop and its wait for memory, as it did before the code was shared.
template <int CH, typename PerOutput>
__device__ __forceinline__ void stage_block(float* lds, const float* W1, const float* b1, const float* W2, const float* b2,
                                            const float* W3, const float* b3, int n_in, int n_out, int tid, int nthreads,
                                            PerOutput&& per_output) {
    using L = atacom::MlpLdsM<4 * CH, H, NK>;
    for (int i = tid; i < H * n_in; i += nthreads) {
        const int u = i / n_in, e = i % n_in;
        lds[L::W1 + u * L::S1 + (e / CH) * 8 + (e % CH)] = W1[i];
    }
    for (int i = tid; i < H * H; i += nthreads) lds[L::W2 + (i / H) * L::S2 + (i % H)] = W2[i];
    for (int i = tid; i < n_out * H; i += nthreads) lds[L::W3 + (i / H) * L::S2 + (i % H)] = W3[i];
    for (int i = tid; i < H; i += nthreads) { lds[L::B1 + i] = b1[i]; lds[L::B2 + i] = b2[i]; }
    for (int i = tid; i < n_out; i += nthreads) {
        lds[L::B3 + i] = b3[i];
        per_output(i);
    }
}

template <int CH>
__device__ __forceinline__ void stage_block(float* lds, const float* W1, const float* b1, const float* W2, const float* b2,
                                            const float* W3, const float* b3, int n_in, int n_out, int tid, int nthreads) {
    stage_block<CH>(lds, W1, b1, W2, b2, W3, b3, n_in, n_out, tid, nthreads, [](int) {});
}

// the block's shift / scale table, [g][8] like W1; padding: shift 0, scale 1
template <int CH>
__device__ __forceinline__ void stage_norm(float* lds, const float* shift, const float* scale, int n_in, int tid, int nthreads) {
    using L = atacom::MlpLdsM<4 * CH, H, NK>;
    for (int i = tid; i < 32; i += nthreads) {
        const int g = i / 8, s = i % 8, e = CH * g + s;
        const bool real = s < CH && e < n_in;
        lds[L::SHIFT + i] = (real && shift) ? shift[e] : 0.0f;
        lds[L::SCALE + i] = (real && scale) ? scale[e] : 1.0f;
    }
}

// The transposition buffer [16 rows][64 units]: written from the accumulator layout (lane (n16, g), tile t, register v = unit
// 16 t + 4 g + v of row n16), read as (row, unit) with the lanes of a read on consecutive units.
__device__ __forceinline__ void put(float* buf, const V4 (&h)[4], int n16, int g) {
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<V4*>(buf + n16 * 64 + ((16 * t + 4 * g + 16 * (n16 & 3)) & 63)) = h[t];
}

__device__ __forceinline__ float get(const float* buf, int row, int unit) {
    return buf[row * 64 + ((unit + 16 * (row & 3)) & 63)];
}

// delta <- delta * act'(a), from the activation h = act(a) itself; one wave-uniform branch
__device__ __forceinline__ void times_act_prime(V4 (&d)[4], const V4 (&h)[4], int activation) {
    if (activation == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v) d[t][v] = h[t][v] > 0.0f ? d[t][v] : 0.0f;
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v) d[t][v] *= __builtin_fmaf(-h[t][v], h[t][v], 1.0f);
    }
}

__device__ __forceinline__ float sum16(float v) {      // over the 16 lanes that share lane / 16, in every one of them
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ float sum64(float v) {      // over the wavefront, in every lane
    v = sum16(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// a wavefront's accumulators of the network's gradient, for the whole walk; WA: with dW2a (acc2a is dead without it)
template <int NT, bool WA = false>
struct Grads {
    V4 acc1[4][NT], acc2[4][4], acc2a[4], acc3[4], db1[4], db2[4];
    static constexpr int kSlots = 16 * (NT + 7 + (WA ? 1 : 0));     // registers of a lane = slots of the hand-over

    __device__ __forceinline__ void zero() {
        const V4 z = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            acc2a[t] = acc3[t] = db1[t] = db2[t] = z;
#pragma unroll
            for (int u = 0; u < 4; ++u) acc2[t][u] = z;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc1[t][nt] = z;
        }
    }
};

// dW1's B operand: input element 16 nt + n16 of a row, normalised as the forward pass does
template <int NT>
struct InputColumns {
    int e[NT];
    bool real[NT];
    float sh[NT], sc[NT];
};

template <int CH, int NT>
__device__ __forceinline__ InputColumns<NT> input_columns(const float* lds, int n_in, int n16) {
    using L = atacom::MlpLdsM<4 * CH, H, NK>;
    InputColumns<NT> c;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int e = 16 * nt + n16;
        c.real[nt] = e < n_in;
        c.e[nt] = c.real[nt] ? e : n_in - 1;
        c.sh[nt] = lds[L::SHIFT + 8 * (c.e[nt] / CH) + c.e[nt] % CH];
        c.sc[nt] = lds[L::SCALE + 8 * (c.e[nt] / CH) + c.e[nt] % CH];
    }
    return c;
}

// A block's loads, all under the full exec mask (an element past n_in is the last one again, and dropped): xin[s] = element
// CH g + s of the lane's own row `fr`, layer 1's B operand, and xb[s][nt] of the rows r0 + 4 s + g, the K index of dW1
template <int CH, int NT, typename P>
__device__ __forceinline__ void load_rows(const P& p, const float* lds, const InputColumns<NT>& c, int64_t r0, int64_t fr, int g,
                                          float (&xin)[CH], float (&xb)[4][NT]) {
    using L = atacom::MlpLdsM<4 * CH, H, NK>;
    const float* xr = row_ptr(p.x, fr, p.n_inner);
#pragma unroll
    for (int s = 0; s < CH; ++s) {
        const int e = CH * g + s;
        const float v = xr[e < p.n_in ? e : p.n_in - 1];
        xin[s] = e < p.n_in ? (v - lds[L::SHIFT + 8 * g + s]) * lds[L::SCALE + 8 * g + s] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float* xs = row_ptr(p.x, flat_row(p, r0 + 4 * s + g), p.n_inner);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float v = xs[c.e[nt]];
            xb[s][nt] = c.real[nt] ? (v - c.sh[nt]) * c.sc[nt] : 0.0f;
        }
    }
}

// layer 1 before its activation, from the staged block `net`: o[t][v] = unit 16 t + 4 g + v of row n16
template <int CH>
__device__ __forceinline__ void layer1(const float* net, const float (&xin)[CH], V4 (&o)[4], int n16, int g) {
    using L = atacom::MlpLdsM<4 * CH, H, NK>;
    float w1[4][8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        o[t] = *reinterpret_cast<const V4*>(net + L::B1 + 16 * t + 4 * g);
        const float* row = net + L::W1 + (16 * t + n16) * L::S1 + 8 * g;
        const V4 lo = *reinterpret_cast<const V4*>(row), hi = *reinterpret_cast<const V4*>(row + 4);
#pragma unroll
        for (int s = 0; s < 4; ++s) { w1[t][s] = lo[s]; w1[t][4 + s] = hi[s]; }
    }
#pragma unroll
    for (int s = 0; s < CH; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t) o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[t][s], xin[s], o[t], 0, 0, 0);
}

// The backward pass of a block whose dy lies in LDS, [16 rows][8] at t_del + 128 (written by this wavefront, not yet fenced):
// dW3, da2, dW2 (and dW2a), da1, dW1 and the bias gradients into `a`.  `lds` is the staged block of the weights; xb[s][nt] =
// element 16 nt + n16 of the first layer's input of row 4 s + g of the block and, with WA, asb[s] = as[n16] of that row: the B
// operands whose K index is the row.  t_act and t_del are the wavefront's two transposition buffers, free again when it returns.
template <int CH, int NT, bool WA>
__device__ __forceinline__ void backward(const float* lds, float* t_act, float* t_del, const V4 (&h1)[4], const V4 (&h2)[4],
                                         const float (&xb)[4][NT], const float (&asb)[4], int activation, int n16, int g,
                                         Grads<NT, WA>& a) {
    using L = atacom::MlpLdsM<4 * CH, H, NK>;
    const V4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    put(t_act, h2, n16, g);                                  // dW3's B operand; dy is its A operand
    atacom::wave_lds_fence();
    // ---- dW3[k][j] += sum_rows dy[row][k] h2[row][j]: M = k (n16 < 8), N = j, K = the row 4 s + g
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float ld = t_del[128 + (4 * s + g) * 8 + (n16 & 7)];
        const float x = n16 < 8 ? ld : 0.0f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            a.acc3[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, get(t_act, 4 * s + g, 16 * u + n16), a.acc3[u], 0, 0, 0);
    }
    // ---- da2 = (W3^T dy) * act'(a2): M = unit, N = row n16, K = the output 4 s + g
    V4 da[4] = {zero, zero, zero, zero};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float b = t_del[128 + n16 * 8 + 4 * s + g];       // dy[4 s + g] of this lane's own row
#pragma unroll
        for (int u = 0; u < 4; ++u)
            da[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[L::W3 + (4 * s + g) * L::S2 + 16 * u + n16], b, da[u], 0, 0, 0);
    }
    times_act_prime(da, h2, activation);
#pragma unroll
    for (int u = 0; u < 4; ++u) a.db2[u] += da[u];
    atacom::wave_lds_fence();                            // dW3 has read both buffers
    put(t_del, da, n16, g);
    put(t_act, h1, n16, g);
    atacom::wave_lds_fence();
    // ---- dW2[j][i] += sum_rows da2[row][j] h1[row][i];  dW2a[j][k] += sum_rows da2[row][j] as[row][k]
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float x[4], b[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { x[t] = get(t_del, 4 * s + g, 16 * t + n16); b[t] = get(t_act, 4 * s + g, 16 * t + n16); }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int u = 0; u < 4; ++u) a.acc2[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[t], b[u], a.acc2[t][u], 0, 0, 0);
            if constexpr (WA) a.acc2a[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[t], asb[s], a.acc2a[t], 0, 0, 0);
        }
    }
    // ---- da1 = (W2^T da2) * act'(a1): K-step (u, v) carries unit j = 16 u + 4 g + v, i.e. register v of da[u]
    V4 d1[4] = {zero, zero, zero, zero};
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const float* wrow = lds + L::W2 + (16 * u + 4 * g + v) * L::S2 + n16;
#pragma unroll
            for (int t = 0; t < 4; ++t) d1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wrow[16 * t], da[u][v], d1[t], 0, 0, 0);
        }
    times_act_prime(d1, h1, activation);
#pragma unroll
    for (int t = 0; t < 4; ++t) a.db1[t] += d1[t];
    atacom::wave_lds_fence();                            // dW2 has read the deltas
    put(t_del, d1, n16, g);
    atacom::wave_lds_fence();
    // ---- dW1[j][e] += sum_rows da1[row][j] xn[row][e]
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float x[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) x[t] = get(t_del, 4 * s + g, 16 * t + n16);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) a.acc1[t][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[t], xb[s][nt], a.acc1[t][nt], 0, 0, 0);
    }
    atacom::wave_lds_fence();                            // before the next block writes over the deltas
}

// ... of a network without the second branch
template <int CH, int NT>
__device__ __forceinline__ void backward(const float* lds, float* t_act, float* t_del, const V4 (&h1)[4], const V4 (&h2)[4],
                                         const float (&xb)[4][NT], int activation, int n16, int g, Grads<NT>& a) {
    const float none[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    backward<CH, NT, false>(lds, t_act, t_del, h1, h2, xb, none, activation, n16, g, a);
}

// the wavefront's sums of the bias gradients over the rows (lane % 16)
template <int NT, bool WA>
__device__ __forceinline__ void sum_biases(Grads<NT, WA>& a) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) { a.db1[t][v] = sum16(a.db1[t][v]); a.db2[t][v] = sum16(a.db2[t][v]); }
}

// The workgroup's sums: wavefronts 1, 2, 3 hand their registers to wavefront 0 through LDS, in that order.  Every register of
// every lane is handed over, [slot][lane]: the Grads<NT, WA>::kSlots of `a` first (per register acc1, acc2, acc2a with WA, acc3,
// db1, db2: the order is part of the bits), then the unit's own -- own(f, q) applies x = f(q++, x) to each of them, q counting
// on from kSlots.  The caller asserts that the slots fit the workgroup's LDS.
template <int NT, bool WA, typename Own>
__device__ __forceinline__ void hand_over(Grads<NT, WA>& a, float* lds, int wave, int lane, Own&& own) {
    auto each = [&](auto&& f) {
        int q = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) a.acc1[t][nt][v] = f(q++, a.acc1[t][nt][v]);
#pragma unroll
                for (int u = 0; u < 4; ++u) a.acc2[t][u][v] = f(q++, a.acc2[t][u][v]);
                if constexpr (WA) a.acc2a[t][v] = f(q++, a.acc2a[t][v]);
                a.acc3[t][v] = f(q++, a.acc3[t][v]);
                a.db1[t][v] = f(q++, a.db1[t][v]);
                a.db2[t][v] = f(q++, a.db2[t][v]);
            }
        own(f, q);
    };
    __syncthreads();
    for (int w = 1; w < kWaves; ++w) {
        if (wave == w) each([&](int q, float v) { lds[q * 64 + lane] = v; return v; });
        __syncthreads();
        if (wave == 0) each([&](int q, float v) { return v + lds[q * 64 + lane]; });
        __syncthreads();
    }
}

// the network part of the partial up to db2, in the layout of the gradient, and with WA dW2a [64][n_act] behind it (at
// NetOffsets::end): plain vector stores.  db3 is the unit's.
template <int NT, bool WA>
__device__ __forceinline__ void store_net(const Grads<NT, WA>& a, float* out, int n_in, int n_out, int n16, int g, int n_act = 0) {
    const NetOffsets o = net_offsets(n_in, n_out);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = 16 * t + 4 * g + v;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                if (16 * nt + n16 < n_in) out[j * n_in + 16 * nt + n16] = a.acc1[t][nt][v];
#pragma unroll
            for (int u = 0; u < 4; ++u) out[o.W2 + j * H + 16 * u + n16] = a.acc2[t][u][v];
            if (4 * g + v < n_out) out[o.W3 + (4 * g + v) * H + 16 * t + n16] = a.acc3[t][v];
            if constexpr (WA)
                if (n16 < n_act) out[o.end + j * n_act + n16] = a.acc2a[t][v];
            if (n16 == 0) { out[o.b1 + j] = a.db1[t][v]; out[o.b2 + j] = a.db2[t][v]; }
        }
}

// ------------------------------------------------------------------------------------------------------------ float64
__device__ __forceinline__ double act_prime(double h, int activation) {
    return activation == 0 ? (h > 0.0 ? 1.0 : 0.0) : __builtin_fma(-h, h, 1.0);
}

// the normalised row into its record
template <typename C, typename P>
__device__ __forceinline__ void load_row_f64(const P& p, int64_t fr, double* me, int c) {
    const double* xr = row_ptr(p.x, fr, p.n_inner);
    for (int e = c; e < p.n_in; e += 16) me[C::X + e] = (xr[e] - (p.shift ? p.shift[e] : 0.0)) * (p.scale ? p.scale[e] : 1.0);
}

// da2 and da1 of the thread's row from its dy, h2 and h1; all threads of the workgroup call it, between two barriers of theirs
template <typename C, typename P>
__device__ __forceinline__ void backward_f64(const P& p, double* me, bool live, int c) {
    if (live)
        for (int j = c; j < H; j += 16) {
            double a = 0.0;
            for (int k = 0; k < p.n_out; ++k) a = __builtin_fma(p.W3[k * H + j], me[C::DY + k], a);
            me[C::D2 + j] = a * act_prime(me[C::H2 + j], p.activation);
        }
    __syncthreads();
    if (live)
        for (int i = c; i < H; i += 16) {
            double a = 0.0;
            for (int j = 0; j < H; ++j) a = __builtin_fma(p.W2[j * H + i], me[C::D2 + j], a);
            me[C::D1 + i] = a * act_prime(me[C::H1 + i], p.activation);
        }
    __syncthreads();
}

// the two columns whose product, summed over the rows, is entry e of the network's gradient; false past its end (ca, cb untouched)
template <typename C>
__device__ __forceinline__ bool net_columns(int e, int n_in, const NetOffsets& o, int& ca, int& cb) {
    if (e < o.b1) { ca = C::D1 + e / n_in; cb = C::X + e % n_in; }
    else if (e < o.W2) ca = C::D1 + (e - o.b1);
    else if (e < o.b2) { ca = C::D2 + (e - o.W2) / H; cb = C::H1 + (e - o.W2) % H; }
    else if (e < o.W3) ca = C::D2 + (e - o.b2);
    else if (e < o.b3) { ca = C::DY + (e - o.W3) / H; cb = C::H2 + (e - o.W3) % H; }
    else if (e < o.end) ca = C::DY + (e - o.b3);
    else return false;
    return true;
}

// ... of a gradient that carries dW2a [64][n_act] behind the network's (C: column AS, the row's as)
template <typename C>
__device__ __forceinline__ bool net_columns(int e, int n_in, int n_act, const NetOffsets& o, int& ca, int& cb) {
    if (net_columns<C>(e, n_in, o, ca, cb)) return true;
    if (e >= o.end + H * n_act) return false;
    ca = C::D2 + (e - o.end) / n_act;
    cb = C::AS + (e - o.end) % n_act;
    return true;
}

// the tile's `rows` records into the thread's entries, then the barrier that frees the records
template <typename C, int NQ>
__device__ __forceinline__ void accumulate_f64(const double* rec, int rows, const int (&ca)[NQ], const int (&cb)[NQ], double (&acc)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        for (int rr = 0; rr < rows; ++rr) acc[q] = __builtin_fma(rec[rr * C::SIZE + ca[q]], rec[rr * C::SIZE + cb[q]], acc[q]);
    __syncthreads();
}

template <int NQ>
__device__ __forceinline__ void store_f64(double* out, int Q, int tid, const double (&acc)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        if (tid + kBlock * q < Q) out[tid + kBlock * q] = acc[q];
}

// ------------------------------------------------------------------------------------------------------------ the reduction
// Value i = blockIdx.x * kReduceValues + threadIdx.x % kReduceValues of the `blocks` partials of q_size values (0 past their
// end), in a fixed order: slice s of the workgroup's threads adds the partials s, s + kReduceSlices, ... in that order (the
// loads of a slice are independent, 128 bytes a partial), and the slices' sums are added in the order of s.  True, with the
// sum in `s`, in the thread of slice 0 that holds a value i < n of the kernel's output; every other thread is done.
template <typename T>
__device__ __forceinline__ bool sum_partials(const T* __restrict__ ws, int blocks, int q_size, int n, int i, T& s) {
    __shared__ T part[kReduceSlices][kReduceValues];
    const int v = threadIdx.x % kReduceValues, slice = threadIdx.x / kReduceValues;
    s = T(0);
    if (i < q_size)
        for (int b = slice; b < blocks; b += kReduceSlices) s += ws[(int64_t)b * q_size + i];
    part[slice][v] = s;
    __syncthreads();
    if (slice != 0 || i >= n) return false;
#pragma unroll
    for (int k = 1; k < kReduceSlices; ++k) s += part[k][v];
    return true;
}

}  // namespace atacom_mlp_backward
