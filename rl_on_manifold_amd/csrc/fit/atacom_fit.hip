// Kernels of libatacom_fit.so (include/atacom_fit_hip.h states the arithmetic): k_fit_gradient<T, CH>, the forward AND the
// backward pass of the 2 x 64 network of ../atacom_policy.h over the rows of a minibatch, and k_fit_reduce<T>, which adds the
// workgroups' partial sums.
//
// Borrowed, not restated: the LDS layout MlpLdsM, the operand mapping of mlp_forward_mfma and the wave-level fence are those of
// ../atacom_policy.h, which this unit includes and does not edit.  The forward pass is written out here (one block of 16 rows
// at a time) because the backward pass needs what mlp_forward_mfma discards: the activations h1 and h2.
//
// Float32, one wavefront, one block of 16 rows (lane = (n16, g) = (lane % 16, lane / 16)):
//   * forward, transposed as in atacom_policy.h: H^T = W X^T, so lane (n16, g) holds, in register v of tile t, unit
//     16 t + 4 g + v of row n16 -- for h1, h2 and, computed the same way from W3^T and W2^T, for da2 and da1.  The activation's
//     derivative meets the data gradient register by register; no mask is stored anywhere.
//   * the weight gradients dW = sum_r delta_r act_r^T have the ROW as the K index, so both operands are needed with
//     lane % 16 = unit, lane / 16 = row: the transposition of the above.  Each goes once through a [16 rows][64 units] buffer of
//     the wavefront's LDS staging area (put / get below; the column is rotated by 16 (row % 4) so that the b128 writes and the
//     b32 reads are both free of bank conflicts without padding: the two buffers are the 8 KB the evaluate kernel stages with).
//   * the accumulators of dW1, dW2, dW3 (16 NT + 64 + 16 registers, NT = 1 or 2 tiles of inputs), of the three bias gradients,
//     of d log std and of the statistics stay in registers for the whole walk: the kernel is bound to one wavefront per SIMD
//     (512 registers), and has no scratch.
// At the end of the walk the bias sums are added across lanes, the four wavefronts add their registers through LDS in wave order
// and wavefront 0 writes the workgroup's partial.  The walk is uniform per wavefront, so every lane reaches every MFMA and
// wave-level LDS exchange; a lane past the end reads the last row again and its dy is zero, which zeroes every contribution.
//
// Float64 pins the arithmetic: a workgroup takes 16 rows at a time, sixteen threads a row, the weights are read from memory, the
// rows' activations and gradients lie in LDS as one record per row, and every thread owns the gradient entries tid, tid + 256,
// ..., each the sum over rows of the product of two columns of the records.
#include "atacom_fit.h"
#include "../atacom_policy.h"

namespace atacom_fit {

constexpr int H = ATACOM_FIT_HIDDEN, NK = ATACOM_FIT_MAX_OUT;
constexpr int kExtra = 8;         // floats after the network block: [0] = the constant c of logp
constexpr int kStage = 2048;      // floats of staging per wavefront: two [16][64] transposition buffers

template <typename T>
struct Rows {
    const T* p;
    int64_t so, si;
};

template <typename T>
struct Params {
    const T *W1, *b1, *W2, *b2, *W3, *b3, *shift, *scale, *std;
    int n_in, n_out, activation, head;
    int64_t n_rows, n_inner;      // n_rows = M
    Rows<T> x, a, w, lp;
    const int64_t* idx;
    T lo, hi;                     // 1 - clip, 1 + clip
    T* workspace;
};

// the flat number of the call's row r; a row past the end is the last one again
template <typename T>
__device__ __forceinline__ int64_t flat_row(const Params<T>& p, int64_t r) {
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

// c = -(sum_k log std_k) - n_out log(2 pi) / 2, in double, rounded once (atacom_evaluate_hip.h)
template <typename T>
__device__ __forceinline__ T logp_constant(const Params<T>& p) {
    double c = -0.5 * p.n_out * 1.8378770664093454835606594728112;
    for (int k = 0; k < p.n_out; ++k) c -= ::log((double)p.std[k]);
    return (T)c;
}

// What a row contributes at the network's output: dy, its term of d log std, of the loss and of the statistics.  `live` is
// false for a row past the end, whose every contribution is zero.
template <typename T>
__device__ __forceinline__ void row_head(const Params<T>& p, int64_t fr, bool live, const T (&y)[NK], const T* std, T c,
                                         T (&dy)[NK], T (&ls)[NK], T (&st)[3]) {
    const T wgt = *row_ptr(p.w, fr, p.n_inner);
    if (p.head == ATACOM_FIT_VALUE) {
        const T d = y[0] - wgt;
#pragma unroll
        for (int k = 0; k < NK; ++k) dy[k] = ls[k] = T(0);
        dy[0] = live ? T(2) * d : T(0);
        st[0] = live ? d * d : T(0);
        st[1] = st[2] = T(0);
        return;
    }
    const T* ar = row_ptr(p.a, fr, p.n_inner);
    const T lpo = *row_ptr(p.lp, fr, p.n_inner);
    T z[NK], s = T(0);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        z[k] = T(0);
        if (k < p.n_out) {
            z[k] = (ar[k] - y[k]) / std[k];
            s = atacom::num<T>::fma(z[k], z[k], s);
        }
    }
    const T logp = atacom::num<T>::fma(T(-0.5), s, c);
    const T rho = atacom::num<T>::exp(logp - lpo);
    const bool inactive = (wgt > T(0) && rho > p.hi) || (wgt < T(0) && rho < p.lo);
    const T gr = (inactive || !live) ? T(0) : -(rho * wgt);
    const T clamped = atacom::num<T>::min(atacom::num<T>::max(rho, p.lo), p.hi);
    st[0] = live ? -atacom::num<T>::min(rho * wgt, clamped * wgt) : T(0);
    st[1] = (live && inactive) ? T(1) : T(0);
    st[2] = live ? lpo - logp : T(0);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        dy[k] = ls[k] = T(0);
        if (k < p.n_out) {
            dy[k] = gr * z[k] / std[k];
            ls[k] = gr * atacom::num<T>::fma(z[k], z[k], T(-1));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ float32
typedef atacom::mfma_v4f V4;

// MlpLdsM<4 CH, 64, 8> with run-time n_in / n_out; everything not written stays zero (padding of W1, rows >= n_out of W3)
template <int CH>
__device__ __forceinline__ void stage_mfma(const Params<float>& p, float* lds, int tid, int nthreads) {
    using L = atacom::MlpLdsM<4 * CH, H, NK>;
    for (int i = tid; i < L::NET + kExtra; i += nthreads) lds[i] = 0.0f;
    __syncthreads();
    for (int i = tid; i < H * p.n_in; i += nthreads) {
        const int u = i / p.n_in, e = i % p.n_in;
        lds[L::W1 + u * L::S1 + (e / CH) * 8 + (e % CH)] = p.W1[i];
    }
    for (int i = tid; i < H * H; i += nthreads) lds[L::W2 + (i / H) * L::S2 + (i % H)] = p.W2[i];
    for (int i = tid; i < p.n_out * H; i += nthreads) lds[L::W3 + (i / H) * L::S2 + (i % H)] = p.W3[i];
    for (int i = tid; i < H; i += nthreads) { lds[L::B1 + i] = p.b1[i]; lds[L::B2 + i] = p.b2[i]; }
    for (int i = tid; i < p.n_out; i += nthreads) {
        lds[L::B3 + i] = p.b3[i];
        lds[L::STD + i] = p.std ? p.std[i] : 1.0f;
    }
    for (int i = tid; i < 32; i += nthreads) {           // [g][8] like W1; padding: shift 0, scale 1
        const int g = i / 8, s = i % 8, e = CH * g + s;
        const bool real = s < CH && e < p.n_in;
        lds[L::SHIFT + i] = (real && p.shift) ? p.shift[e] : 0.0f;
        lds[L::SCALE + i] = (real && p.scale) ? p.scale[e] : 1.0f;
    }
    if (tid == 0 && p.head == ATACOM_FIT_PPO_CLIP) lds[L::NET] = logp_constant(p);
    __syncthreads();
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

template <int CH>
__device__ __forceinline__ void gradient_f32(const Params<float>& p) {
    constexpr int D = 4 * CH, NT = D > 16 ? 2 : 1;
    using L = atacom::MlpLdsM<D, H, NK>;
    __shared__ __attribute__((aligned(16))) float lds[L::NET + kExtra + kWaves * kStage];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n16 = lane & 15, g = lane >> 4;
    stage_mfma<CH>(p, lds, threadIdx.x, kBlock);
    float* t_act = lds + L::NET + kExtra + wave * kStage;      // activations [16][64]
    float* t_del = t_act + 1024;                                // deltas [16][64]; before them: y [16][8], dy [16][8]
    const float c = lds[L::NET];

    V4 acc1[4][NT], acc2[4][4], acc3[4], db1[4], db2[4];
    float db3[NK], dls[NK], st[3] = {0.0f, 0.0f, 0.0f};
    const V4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        acc3[t] = db1[t] = db2[t] = zero;
#pragma unroll
        for (int u = 0; u < 4; ++u) acc2[t][u] = zero;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc1[t][nt] = zero;
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) db3[k] = dls[k] = 0.0f;

    // dW1's B operand: input element 16 nt + n16 of a row, normalised as the forward pass does
    int e1[NT];
    bool real1[NT];
    float sh1[NT], sc1[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int e = 16 * nt + n16;
        real1[nt] = e < p.n_in;
        e1[nt] = real1[nt] ? e : p.n_in - 1;
        sh1[nt] = lds[L::SHIFT + 8 * (e1[nt] / CH) + e1[nt] % CH];
        sc1[nt] = lds[L::SCALE + 8 * (e1[nt] / CH) + e1[nt] % CH];
    }

    const int64_t n_tiles = (p.n_rows + kRowsF32 - 1) / kRowsF32;
    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wave; tile < n_tiles; tile += (int64_t)gridDim.x * kWaves) {
#pragma unroll 1
        for (int blk = 0; blk < kRowsF32 / 16; ++blk) {
            const int64_t r0 = tile * kRowsF32 + 16 * blk;
            if (r0 >= p.n_rows) break;                           // uniform: the whole block is past the end
            const int64_t r = r0 + n16;
            const bool live = r < p.n_rows;
            const int64_t fr = flat_row(p, r);
            // ---- loads, all under the full exec mask: an element past n_in is the last one again, and dropped
            const float* xr = row_ptr(p.x, fr, p.n_inner);
            float xin[CH];
#pragma unroll
            for (int s = 0; s < CH; ++s) {
                const int e = CH * g + s;
                const float v = xr[e < p.n_in ? e : p.n_in - 1];
                xin[s] = e < p.n_in ? (v - lds[L::SHIFT + 8 * g + s]) * lds[L::SCALE + 8 * g + s] : 0.0f;
            }
            float xb[4][NT];                                     // rows r0 + 4 s + g: the K index of dW1
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float* xs = row_ptr(p.x, flat_row(p, r0 + 4 * s + g), p.n_inner);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const float v = xs[e1[nt]];
                    xb[s][nt] = real1[nt] ? (v - sh1[nt]) * sc1[nt] : 0.0f;
                }
            }
            // ---- layer 1: h1[t][v] = unit 16 t + 4 g + v of row n16
            V4 h1[4], h2[4];
            {
                float w1[4][8];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    h1[t] = *reinterpret_cast<const V4*>(lds + L::B1 + 16 * t + 4 * g);
                    const float* row = lds + L::W1 + (16 * t + n16) * L::S1 + 8 * g;
                    const V4 lo = *reinterpret_cast<const V4*>(row), hi = *reinterpret_cast<const V4*>(row + 4);
#pragma unroll
                    for (int s = 0; s < 4; ++s) { w1[t][s] = lo[s]; w1[t][4 + s] = hi[s]; }
                }
#pragma unroll
                for (int s = 0; s < CH; ++s)
#pragma unroll
                    for (int t = 0; t < 4; ++t) h1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[t][s], xin[s], h1[t], 0, 0, 0);
            }
            atacom::mlp_act16(h1, p.activation);
            // ---- layer 2: K-step (t, v) carries unit 16 t + 4 g + v, i.e. register v of h1[t]
#pragma unroll
            for (int u = 0; u < 4; ++u) h2[u] = *reinterpret_cast<const V4*>(lds + L::B2 + 16 * u + 4 * g);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                V4 w[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) w[u] = *reinterpret_cast<const V4*>(lds + L::W2 + (16 * u + n16) * L::S2 + 16 * t + 4 * g);
#pragma unroll
                for (int v = 0; v < 4; ++v)
#pragma unroll
                    for (int u = 0; u < 4; ++u) h2[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u][v], h1[t][v], h2[u], 0, 0, 0);
            }
            atacom::mlp_act16(h2, p.activation);
            // ---- output layer: rows >= n_out of W3 are zero; two accumulators halve the dependent chain
            V4 oa = *reinterpret_cast<const V4*>(lds + L::B3 + 4 * g), ob = zero;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const V4 w = *reinterpret_cast<const V4*>(lds + L::W3 + n16 * L::S2 + 16 * t + 4 * g);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    if ((t & 1) == 0) oa = __builtin_amdgcn_mfma_f32_16x16x4f32(w[v], h2[t][v], oa, 0, 0, 0);
                    else ob = __builtin_amdgcn_mfma_f32_16x16x4f32(w[v], h2[t][v], ob, 0, 0, 0);
                }
            }
            // ---- the row's outputs to its four lanes; each of them forms the row's head (identically)
            if (g < 2) *reinterpret_cast<V4*>(t_del + n16 * 8 + 4 * g) = oa + ob;
            atacom::wave_lds_fence();
            float y[NK], dy[NK], ls[NK], s3[3];
            {
                const V4 m0 = *reinterpret_cast<const V4*>(t_del + n16 * 8), m1 = *reinterpret_cast<const V4*>(t_del + n16 * 8 + 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) { y[k] = m0[k]; y[4 + k] = m1[k]; }
            }
            row_head<float>(p, fr, live, y, lds + L::STD, c, dy, ls, s3);
#pragma unroll
            for (int k = 0; k < NK; ++k) { db3[k] += dy[k]; dls[k] += ls[k]; }
#pragma unroll
            for (int i = 0; i < 3; ++i) st[i] += s3[i];
            // dy [16][8] for dW3's A operand (the four lanes of a row store the same values), h2 for its B operand
            *reinterpret_cast<V4*>(t_del + 128 + n16 * 8) = V4{dy[0], dy[1], dy[2], dy[3]};
            *reinterpret_cast<V4*>(t_del + 128 + n16 * 8 + 4) = V4{dy[4], dy[5], dy[6], dy[7]};
            put(t_act, h2, n16, g);
            atacom::wave_lds_fence();
            // ---- dW3[k][j] += sum_rows dy[row][k] h2[row][j]: M = k (n16 < 8), N = j, K = the row 4 s + g
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float ld = t_del[128 + (4 * s + g) * 8 + (n16 & 7)];
                const float a = n16 < 8 ? ld : 0.0f;
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    acc3[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, get(t_act, 4 * s + g, 16 * u + n16), acc3[u], 0, 0, 0);
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
            times_act_prime(da, h2, p.activation);
#pragma unroll
            for (int u = 0; u < 4; ++u) db2[u] += da[u];
            atacom::wave_lds_fence();                            // dW3 has read both buffers
            put(t_del, da, n16, g);
            put(t_act, h1, n16, g);
            atacom::wave_lds_fence();
            // ---- dW2[j][i] += sum_rows da2[row][j] h1[row][i]
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float a[4], b[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) { a[t] = get(t_del, 4 * s + g, 16 * t + n16); b[t] = get(t_act, 4 * s + g, 16 * t + n16); }
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc2[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[u], acc2[t][u], 0, 0, 0);
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
            times_act_prime(d1, h1, p.activation);
#pragma unroll
            for (int t = 0; t < 4; ++t) db1[t] += d1[t];
            atacom::wave_lds_fence();                            // dW2 has read the deltas
            put(t_del, d1, n16, g);
            atacom::wave_lds_fence();
            // ---- dW1[j][e] += sum_rows da1[row][j] xn[row][e]
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float a[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) a[t] = get(t_del, 4 * s + g, 16 * t + n16);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc1[t][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], xb[s][nt], acc1[t][nt], 0, 0, 0);
            }
            atacom::wave_lds_fence();                            // before the next block writes y over the deltas
        }
    }

    // ---- the wavefront's sums: the bias gradients over the rows (lane % 16), the row heads over the lanes with g = 0
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) { db1[t][v] = sum16(db1[t][v]); db2[t][v] = sum16(db2[t][v]); }
#pragma unroll
    for (int k = 0; k < NK; ++k) { db3[k] = sum16(db3[k]); dls[k] = sum16(dls[k]); }
#pragma unroll
    for (int i = 0; i < 3; ++i) st[i] = sum16(st[i]);

    // ---- the workgroup's sums: wavefronts 1, 2, 3 hand their registers to wavefront 0 through LDS, in that order.  Every
    // register of every lane is handed over, [register][lane]: 131 + 16 NT rows of 64 floats over the network and the staging
    auto each = [&](auto&& f) {
        int q = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc1[t][nt][v] = f(q++, acc1[t][nt][v]);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc2[t][u][v] = f(q++, acc2[t][u][v]);
                acc3[t][v] = f(q++, acc3[t][v]);
                db1[t][v] = f(q++, db1[t][v]);
                db2[t][v] = f(q++, db2[t][v]);
            }
#pragma unroll
        for (int k = 0; k < NK; ++k) { db3[k] = f(q++, db3[k]); dls[k] = f(q++, dls[k]); }
#pragma unroll
        for (int i = 0; i < 3; ++i) st[i] = f(q++, st[i]);
    };
    static_assert((131 + 16 * NT) * 64 <= L::NET + kExtra + kWaves * kStage, "the hand-over fits the workgroup's LDS");
    __syncthreads();
    for (int w = 1; w < kWaves; ++w) {
        if (wave == w) each([&](int q, float v) { lds[q * 64 + lane] = v; return v; });
        __syncthreads();
        if (wave == 0) each([&](int q, float v) { return v + lds[q * 64 + lane]; });
        __syncthreads();
    }
    if (wave != 0) return;
    // ---- the partial, in the layout of grad: plain vector stores
    float* out = p.workspace + (int64_t)blockIdx.x * partial_size(p.n_in, p.n_out);
    const int oW1 = 0, ob1 = oW1 + H * p.n_in, oW2 = ob1 + H, ob2 = oW2 + H * H, oW3 = ob2 + H, ob3 = oW3 + H * p.n_out,
              ols = ob3 + p.n_out, ost = ols + p.n_out;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = 16 * t + 4 * g + v;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                if (16 * nt + n16 < p.n_in) out[oW1 + j * p.n_in + 16 * nt + n16] = acc1[t][nt][v];
#pragma unroll
            for (int u = 0; u < 4; ++u) out[oW2 + j * H + 16 * u + n16] = acc2[t][u][v];
            if (4 * g + v < p.n_out) out[oW3 + (4 * g + v) * H + 16 * t + n16] = acc3[t][v];
            if (n16 == 0) { out[ob1 + j] = db1[t][v]; out[ob2 + j] = db2[t][v]; }
        }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (k < p.n_out) { out[ob3 + k] = db3[k]; out[ols + k] = dls[k]; }
#pragma unroll
        for (int i = 0; i < 3; ++i) out[ost + i] = st[i];
        out[ost + 3] = 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------------------ float64
// One record per row of the tile, columns: h1 | h2 | da1 | da2 | xn | y | dy | d log std terms | statistics (3, and a 0) | 1
template <int D>
struct Rec {
    static constexpr int H1 = 0, H2 = H1 + H, D1 = H2 + H, D2 = D1 + H, X = D2 + H, Y = X + D, DY = Y + NK, LS = DY + NK,
                         ST = LS + NK, ONE = ST + 4, SIZE = ONE + 1;
};

template <int CH>
__device__ __forceinline__ void gradient_f64(const Params<double>& p) {
    constexpr int D = 4 * CH, R = kRowsF64;
    using C = Rec<D>;
    constexpr int kMaxQ = H * D + H + H * H + H + H * NK + NK + NK + ATACOM_FIT_STATS, NQ = (kMaxQ + kBlock - 1) / kBlock;
    __shared__ double rec[R * C::SIZE];
    const int tid = threadIdx.x, row = tid >> 4, c = tid & 15;
    const int Q = (int)partial_size(p.n_in, p.n_out);
    const int ob1 = H * p.n_in, oW2 = ob1 + H, ob2 = oW2 + H * H, oW3 = ob2 + H, ob3 = oW3 + H * p.n_out, ols = ob3 + p.n_out,
              ost = ols + p.n_out;
    // the two columns whose product, summed over the rows, is this thread's entry q; past the end: 0 * 1
    int ca[NQ], cb[NQ];
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int e = tid + kBlock * q;
        acc[q] = 0.0;
        ca[q] = C::ST + 3;
        cb[q] = C::ONE;
        if (e < ob1) { ca[q] = C::D1 + e / p.n_in; cb[q] = C::X + e % p.n_in; }
        else if (e < oW2) ca[q] = C::D1 + (e - ob1);
        else if (e < ob2) { ca[q] = C::D2 + (e - oW2) / H; cb[q] = C::H1 + (e - oW2) % H; }
        else if (e < oW3) ca[q] = C::D2 + (e - ob2);
        else if (e < ob3) { ca[q] = C::DY + (e - oW3) / H; cb[q] = C::H2 + (e - oW3) % H; }
        else if (e < ols) ca[q] = C::DY + (e - ob3);
        else if (e < ost) ca[q] = C::LS + (e - ols);
        else if (e < Q) ca[q] = C::ST + (e - ost);
    }
    const double cst = p.head == ATACOM_FIT_PPO_CLIP ? logp_constant(p) : 0.0;
    const int64_t n_tiles = (p.n_rows + R - 1) / R;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * R + row;
        const bool live = r < p.n_rows;
        const int64_t left = p.n_rows - tile * R;
        const int rows = left < R ? (int)left : R;
        const int64_t fr = flat_row(p, r);
        double* me = rec + row * C::SIZE;
        if (live) {
            const double* xr = row_ptr(p.x, fr, p.n_inner);
            for (int e = c; e < p.n_in; e += 16) me[C::X + e] = (xr[e] - (p.shift ? p.shift[e] : 0.0)) * (p.scale ? p.scale[e] : 1.0);
            if (c == 0) { me[C::ONE] = 1.0; me[C::ST + 3] = 0.0; }
        }
        __syncthreads();
        if (live)
            for (int j = c; j < H; j += 16) {
                double a = p.b1[j];
                for (int e = 0; e < p.n_in; ++e) a = __builtin_fma(p.W1[j * p.n_in + e], me[C::X + e], a);
                me[C::H1 + j] = atacom::mlp_act(a, p.activation);
            }
        __syncthreads();
        if (live)
            for (int j = c; j < H; j += 16) {
                double a = p.b2[j];
                for (int i = 0; i < H; ++i) a = __builtin_fma(p.W2[j * H + i], me[C::H1 + i], a);
                me[C::H2 + j] = atacom::mlp_act(a, p.activation);
            }
        __syncthreads();
        if (live && c < p.n_out) {
            double a = p.b3[c];
            for (int j = 0; j < H; ++j) a = __builtin_fma(p.W3[c * H + j], me[C::H2 + j], a);
            me[C::Y + c] = a;
        }
        __syncthreads();
        if (live && c == 0) {
            double y[NK], dy[NK], ls[NK], s3[3];
#pragma unroll
            for (int k = 0; k < NK; ++k) y[k] = k < p.n_out ? me[C::Y + k] : 0.0;
            row_head<double>(p, fr, true, y, p.std, cst, dy, ls, s3);
#pragma unroll
            for (int k = 0; k < NK; ++k) { me[C::DY + k] = dy[k]; me[C::LS + k] = ls[k]; }
#pragma unroll
            for (int i = 0; i < 3; ++i) me[C::ST + i] = s3[i];
        }
        __syncthreads();
        if (live)
            for (int j = c; j < H; j += 16) {
                double a = 0.0;
                for (int k = 0; k < p.n_out; ++k) a = __builtin_fma(p.W3[k * H + j], me[C::DY + k], a);
                const double h = me[C::H2 + j];
                me[C::D2 + j] = a * (p.activation == 0 ? (h > 0.0 ? 1.0 : 0.0) : 1.0 - h * h);
            }
        __syncthreads();
        if (live)
            for (int i = c; i < H; i += 16) {
                double a = 0.0;
                for (int j = 0; j < H; ++j) a = __builtin_fma(p.W2[j * H + i], me[C::D2 + j], a);
                const double h = me[C::H1 + i];
                me[C::D1 + i] = a * (p.activation == 0 ? (h > 0.0 ? 1.0 : 0.0) : 1.0 - h * h);
            }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            for (int rr = 0; rr < rows; ++rr) acc[q] = __builtin_fma(rec[rr * C::SIZE + ca[q]], rec[rr * C::SIZE + cb[q]], acc[q]);
        __syncthreads();
    }
    double* out = p.workspace + (int64_t)blockIdx.x * Q;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
        if (tid + kBlock * q < Q) out[tid + kBlock * q] = acc[q];
}

// one wavefront per SIMD: the float32 kernel keeps up to 163 accumulator registers next to its operands
template <typename T, int CH>
__global__ __launch_bounds__(kBlock, 1) void k_fit_gradient(const Params<T> p) {
    if constexpr (std::is_same<T, float>::value) gradient_f32<CH>(p);
    else gradient_f64<CH>(p);
}

// grad and stats from the partials, in a fixed order: a workgroup takes kReduceValues consecutive values, slice s of its
// threads adds the partials s, s + kReduceSlices, ... in that order (the loads of a slice are independent, 128 bytes a
// partial), and the slices' sums are added in the order of s
template <typename T>
__global__ __launch_bounds__(kReduceBlock) void k_fit_reduce(const T* __restrict__ ws, int blocks, int q_size, int n_grad,
                                                             T* __restrict__ grad, T* __restrict__ stats, T m) {
    __shared__ T part[kReduceSlices][kReduceValues];
    const int v = threadIdx.x % kReduceValues, slice = threadIdx.x / kReduceValues;
    const int i = blockIdx.x * kReduceValues + v;
    T s = T(0);
    if (i < q_size)
        for (int b = slice; b < blocks; b += kReduceSlices) s += ws[(int64_t)b * q_size + i];
    part[slice][v] = s;
    __syncthreads();
    if (slice != 0 || i >= q_size) return;
#pragma unroll
    for (int k = 1; k < kReduceSlices; ++k) s += part[k][v];
    s = s / m;
    if (i < n_grad) grad[i] = s;
    else if (i >= q_size - ATACOM_FIT_STATS) stats[i - (q_size - ATACOM_FIT_STATS)] = s;
}

namespace {

template <typename T>
Params<T> params(const atacom_fit_args& a, const atacom_mlp& net, int64_t rows) {
    Params<T> p{};
    p.W1 = (const T*)net.W1; p.b1 = (const T*)net.b1; p.W2 = (const T*)net.W2; p.b2 = (const T*)net.b2;
    p.W3 = (const T*)net.W3; p.b3 = (const T*)net.b3;
    p.shift = (const T*)net.obs_shift; p.scale = (const T*)net.obs_scale; p.std = (const T*)net.std;
    p.n_in = net.n_in; p.n_out = net.n_out; p.activation = net.activation; p.head = a.head;
    p.n_rows = rows; p.n_inner = a.n_inner;
    p.x = {(const T*)a.x.ptr, a.x.stride_outer, a.x.stride_inner};
    p.a = {(const T*)a.action.ptr, a.action.stride_outer, a.action.stride_inner};
    p.w = {(const T*)a.weight.ptr, a.weight.stride_outer, a.weight.stride_inner};
    p.lp = {(const T*)a.logp_old.ptr, a.logp_old.stride_outer, a.logp_old.stride_inner};
    p.idx = a.idx;
    p.lo = (T)(1.0 - a.clip); p.hi = (T)(1.0 + a.clip);
    p.workspace = (T*)a.workspace;
    return p;
}

template <typename T>
int launch(const atacom_fit_args& a, const atacom_mlp& net, int blocks, int64_t rows, hipStream_t s) {
    const Params<T> p = params<T>(a, net, rows);
#define FIT_GO(CH) \
    case CH: hipLaunchKernelGGL((k_fit_gradient<T, CH>), dim3(blocks), dim3(kBlock), 0, s, p); break
    switch ((net.n_in + 3) / 4) {
        FIT_GO(1); FIT_GO(2); FIT_GO(3); FIT_GO(4);
        FIT_GO(5); FIT_GO(6); FIT_GO(7); FIT_GO(8);
        default: return ATACOM_FIT_E_UNSUPPORTED;
    }
#undef FIT_GO
    const int q = (int)partial_size(net.n_in, net.n_out);
    const int n_grad = (int)grad_size(net.n_in, net.n_out) + (a.head == ATACOM_FIT_PPO_CLIP ? net.n_out : 0);
    hipLaunchKernelGGL((k_fit_reduce<T>), dim3((q + kReduceValues - 1) / kReduceValues), dim3(kReduceBlock), 0, s,
                       (const T*)a.workspace, blocks, q, n_grad, (T*)a.grad, (T*)a.stats, (T)rows);
    return ATACOM_FIT_OK;
}

}  // namespace

int fit_launch(const atacom_fit_args& a, const atacom_mlp& net, int blocks, int64_t rows, hipStream_t s) {
    if (a.dtype == ATACOM_FIT_F32) return launch<float>(a, net, blocks, rows, s);
    if (a.dtype == ATACOM_FIT_F64) return launch<double>(a, net, blocks, rows, s);
    return ATACOM_FIT_E_UNSUPPORTED;
}

}  // namespace atacom_fit
