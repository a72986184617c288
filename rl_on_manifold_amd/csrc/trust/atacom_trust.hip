// Kernels of libatacom_trust.so (include/atacom_trust_hip.h states the arithmetic): k_trust_fvp<T, CH>, the forward, the tangent
// AND the backward pass of the 2 x 64 network of ../atacom_policy.h over the rows of a collection, and k_trust_reduce<T>, which
// adds the workgroups' partial sums, divides by the number of rows and adds the log-std block and the damping.
//
// Borrowed, not restated: the LDS layout MlpLdsM, the operand mapping of mlp_forward_mfma and the wave-level fence are those of
// ../atacom_policy.h, which this unit includes and does not edit.  The walk over the rows, the transposition buffers and the
// backward pass are those of ../fit/atacom_fit.hip (k_fit_gradient), written out here because that unit is a library of its own.
//
// Float32, one wavefront, one block of 16 rows (lane = (n16, g) = (lane % 16, lane / 16)):
//   * the direction's network part (V1, vb1, V2, vb2, V3, vb3) is staged as a SECOND MlpLdsM block behind the weights, so a
//     tangent product reads its A operand at the same offsets as the forward product, one block further;
//   * forward and tangent, transposed as in atacom_policy.h: H^T = W X^T, so lane (n16, g) holds, in register v of tile t, unit
//     16 t + 4 g + v of row n16 -- for h1, h2, t1, t2 and, computed the same way from W3^T and W2^T, for da2 and da1.  The
//     activation's derivative meets the tangent and the data gradient register by register; no mask is stored anywhere.  The
//     network's output itself is not needed and not formed;
//   * the weight gradients dW = sum_r delta_r act_r^T have the ROW as the K index: both operands go once through a [16 rows][64
//     units] buffer of the wavefront's LDS staging area (put / get below, the column rotated by 16 (row % 4));
//   * the accumulators of dW1, dW2, dW3 (16 NT + 64 + 16 registers, NT = 1 or 2 tiles of inputs) and of the three bias gradients
//     stay in registers for the whole walk: the kernel is bound to one wavefront per SIMD (512 registers), and has no scratch.
// At the end of the walk the bias sums are added across lanes, the four wavefronts add their registers through LDS in wave order
// and wavefront 0 writes the workgroup's partial.  The walk is uniform per wavefront, so every lane reaches every MFMA and
// wave-level LDS exchange; a lane past the end reads the last row again and its dy is zero, which zeroes every contribution.
//
// Float64 pins the arithmetic: a workgroup takes 16 rows at a time, sixteen threads a row, the weights and the direction are
// read from memory, the rows' activations, tangents and gradients lie in LDS as one record per row, and every thread owns the
// entries tid, tid + 256, ..., each the sum over rows of the product of two columns of the records.
#include "atacom_trust.h"
#include "../atacom_policy.h"

namespace atacom_trust {

constexpr int H = ATACOM_TRUST_HIDDEN, NK = ATACOM_TRUST_MAX_OUT;
constexpr int kExtra = 8;         // floats after the two network blocks: std_k^2 (1 past n_out)
constexpr int kStage = 2048;      // floats of staging per wavefront: two [16][64] transposition buffers

template <typename T>
struct Rows {
    const T* p;
    int64_t so, si;
};

template <typename T>
struct Params {
    const T *W1, *b1, *W2, *b2, *W3, *b3, *shift, *scale, *std;
    const T* v;                   // the direction, in the order of the partial
    int n_in, n_out, activation;
    int64_t n_rows, n_inner;      // n_rows = M
    Rows<T> x;
    const int64_t* idx;
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

// ------------------------------------------------------------------------------------------------------------ float32
typedef atacom::mfma_v4f V4;

// One MlpLdsM<4 CH, 64, 8> block with run-time n_in / n_out from six tensors; what is not written stays zero (padding of W1,
// rows >= n_out of W3).  The caller has zeroed the block.
template <int CH>
__device__ __forceinline__ void stage_block(float* lds, const float* W1, const float* b1, const float* W2, const float* b2,
                                            const float* W3, const float* b3, int n_in, int n_out, int tid, int nthreads) {
    using L = atacom::MlpLdsM<4 * CH, H, NK>;
    for (int i = tid; i < H * n_in; i += nthreads) {
        const int u = i / n_in, e = i % n_in;
        lds[L::W1 + u * L::S1 + (e / CH) * 8 + (e % CH)] = W1[i];
    }
    for (int i = tid; i < H * H; i += nthreads) lds[L::W2 + (i / H) * L::S2 + (i % H)] = W2[i];
    for (int i = tid; i < n_out * H; i += nthreads) lds[L::W3 + (i / H) * L::S2 + (i % H)] = W3[i];
    for (int i = tid; i < H; i += nthreads) { lds[L::B1 + i] = b1[i]; lds[L::B2 + i] = b2[i]; }
    for (int i = tid; i < n_out; i += nthreads) lds[L::B3 + i] = b3[i];
}

// [weights][direction][std^2]: the direction's tensors follow each other in p.v in the order of the partial
template <int CH>
__device__ __forceinline__ void stage_mfma(const Params<float>& p, float* lds, int tid, int nthreads) {
    using L = atacom::MlpLdsM<4 * CH, H, NK>;
    for (int i = tid; i < 2 * L::NET + kExtra; i += nthreads) lds[i] = 0.0f;
    __syncthreads();
    stage_block<CH>(lds, p.W1, p.b1, p.W2, p.b2, p.W3, p.b3, p.n_in, p.n_out, tid, nthreads);
    const float *V1 = p.v, *vb1 = V1 + H * p.n_in, *V2 = vb1 + H, *vb2 = V2 + H * H, *V3 = vb2 + H, *vb3 = V3 + p.n_out * H;
    stage_block<CH>(lds + L::NET, V1, vb1, V2, vb2, V3, vb3, p.n_in, p.n_out, tid, nthreads);
    for (int i = tid; i < NK; i += nthreads) {
        const float s = i < p.n_out ? p.std[i] : 1.0f;
        lds[2 * L::NET + i] = s * s;
    }
    for (int i = tid; i < 32; i += nthreads) {           // [g][8] like W1; padding: shift 0, scale 1
        const int g = i / 8, s = i % 8, e = CH * g + s;
        const bool real = s < CH && e < p.n_in;
        lds[L::SHIFT + i] = (real && p.shift) ? p.shift[e] : 0.0f;
        lds[L::SCALE + i] = (real && p.scale) ? p.scale[e] : 1.0f;
    }
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
__device__ __forceinline__ void fvp_f32(const Params<float>& p) {
    constexpr int D = 4 * CH, NT = D > 16 ? 2 : 1;
    using L = atacom::MlpLdsM<D, H, NK>;
    constexpr int kDir = L::NET;                                // the direction's block
    constexpr int kS2 = 2 * L::NET;                             // std^2
    __shared__ __attribute__((aligned(16))) float lds[2 * L::NET + kExtra + kWaves * kStage];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n16 = lane & 15, g = lane >> 4;
    stage_mfma<CH>(p, lds, threadIdx.x, kBlock);
    float* t_act = lds + 2 * L::NET + kExtra + wave * kStage;   // activations [16][64]
    float* t_del = t_act + 1024;                                // deltas [16][64]; before them, at 128: dy [16][8]
    const V4 s2 = *reinterpret_cast<const V4*>(lds + kS2 + 4 * (g & 1));

    V4 acc1[4][NT], acc2[4][4], acc3[4], db1[4], db2[4];
    const V4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    V4 db3 = zero;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        acc3[t] = db1[t] = db2[t] = zero;
#pragma unroll
        for (int u = 0; u < 4; ++u) acc2[t][u] = zero;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc1[t][nt] = zero;
    }

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
            // ---- layer 1, the weights and then the direction: h1[t][v], t1[t][v] = unit 16 t + 4 g + v of row n16
            V4 h1[4], h2[4], t1[4], t2[4];
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const float* net = lds + pass * kDir;
                V4(&o)[4] = pass ? t1 : h1;
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
            atacom::mlp_act16(h1, p.activation);
            times_act_prime(t1, h1, p.activation);
            // ---- layer 2: K-step (t, v) carries unit 16 t + 4 g + v, i.e. register v of h1[t] and of t1[t];
            //      t2 = W2 t1 + V2 h1 + vb2 shares the loads of W2 with h2
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                h2[u] = *reinterpret_cast<const V4*>(lds + L::B2 + 16 * u + 4 * g);
                t2[u] = *reinterpret_cast<const V4*>(lds + kDir + L::B2 + 16 * u + 4 * g);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                V4 w[4], d[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    w[u] = *reinterpret_cast<const V4*>(lds + L::W2 + (16 * u + n16) * L::S2 + 16 * t + 4 * g);
                    d[u] = *reinterpret_cast<const V4*>(lds + kDir + L::W2 + (16 * u + n16) * L::S2 + 16 * t + 4 * g);
                }
#pragma unroll
                for (int v = 0; v < 4; ++v)
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        h2[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u][v], h1[t][v], h2[u], 0, 0, 0);
                        t2[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u][v], t1[t][v], t2[u], 0, 0, 0);
                    }
#pragma unroll
                for (int v = 0; v < 4; ++v)
#pragma unroll
                    for (int u = 0; u < 4; ++u) t2[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(d[u][v], h1[t][v], t2[u], 0, 0, 0);
            }
            atacom::mlp_act16(h2, p.activation);
            times_act_prime(t2, h2, p.activation);
            // ---- output layer, tangent only: ty = W3 t2 + V3 h2 + vb3; rows >= n_out of W3 and V3 are zero
            V4 oa = *reinterpret_cast<const V4*>(lds + kDir + L::B3 + 4 * g), ob = zero;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const V4 w = *reinterpret_cast<const V4*>(lds + L::W3 + n16 * L::S2 + 16 * t + 4 * g);
                const V4 d = *reinterpret_cast<const V4*>(lds + kDir + L::W3 + n16 * L::S2 + 16 * t + 4 * g);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    oa = __builtin_amdgcn_mfma_f32_16x16x4f32(w[v], t2[t][v], oa, 0, 0, 0);
                    ob = __builtin_amdgcn_mfma_f32_16x16x4f32(d[v], h2[t][v], ob, 0, 0, 0);
                }
            }
            // ---- the head: lane (n16, g < 2) holds ty of outputs 4 g + v of row n16; dy = ty / std^2, zero past the end
            const V4 ty = oa + ob;
            V4 dy;
#pragma unroll
            for (int v = 0; v < 4; ++v) dy[v] = (live && g < 2) ? ty[v] / s2[v] : 0.0f;
            db3 += dy;
            // dy [16][8] for dW3's A operand, h2 for its B operand
            if (g < 2) *reinterpret_cast<V4*>(t_del + 128 + n16 * 8 + 4 * g) = dy;
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
            atacom::wave_lds_fence();                            // before the next block writes dy over the deltas
        }
    }

    // ---- the wavefront's sums: the bias gradients over the rows (lane % 16)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) { db1[t][v] = sum16(db1[t][v]); db2[t][v] = sum16(db2[t][v]); }
#pragma unroll
    for (int v = 0; v < 4; ++v) db3[v] = sum16(db3[v]);

    // ---- the workgroup's sums: wavefronts 1, 2, 3 hand their registers to wavefront 0 through LDS, in that order.  Every
    // register of every lane is handed over, [register][lane]: 116 + 16 NT rows of 64 floats over the staged blocks
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
        for (int v = 0; v < 4; ++v) db3[v] = f(q++, db3[v]);
    };
    static_assert((116 + 16 * NT) * 64 <= 2 * L::NET + kExtra + kWaves * kStage, "the hand-over fits the workgroup's LDS");
    __syncthreads();
    for (int w = 1; w < kWaves; ++w) {
        if (wave == w) each([&](int q, float v) { lds[q * 64 + lane] = v; return v; });
        __syncthreads();
        if (wave == 0) each([&](int q, float v) { return v + lds[q * 64 + lane]; });
        __syncthreads();
    }
    if (wave != 0) return;
    // ---- the partial, in the layout of out: plain vector stores
    float* out = p.workspace + (int64_t)blockIdx.x * net_size(p.n_in, p.n_out);
    const int oW1 = 0, ob1 = oW1 + H * p.n_in, oW2 = ob1 + H, ob2 = oW2 + H * H, oW3 = ob2 + H, ob3 = oW3 + H * p.n_out;
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
    if (n16 == 0 && g < 2) {
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (4 * g + v < p.n_out) out[ob3 + 4 * g + v] = db3[v];
    }
}

// ------------------------------------------------------------------------------------------------------------ float64
// One record per row of the tile, columns: h1 | h2 | t1 | t2 | da1 | da2 | xn | dy | 1
template <int D>
struct Rec {
    static constexpr int H1 = 0, H2 = H1 + H, T1 = H2 + H, T2 = T1 + H, D1 = T2 + H, D2 = D1 + H, X = D2 + H, DY = X + D,
                         ONE = DY + NK, SIZE = ONE + 1;
};

__device__ __forceinline__ double act_prime(double h, int activation) {
    return activation == 0 ? (h > 0.0 ? 1.0 : 0.0) : 1.0 - h * h;
}

template <int CH>
__device__ __forceinline__ void fvp_f64(const Params<double>& p) {
    constexpr int D = 4 * CH, R = kRowsF64;
    using C = Rec<D>;
    constexpr int kMaxQ = H * D + H + H * H + H + H * NK + NK, NQ = (kMaxQ + kBlock - 1) / kBlock;
    __shared__ double rec[R * C::SIZE];
    const int tid = threadIdx.x, row = tid >> 4, c = tid & 15;
    const int Q = (int)net_size(p.n_in, p.n_out);
    const int ob1 = H * p.n_in, oW2 = ob1 + H, ob2 = oW2 + H * H, oW3 = ob2 + H, ob3 = oW3 + H * p.n_out;
    const double *V1 = p.v, *vb1 = V1 + ob1, *V2 = p.v + oW2, *vb2 = p.v + ob2, *V3 = p.v + oW3, *vb3 = p.v + ob3;
    // the two columns whose product, summed over the rows, is this thread's entry q; past the end: 1 * 1, never written
    int ca[NQ], cb[NQ];
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int e = tid + kBlock * q;
        acc[q] = 0.0;
        ca[q] = C::ONE;
        cb[q] = C::ONE;
        if (e < ob1) { ca[q] = C::D1 + e / p.n_in; cb[q] = C::X + e % p.n_in; }
        else if (e < oW2) ca[q] = C::D1 + (e - ob1);
        else if (e < ob2) { ca[q] = C::D2 + (e - oW2) / H; cb[q] = C::H1 + (e - oW2) % H; }
        else if (e < oW3) ca[q] = C::D2 + (e - ob2);
        else if (e < ob3) { ca[q] = C::DY + (e - oW3) / H; cb[q] = C::H2 + (e - oW3) % H; }
        else if (e < Q) ca[q] = C::DY + (e - ob3);
    }
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
            if (c == 0) me[C::ONE] = 1.0;
        }
        __syncthreads();
        if (live)
            for (int j = c; j < H; j += 16) {
                double a = p.b1[j], t = vb1[j];
                for (int e = 0; e < p.n_in; ++e) a = __builtin_fma(p.W1[j * p.n_in + e], me[C::X + e], a);
                for (int e = 0; e < p.n_in; ++e) t = __builtin_fma(V1[j * p.n_in + e], me[C::X + e], t);
                const double h = atacom::mlp_act(a, p.activation);
                me[C::H1 + j] = h;
                me[C::T1 + j] = t * act_prime(h, p.activation);
            }
        __syncthreads();
        if (live)
            for (int j = c; j < H; j += 16) {
                double a = p.b2[j], t = vb2[j];
                for (int i = 0; i < H; ++i) a = __builtin_fma(p.W2[j * H + i], me[C::H1 + i], a);
                for (int i = 0; i < H; ++i) t = __builtin_fma(p.W2[j * H + i], me[C::T1 + i], t);
                for (int i = 0; i < H; ++i) t = __builtin_fma(V2[j * H + i], me[C::H1 + i], t);
                const double h = atacom::mlp_act(a, p.activation);
                me[C::H2 + j] = h;
                me[C::T2 + j] = t * act_prime(h, p.activation);
            }
        __syncthreads();
        if (live && c < p.n_out) {
            double t = vb3[c];
            for (int j = 0; j < H; ++j) t = __builtin_fma(p.W3[c * H + j], me[C::T2 + j], t);
            for (int j = 0; j < H; ++j) t = __builtin_fma(V3[c * H + j], me[C::H2 + j], t);
            const double s2 = p.std[c] * p.std[c];
            me[C::DY + c] = t / s2;
        }
        __syncthreads();
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

// one wavefront per SIMD: the float32 kernel keeps up to 148 accumulator registers next to its operands
template <typename T, int CH>
__global__ __launch_bounds__(kBlock, 1) void k_trust_fvp(const Params<T> p) {
    if constexpr (std::is_same<T, float>::value) fvp_f32<CH>(p);
    else fvp_f64<CH>(p);
}

// out from the partials, in a fixed order: a workgroup takes kReduceValues consecutive values, slice s of its threads adds the
// partials s, s + kReduceSlices, ... in that order, and the slices' sums are added in the order of s.  Then, each operation
// rounded on its own:  out_i = sum_i / M + d v_i  for the n_net values of the network,  out_k = 2 v_k + d v_k  for log std.
template <typename T>
__global__ __launch_bounds__(kReduceBlock) void k_trust_reduce(const T* __restrict__ ws, int blocks, int n_net, int n_out,
                                                               const T* __restrict__ dir, T d, T* __restrict__ out, T m) {
#pragma clang fp contract(off)
    __shared__ T part[kReduceSlices][kReduceValues];
    const int v = threadIdx.x % kReduceValues, slice = threadIdx.x / kReduceValues;
    const int i = blockIdx.x * kReduceValues + v;
    T s = T(0);
    if (i < n_net)
        for (int b = slice; b < blocks; b += kReduceSlices) s += ws[(int64_t)b * n_net + i];
    part[slice][v] = s;
    __syncthreads();
    if (slice != 0 || i >= n_net + n_out) return;
#pragma unroll
    for (int k = 1; k < kReduceSlices; ++k) s += part[k][v];
    const T x = dir[i];
    const T fv = i < n_net ? s / m : T(2) * x;
    const T dv = d * x;
    out[i] = fv + dv;
}

namespace {

template <typename T>
Params<T> params(const atacom_trust_args& a, const atacom_mlp& net, int64_t rows) {
    Params<T> p{};
    p.W1 = (const T*)net.W1; p.b1 = (const T*)net.b1; p.W2 = (const T*)net.W2; p.b2 = (const T*)net.b2;
    p.W3 = (const T*)net.W3; p.b3 = (const T*)net.b3;
    p.shift = (const T*)net.obs_shift; p.scale = (const T*)net.obs_scale; p.std = (const T*)net.std;
    p.v = (const T*)a.v;
    p.n_in = net.n_in; p.n_out = net.n_out; p.activation = net.activation;
    p.n_rows = rows; p.n_inner = a.n_inner;
    p.x = {(const T*)a.x.ptr, a.x.stride_outer, a.x.stride_inner};
    p.idx = a.idx;
    p.workspace = (T*)a.workspace;
    return p;
}

template <typename T>
int launch(const atacom_trust_args& a, const atacom_mlp& net, int blocks, int64_t rows, hipStream_t s) {
    const Params<T> p = params<T>(a, net, rows);
#define TRUST_GO(CH) \
    case CH: hipLaunchKernelGGL((k_trust_fvp<T, CH>), dim3(blocks), dim3(kBlock), 0, s, p); break
    switch ((net.n_in + 3) / 4) {
        TRUST_GO(1); TRUST_GO(2); TRUST_GO(3); TRUST_GO(4);
        TRUST_GO(5); TRUST_GO(6); TRUST_GO(7); TRUST_GO(8);
        default: return ATACOM_TRUST_E_UNSUPPORTED;
    }
#undef TRUST_GO
    const int n_net = (int)net_size(net.n_in, net.n_out);
    hipLaunchKernelGGL((k_trust_reduce<T>), dim3((n_net + net.n_out + kReduceValues - 1) / kReduceValues), dim3(kReduceBlock), 0, s,
                       (const T*)a.workspace, blocks, n_net, (int)net.n_out, (const T*)a.v, (T)a.damping, (T*)a.out, (T)rows);
    return ATACOM_TRUST_OK;
}

}  // namespace

int trust_launch(const atacom_trust_args& a, const atacom_mlp& net, int blocks, int64_t rows, hipStream_t s) {
    if (a.dtype == ATACOM_TRUST_F32) return launch<float>(a, net, blocks, rows, s);
    if (a.dtype == ATACOM_TRUST_F64) return launch<double>(a, net, blocks, rows, s);
    return ATACOM_TRUST_E_UNSUPPORTED;
}

}  // namespace atacom_trust
