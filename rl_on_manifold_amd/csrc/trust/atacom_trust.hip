// Kernels of libatacom_trust.so (include/atacom_trust_hip.h states the arithmetic): k_trust_fvp<T, CH>, the forward, the tangent
// AND the backward pass of the 2 x 64 network of ../atacom_policy.h over the rows of a collection, and k_trust_reduce<T>, which
// adds the workgroups' partial sums, divides by the number of rows and adds the log-std block and the damping.
//
// Borrowed, not restated.  From ../atacom_policy.h: the LDS layout MlpLdsM, the operand mapping of mlp_forward_mfma and the
// wave-level fence.  From ../mlp/atacom_mlp_backward.h (namespace atacom_mlp_backward, shared with the gradient library's unit),
// whose header describes the mappings: the row views and their walk (Rows, flat_row, row_ptr, load_rows), the staging of a
// block and of the shift / scale table, layer 1, the transposition buffers, the backward pass of a block from dy on (backward),
// the accumulators (Grads) with their bias sums, hand-over between the wavefronts and store, the float64 backward loops, column
// pairs and accumulation, the slice sum of the reduction and the CH switch of the launcher.
//
// This unit's own.  Float32:
//   * the direction's network part (V1, vb1, V2, vb2, V3, vb3) is staged as a SECOND MlpLdsM block behind the weights, so a
//     tangent product reads its A operand at the same offsets as the forward product, one block further (layer 1 is the shared
//     one, run once per block), and std^2 behind both;
//   * the fused forward / tangent layers 2 and 3, which share the loads of W2: t1, t2 lie in registers like h1, h2, the
//     activation's derivative meets the tangent register by register, and the network's output itself is not formed;
//   * the head dy = ty / std^2 and, in the hand-over and the partial, db3, which stays in registers for the whole walk like
//     Grads (the kernel is bound to one wavefront per SIMD, 512 registers, and has no scratch).
// The walk is uniform per wavefront, so every lane reaches every MFMA and wave-level LDS exchange; a lane past the end reads the
// last row again and its dy is zero, which zeroes every contribution.
//
// Float64 pins the arithmetic: a workgroup takes 16 rows at a time, sixteen threads a row, the weights and the direction are
// read from memory, the rows' activations, tangents and gradients lie in LDS as one record per row (Rec), and every thread owns
// the entries tid, tid + 256, ..., each the sum over rows of the product of two columns of the records.
#include "atacom_trust.h"

namespace atacom_trust {

static_assert(H == ATACOM_TRUST_HIDDEN && NK == ATACOM_TRUST_MAX_OUT, "the shared backward pass is that of this library's network");
constexpr int kExtra = 8;         // floats after the two network blocks: std_k^2 (1 past n_out)

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

// ------------------------------------------------------------------------------------------------------------ float32
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
    stage_norm<CH>(lds, p.shift, p.scale, p.n_in, tid, nthreads);
    __syncthreads();
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

    Grads<NT> acc;
    acc.zero();
    const V4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    V4 db3 = zero;
    const InputColumns<NT> cols = input_columns<CH, NT>(lds, p.n_in, n16);

    const int64_t n_tiles = (p.n_rows + kRowsF32 - 1) / kRowsF32;
    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wave; tile < n_tiles; tile += (int64_t)gridDim.x * kWaves) {
#pragma unroll 1
        for (int blk = 0; blk < kRowsF32 / 16; ++blk) {
            const int64_t r0 = tile * kRowsF32 + 16 * blk;
            if (r0 >= p.n_rows) break;                           // uniform: the whole block is past the end
            const int64_t r = r0 + n16;
            const bool live = r < p.n_rows;
            const int64_t fr = flat_row(p, r);
            float xin[CH], xb[4][NT];
            load_rows<CH, NT>(p, lds, cols, r0, fr, g, xin, xb);
            // ---- layer 1, the weights and then the direction: h1[t][v], t1[t][v] = unit 16 t + 4 g + v of row n16
            V4 h1[4], h2[4], t1[4], t2[4];
            layer1<CH>(lds, xin, h1, n16, g);
            layer1<CH>(lds + kDir, xin, t1, n16, g);
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
            backward<CH, NT>(lds, t_act, t_del, h1, h2, xb, p.activation, n16, g, acc);
        }
    }

    // ---- the wavefront's sums: the bias gradients over the rows (lane % 16)
    sum_biases(acc);
#pragma unroll
    for (int v = 0; v < 4; ++v) db3[v] = sum16(db3[v]);

    // ---- the workgroup's sums, over the staged blocks; this unit's slots: db3
    static_assert((Grads<NT>::kSlots + 4) * 64 <= 2 * L::NET + kExtra + kWaves * kStage, "the hand-over fits the workgroup's LDS");
    hand_over(acc, lds, wave, lane, [&](auto&& f, int q) {
#pragma unroll
        for (int v = 0; v < 4; ++v) db3[v] = f(q++, db3[v]);
    });
    if (wave != 0) return;
    // ---- the partial, in the layout of out: plain vector stores
    float* out = p.workspace + (int64_t)blockIdx.x * net_size(p.n_in, p.n_out);
    store_net(acc, out, p.n_in, p.n_out, n16, g);
    const int ob3 = net_offsets(p.n_in, p.n_out).b3;
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

template <int CH>
__device__ __forceinline__ void fvp_f64(const Params<double>& p) {
    constexpr int D = 4 * CH, R = kRowsF64;
    using C = Rec<D>;
    constexpr int kMaxQ = H * D + H + H * H + H + H * NK + NK, NQ = (kMaxQ + kBlock - 1) / kBlock;
    __shared__ double rec[R * C::SIZE];
    const int tid = threadIdx.x, row = tid >> 4, c = tid & 15;
    const int Q = (int)net_size(p.n_in, p.n_out);
    const NetOffsets o = net_offsets(p.n_in, p.n_out);
    const double *V1 = p.v, *vb1 = p.v + o.b1, *V2 = p.v + o.W2, *vb2 = p.v + o.b2, *V3 = p.v + o.W3, *vb3 = p.v + o.b3;
    // the two columns whose product, summed over the rows, is this thread's entry q; past the end: 1 * 1, never written
    int ca[NQ], cb[NQ];
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        acc[q] = 0.0;
        ca[q] = C::ONE;
        cb[q] = C::ONE;
        net_columns<C>(tid + kBlock * q, p.n_in, o, ca[q], cb[q]);
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
            load_row_f64<C>(p, fr, me, c);
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
        backward_f64<C>(p, me, live, c);
        accumulate_f64<C>(rec, rows, ca, cb, acc);
    }
    store_f64(p.workspace + (int64_t)blockIdx.x * Q, Q, tid, acc);
}

// one wavefront per SIMD: the float32 kernel keeps up to 148 accumulator registers next to its operands
template <typename T, int CH>
__global__ __launch_bounds__(kBlock, 1) void k_trust_fvp(const Params<T> p) {
    if constexpr (std::is_same<T, float>::value) fvp_f32<CH>(p);
    else fvp_f64<CH>(p);
}

// out from the partials: a workgroup takes kReduceValues consecutive values, each summed in the fixed order of sum_partials.
// Then, each operation rounded on its own:  out_i = sum_i / M + d v_i  for the n_net values of the network,
// out_k = 2 v_k + d v_k  for log std.
template <typename T>
__global__ __launch_bounds__(kReduceBlock) void k_trust_reduce(const T* __restrict__ ws, int blocks, int n_net, int n_out,
                                                               const T* __restrict__ dir, T d, T* __restrict__ out, T m) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * kReduceValues + threadIdx.x % kReduceValues;
    T s;
    if (!sum_partials(ws, blocks, n_net, n_net + n_out, i, s)) return;
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
    if (!with_ch(net.n_in, [&](auto ch) {
            hipLaunchKernelGGL((k_trust_fvp<T, decltype(ch)::value>), dim3(blocks), dim3(kBlock), 0, s, p);
        }))
        return ATACOM_TRUST_E_UNSUPPORTED;
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
