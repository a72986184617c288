// Kernels of libatacom_fit.so (include/atacom_fit_hip.h states the arithmetic): k_fit_gradient<T, CH>, the forward AND the
// backward pass of the 2 x 64 network of ../atacom_policy.h over the rows of a minibatch, and k_fit_reduce<T>, which adds the
// workgroups' partial sums.
//
// Borrowed, not restated.  From ../atacom_policy.h: the LDS layout MlpLdsM, the operand mapping of mlp_forward_mfma and the
// wave-level fence.  From ../mlp/atacom_mlp_backward.h (namespace atacom_mlp_backward, shared with ../trust/atacom_trust.hip),
// whose header describes the mappings: the row views and their walk (Rows, flat_row, row_ptr, load_rows), the staging of a
// block and of the shift / scale table, layer 1, the transposition buffers, the backward pass of a block from dy on (backward),
// the accumulators (Grads) with their bias sums, hand-over between the wavefronts and store, the float64 backward loops, column
// pairs and accumulation, the slice sum of the reduction and the CH switch of the launcher.
//
// This unit's own.  Float32: the forward layers 2 and 3, written out (one block of 16 rows at a time) because the backward
// pass needs what mlp_forward_mfma discards, the activations h1 and h2; the row's head (row_head: dy, its term of d log std, of
// the loss and of the statistics) formed by the row's four lanes from the outputs exchanged through LDS; and the tail of the
// hand-over and of the partial: db3, d log std and the statistics, which stay in registers for the whole walk like Grads (the
// kernel is bound to one wavefront per SIMD, 512 registers, and has no scratch).  The walk is uniform per wavefront, so every
// lane reaches every MFMA and wave-level LDS exchange; a lane past the end reads the last row again and its dy is zero, which
// zeroes every contribution.
//
// Float64 pins the arithmetic: a workgroup takes 16 rows at a time, sixteen threads a row, the weights are read from memory, the
// rows' activations and gradients lie in LDS as one record per row (Rec), and every thread owns the gradient entries tid,
// tid + 256, ..., each the sum over rows of the product of two columns of the records.
#include "atacom_fit.h"

namespace atacom_fit {

static_assert(H == ATACOM_FIT_HIDDEN && NK == ATACOM_FIT_MAX_OUT, "the shared backward pass is that of this library's network");
constexpr int kExtra = 8;         // floats after the network block: [0] = the constant c of logp

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
// [weights][c]; std_k (1 where the network has none) and the shift / scale table in the block's own slots
template <int CH>
__device__ __forceinline__ void stage_mfma(const Params<float>& p, float* lds, int tid, int nthreads) {
    using L = atacom::MlpLdsM<4 * CH, H, NK>;
    for (int i = tid; i < L::NET + kExtra; i += nthreads) lds[i] = 0.0f;
    __syncthreads();
    stage_block<CH>(lds, p.W1, p.b1, p.W2, p.b2, p.W3, p.b3, p.n_in, p.n_out, tid, nthreads,
                    [&](int i) { lds[L::STD + i] = p.std ? p.std[i] : 1.0f; });
    stage_norm<CH>(lds, p.shift, p.scale, p.n_in, tid, nthreads);
    if (tid == 0 && p.head == ATACOM_FIT_PPO_CLIP) lds[L::NET] = logp_constant(p);
    __syncthreads();
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

    Grads<NT> acc;
    acc.zero();
    float db3[NK], dls[NK], st[3] = {0.0f, 0.0f, 0.0f};
    const V4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < NK; ++k) db3[k] = dls[k] = 0.0f;
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
            V4 h1[4], h2[4];
            layer1<CH>(lds, xin, h1, n16, g);
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
            backward<CH, NT>(lds, t_act, t_del, h1, h2, xb, p.activation, n16, g, acc);
        }
    }

    // ---- the wavefront's sums: the bias gradients over the rows (lane % 16), the row heads over the lanes with g = 0
    sum_biases(acc);
#pragma unroll
    for (int k = 0; k < NK; ++k) { db3[k] = sum16(db3[k]); dls[k] = sum16(dls[k]); }
#pragma unroll
    for (int i = 0; i < 3; ++i) st[i] = sum16(st[i]);

    // ---- the workgroup's sums, over the network block and the staging; this unit's slots: db3, d log std, the statistics
    static_assert((Grads<NT>::kSlots + 2 * NK + 3) * 64 <= L::NET + kExtra + kWaves * kStage, "the hand-over fits the workgroup's LDS");
    hand_over(acc, lds, wave, lane, [&](auto&& f, int q) {
#pragma unroll
        for (int k = 0; k < NK; ++k) { db3[k] = f(q++, db3[k]); dls[k] = f(q++, dls[k]); }
#pragma unroll
        for (int i = 0; i < 3; ++i) st[i] = f(q++, st[i]);
    });
    if (wave != 0) return;
    // ---- the partial, in the layout of grad: plain vector stores
    float* out = p.workspace + (int64_t)blockIdx.x * partial_size(p.n_in, p.n_out);
    store_net(acc, out, p.n_in, p.n_out, n16, g);
    const int ob3 = net_offsets(p.n_in, p.n_out).b3, ols = ob3 + p.n_out, ost = ols + p.n_out;
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
    const NetOffsets o = net_offsets(p.n_in, p.n_out);
    const int ols = o.end, ost = ols + p.n_out;
    // the two columns whose product, summed over the rows, is this thread's entry q; past the end: 0 * 1
    int ca[NQ], cb[NQ];
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int e = tid + kBlock * q;
        acc[q] = 0.0;
        ca[q] = C::ST + 3;
        cb[q] = C::ONE;
        if (net_columns<C>(e, p.n_in, o, ca[q], cb[q])) continue;
        if (e < ost) ca[q] = C::LS + (e - ols);
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
            load_row_f64<C>(p, fr, me, c);
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
        backward_f64<C>(p, me, live, c);
        accumulate_f64<C>(rec, rows, ca, cb, acc);
    }
    store_f64(p.workspace + (int64_t)blockIdx.x * Q, Q, tid, acc);
}

// one wavefront per SIMD: the float32 kernel keeps up to 163 accumulator registers next to its operands
template <typename T, int CH>
__global__ __launch_bounds__(kBlock, 1) void k_fit_gradient(const Params<T> p) {
    if constexpr (std::is_same<T, float>::value) gradient_f32<CH>(p);
    else gradient_f64<CH>(p);
}

// grad and stats from the partials: a workgroup takes kReduceValues consecutive values, each summed in the fixed order of
// sum_partials and divided by the number of rows
template <typename T>
__global__ __launch_bounds__(kReduceBlock) void k_fit_reduce(const T* __restrict__ ws, int blocks, int q_size, int n_grad,
                                                             T* __restrict__ grad, T* __restrict__ stats, T m) {
    const int i = blockIdx.x * kReduceValues + threadIdx.x % kReduceValues;
    T s;
    if (!sum_partials(ws, blocks, q_size, q_size, i, s)) return;
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
    if (!with_ch(net.n_in, [&](auto ch) {
            hipLaunchKernelGGL((k_fit_gradient<T, decltype(ch)::value>), dim3(blocks), dim3(kBlock), 0, s, p);
        }))
        return ATACOM_FIT_E_UNSUPPORTED;
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
