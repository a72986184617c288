// Kernels of libatacom_evaluate.so (include/atacom_evaluate_hip.h states the arithmetic): k_evaluate_mlp<T, CH>, the 2 x 64
// network of atacom_policy.h over the rows of a finished collection instead of inside an environment step.
//
// The network itself is borrowed, not restated: the LDS layouts MlpLdsM / MlpLds, mlp_obs_to_operand + mlp_forward_mfma (float,
// NB = 4: one wavefront = 64 rows, one row per lane) and mlp_forward (double, four lanes per row) are those of
// ../csrc/atacom_policy.h, which this unit includes and does not edit.  What it cannot take from there is the staging:
// mlp_stage_weights_mfma / mlp_stage_weights know n_in and n_out at compile time and would read past the arrays of a smaller
// network.  Here they are arguments (1 <= n_in <= 32, 1 <= n_out <= 8), so stage_mfma / stage_valu below write the same layouts
// with run-time sizes, and a kernel is instantiated per CH = ceil(n_in / 4) -- the K-steps of layer 1, the only thing the
// forward pass needs at compile time -- with 8 outputs, of which the rows past n_out of W3 are zero and are not stored.
//
// A workgroup stages the weights once and then walks the row tiles b, b + gridDim.x, ...; the walk is uniform per wavefront, so
// every lane reaches every MFMA, DPP move and wave-level LDS exchange (rows past the end are computed from zeros and not
// stored).  Registers and LDS only: no scratch in the float kernels, no atomics, plain vector stores.
#include "atacom_evaluate.h"
#include "atacom_policy.h"

namespace atacom_evaluate {

constexpr int H = ATACOM_EVALUATE_HIDDEN, NK = ATACOM_EVALUATE_MAX_OUT;
constexpr int kExtra = 8;      // floats after the network block: [0] = the constant c of logp

template <typename T>
struct Rows {
    T* p;
    int64_t so, si;
};

template <typename T>
struct Params {
    const T *W1, *b1, *W2, *b2, *W3, *b3, *shift, *scale, *std;
    int n_in, n_out, activation;
    int64_t n_rows, n_inner;
    Rows<const T> x, a;
    Rows<T> y, logp;
};

// the host admits at most 2^31 - 1 rows, so the row's (outer, inner) index is a 32-bit division; the offsets are 64-bit
template <typename T>
__device__ __forceinline__ T* row_ptr(const Rows<T>& v, int64_t r, int64_t n_inner) {
    const uint32_t o = (uint32_t)r / (uint32_t)n_inner, i = (uint32_t)r - o * (uint32_t)n_inner;
    return v.p + (int64_t)o * v.so + (int64_t)i * v.si;
}

// c = -(sum_k log std_k) - n_out log(2 pi) / 2, in double, rounded once
template <typename T>
__device__ __forceinline__ T logp_constant(const Params<T>& p) {
    double c = -0.5 * p.n_out * 1.8378770664093454835606594728112;
    for (int k = 0; k < p.n_out; ++k) c -= ::log((double)p.std[k]);
    return (T)c;
}

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
    if (tid == 0 && p.logp.p) lds[L::NET] = logp_constant(p);
    __syncthreads();
}

// MlpLds<4 CH, 64, 8> with run-time n_in / n_out
template <typename T, int CH>
__device__ __forceinline__ void stage_valu(const Params<T>& p, T* lds, int tid, int nthreads) {
    using L = atacom::MlpLds<4 * CH, H, NK>;
    for (int i = tid; i < L::TOTAL + kExtra; i += nthreads) lds[i] = T(0);
    __syncthreads();
    for (int i = tid; i < H * p.n_in; i += nthreads) lds[L::W1 + (i / p.n_in) * L::S1 + (i % p.n_in)] = p.W1[i];
    for (int i = tid; i < H * H; i += nthreads) lds[L::W2 + (i / H) * L::S2 + (i % H)] = p.W2[i];
    for (int i = tid; i < p.n_out * H; i += nthreads) lds[L::W3T + (i % H) * L::S3 + (i / H)] = p.W3[i];
    for (int i = tid; i < H; i += nthreads) { lds[L::B1 + i] = p.b1[i]; lds[L::B2 + i] = p.b2[i]; }
    for (int i = tid; i < p.n_out; i += nthreads) {
        lds[L::B3 + i] = p.b3[i];
        lds[L::STD + i] = p.std ? p.std[i] : T(1);
    }
    for (int i = tid; i < 4 * CH; i += nthreads) {
        const bool real = i < p.n_in;
        lds[L::SHIFT + i] = (real && p.shift) ? p.shift[i] : T(0);
        lds[L::SCALE + i] = (real && p.scale) ? p.scale[i] : T(1);
    }
    if (tid == 0 && p.logp.p) lds[L::TOTAL] = logp_constant(p);
    __syncthreads();
}

// what a row's owner does with its mean: y, and logp = fma(-1/2, sum_k z_k^2, c)
template <typename T>
__device__ __forceinline__ void store_row(const Params<T>& p, int64_t r, const T (&mean)[NK], const T (&act)[NK],
                                          const T* std, T c) {
#pragma clang fp contract(off)
    if (p.y.p) {
        T* yr = row_ptr(p.y, r, p.n_inner);
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (k < p.n_out) yr[k] = mean[k];
    }
    if (p.logp.p) {
        T s = T(0);
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (k < p.n_out) {
                const T z = (act[k] - mean[k]) / std[k];
                s = atacom::num<T>::fma(z, z, s);
            }
        *row_ptr(p.logp, r, p.n_inner) = atacom::num<T>::fma(T(-0.5), s, c);
    }
}

// float: two wavefronts per SIMD, i.e. at most 256 registers (atacom_evaluate.h: kResident); double takes what it needs
template <typename T> constexpr int kWavesPerSimd = std::is_same<T, float>::value ? 2 : 1;

template <typename T, int CH>
__global__ __launch_bounds__(kBlock, kWavesPerSimd<T>) void k_evaluate_mlp(const Params<T> p) {
    constexpr int D = 4 * CH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if constexpr (std::is_same<T, float>::value) {
        using L = atacom::MlpLdsM<D, H, NK>;
        constexpr int NB = kRowsF32 / 16;
        // Per-wave staging: the 64 x 32 floats through which mlp_obs_to_operand turns the rows into B operands.  The 64 x 8
        // floats through which mlp_forward_mfma hands the outputs back to their lanes lie, in MlpLdsM, behind them at
        // act_offset(NB); here they are laid OVER them -- the operands are in registers by then, and both functions end in a
        // wave-level fence -- by handing mlp_forward_mfma the staging pointer moved back by that offset (it reads and writes
        // nothing below stage + act_offset).  That is 8 KB a wavefront instead of 10, and four wavefronts fit the 64 KB of a
        // workgroup next to the weights.
        constexpr int kStage = L::act_offset(NB);
        static_assert(L::wave_stage(NB) - kStage <= kStage, "the outputs fit over the operands");
        __shared__ __attribute__((aligned(16))) float lds[L::NET + kExtra + kWaves * kStage];
        stage_mfma<CH>(p, lds, threadIdx.x, kBlock);
        float* stage = lds + L::NET + kExtra + wave * kStage;
        const int64_t n_tiles = (p.n_rows + kRowsF32 - 1) / kRowsF32;
        // The rows of the next tile and the actions of this one are requested before the network runs, and arrive behind its
        // 300 to 450 MFMAs.  Loads are not predicated per lane: a lane past the end reads the last row again (and stores
        // nothing), so every load runs under the full exec mask and the conditions left, c < n_in and k < n_out, are scalar.
        const int64_t step = (int64_t)gridDim.x * kWaves, last = p.n_rows - 1;
        auto load_rows = [&](int64_t tile, float (&obs)[D]) {
            const int64_t r = tile * kRowsF32 + lane;
            const float* xr = row_ptr(p.x, r < last ? r : last, p.n_inner);
#pragma unroll
            for (int c = 0; c < D; ++c) obs[c] = c < p.n_in ? xr[c] : 0.0f;
        };
        float obs[D];
        int64_t tile = (int64_t)blockIdx.x * kWaves + wave;
        load_rows(tile, obs);
        for (; tile < n_tiles; tile += step) {
            const int64_t r = tile * kRowsF32 + lane;
            float xin[NB][CH], mean[NK], next[D], act[NK];
            atacom::mlp_obs_to_operand<D, H, NK, NB>(lds, stage, obs, lane, lane, xin);
            load_rows(tile + step, next);
            const float* ar = row_ptr(p.a, r < last ? r : last, p.n_inner);      // not dereferenced without logp
#pragma unroll
            for (int k = 0; k < NK; ++k) act[k] = (p.logp.p && k < p.n_out) ? ar[k] : 0.0f;
            atacom::mlp_forward_mfma<D, H, NK, NB>(lds, stage - kStage, xin, p.activation, lane, lane, mean);
            if (r <= last) store_row<float>(p, r, mean, act, lds + L::STD, lds[L::NET]);
#pragma unroll
            for (int c = 0; c < D; ++c) obs[c] = next[c];
        }
    } else {
        using L = atacom::MlpLds<D, H, NK>;
        __shared__ __attribute__((aligned(32))) T lds[L::TOTAL + kExtra];
        stage_valu<T, CH>(p, lds, threadIdx.x, kBlock);
        const int lq = lane & 3;
        const int64_t n_tiles = (p.n_rows + kRowsF64 - 1) / kRowsF64;
        for (int64_t tile = (int64_t)blockIdx.x * kWaves + wave; tile < n_tiles; tile += (int64_t)gridDim.x * kWaves) {
            const int64_t r = tile * kRowsF64 + (lane >> 2);
            const bool live = r < p.n_rows;
            const T* xr = row_ptr(p.x, live ? r : 0, p.n_inner);
            T obs[D], mean[NK], act[NK];
#pragma unroll
            for (int c = 0; c < D; ++c) obs[c] = (live && c < p.n_in) ? xr[c] : T(0);
            const T* ar = row_ptr(p.a, live ? r : 0, p.n_inner);              // not dereferenced without logp
#pragma unroll
            for (int k = 0; k < NK; ++k) act[k] = (p.logp.p && live && lq == 0 && k < p.n_out) ? ar[k] : T(0);
            atacom::mlp_forward<T, D, H, NK, 4>(lds, lds, obs, p.activation, lq, mean);
            if (live && lq == 0) store_row<T>(p, r, mean, act, lds + L::STD, lds[L::TOTAL]);
        }
    }
}

namespace {

template <typename T>
Params<T> params(const atacom_evaluate_args& a, const atacom_mlp& net) {
    Params<T> p{};
    p.W1 = (const T*)net.W1; p.b1 = (const T*)net.b1; p.W2 = (const T*)net.W2; p.b2 = (const T*)net.b2;
    p.W3 = (const T*)net.W3; p.b3 = (const T*)net.b3;
    p.shift = (const T*)net.obs_shift; p.scale = (const T*)net.obs_scale; p.std = (const T*)net.std;
    p.n_in = net.n_in; p.n_out = net.n_out; p.activation = net.activation;
    p.n_rows = a.n_outer * a.n_inner; p.n_inner = a.n_inner;
    p.x = {(const T*)a.x.ptr, a.x.stride_outer, a.x.stride_inner};
    p.a = {(const T*)a.action.ptr, a.action.stride_outer, a.action.stride_inner};
    p.y = {(T*)a.y.ptr, a.y.stride_outer, a.y.stride_inner};
    p.logp = {(T*)a.logp.ptr, a.logp.stride_outer, a.logp.stride_inner};
    return p;
}

template <typename T>
int launch(const atacom_evaluate_args& a, const atacom_mlp& net, int blocks, hipStream_t s) {
    const Params<T> p = params<T>(a, net);
#define EVALUATE_GO(CH) \
    case CH: hipLaunchKernelGGL((k_evaluate_mlp<T, CH>), dim3(blocks), dim3(kBlock), 0, s, p); break
    switch ((net.n_in + 3) / 4) {
        EVALUATE_GO(1); EVALUATE_GO(2); EVALUATE_GO(3); EVALUATE_GO(4);
        EVALUATE_GO(5); EVALUATE_GO(6); EVALUATE_GO(7); EVALUATE_GO(8);
        default: return ATACOM_EVALUATE_E_UNSUPPORTED;
    }
#undef EVALUATE_GO
    return ATACOM_EVALUATE_OK;
}

}  // namespace

int evaluate_launch(const atacom_evaluate_args& a, const atacom_mlp& net, int blocks, hipStream_t s) {
    if (a.dtype == ATACOM_EVALUATE_F32) return launch<float>(a, net, blocks, s);
    if (a.dtype == ATACOM_EVALUATE_F64) return launch<double>(a, net, blocks, s);
    return ATACOM_EVALUATE_E_UNSUPPORTED;
}

}  // namespace atacom_evaluate
