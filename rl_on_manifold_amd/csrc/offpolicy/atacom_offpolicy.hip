// Kernels of libatacom_offpolicy.so (include/atacom_offpolicy_hip.h states the arithmetic): k_offpolicy_net<T, CH>, which runs
// one to three 2 x 64 networks over the rows of a call as phases of a workgroup -- the critic alone (atacom_offpolicy_q), or
// the target actor and then one or two critics (atacom_offpolicy_target) -- and k_soft_update<T>.
//
// Borrowed from ../atacom_policy.h, which this unit includes and does not edit: the LDS layouts MlpLdsM / MlpLds, mlp_act16,
// wave_lds_fence and num<T>.  What cannot be borrowed is the forward pass: layer 2 of the critic accumulates the 16 K-steps of
// W2 h1 and then ceil(k / 4) more of W2a as, whose operand comes from the row's action, so forward_mfma / forward_valu below
// are this unit's own, with the number of action steps a wave-uniform argument (0 for the actor).  The staging has run-time
// n1 / n_out like that of atacom_evaluate.hip, and a kernel is instantiated per CH = ceil(n1 / 4), n1 the critic's first-layer
// width: the actor of a target call (n_in = D <= n1) is staged in the same layout, its W1 zero-padded.
//
// LDS (float32): one network block MlpLdsM<.., 64, 8>::NET, 8 floats, and 8 KB of staging per wavefront whose 64 x 8 outputs
// lie over the 64 x 32 operands -- the 63808 bytes of k_evaluate_mlp.  W2a [64][8] needs no room of its own: the W3 block of
// MlpLdsM has 16 rows so that every lane of the output layer's A operand reads one, the outputs 8 .. 15 that rows 8 .. 15
// produce are never stored, and a matrix-core output row depends on its own A row alone -- W2a lives in those rows.
//
// One network is resident at a time.  A workgroup takes one tile per wavefront, walks the phases over it -- restaging behind a
// barrier -- with the row's a'' and q_1 in the registers of the lane that owns the row, and then takes its next tiles
// (b + n_blocks, ...) the same way; a q call stages once.  The walk is uniform per workgroup, so every wavefront reaches every
// barrier, MFMA and wave-level LDS exchange.  Loads are not predicated per lane: a lane past the end reads the last row again
// and only its store is guarded.  Registers and LDS only: no scratch in the float kernels, no atomics, plain vector stores.
// Compiled with -ffp-contract=off (build.UNIT_FLAGS): the row arithmetic and the soft update are the individually rounded
// operations the header writes; the fused multiply-adds of the float64 networks are explicit.
#include "atacom_offpolicy.h"
#include "../atacom_policy.h"

namespace atacom_offpolicy {

constexpr int H = ATACOM_OFFPOLICY_HIDDEN, NK = ATACOM_OFFPOLICY_MAX_ACT;
constexpr int kExtra = 8;      // floats after the network block, unused: the block and the staging keep evaluate's offsets

template <typename T>
struct Rows {
    const T* p;
    int64_t so, si;
};

template <typename T>
struct Net {
    const T *W1, *b1, *W2, *b2, *W2a, *W3, *b3, *shift, *scale, *act_scale;
    int n1, n_out, activation, mean_mode;
};

template <typename T>
struct Params {
    Net<T> net[3];
    int has_actor, n_nets, kind, n_obs, n_act;
    int64_t n_rows, n_inner;
    const int64_t* idx;
    Rows<T> obs, action, reward, absorbing;
    const T* eps;
    int64_t eps_stride;
    const T *low, *high;
    T noise_std, noise_clip, gamma;
    T* y;
    int64_t y_stride;
    T* aout;
    int64_t aout_stride;
};

// the host admits at most 2^31 - 1 rows, so the row's (outer, inner) index is a 32-bit division; the offsets are 64-bit
template <typename T>
__device__ __forceinline__ const T* row_ptr(const Rows<T>& v, int64_t r, int64_t n_inner) {
    const uint32_t o = (uint32_t)r / (uint32_t)n_inner, i = (uint32_t)r - o * (uint32_t)n_inner;
    return v.p + (int64_t)o * v.so + (int64_t)i * v.si;
}

// ---- float32: MlpLdsM<4 CH, 64, 8> with run-time n1 / n_out, W2a in rows 8 .. 15 of the W3 block
template <int CH>
struct LdsM : atacom::MlpLdsM<4 * CH, H, NK> {
    using L = atacom::MlpLdsM<4 * CH, H, NK>;
    static constexpr int W2A = L::W3 + 8 * L::S2;      // [64][8]
    static constexpr int AUX = L::EXPLORE;             // [act_scale | low | high], 8 each
    static_assert(H * 8 <= 8 * L::S2, "W2a fits the unread half of the W3 block");
};

template <int CH>
__device__ __forceinline__ void stage_mfma(const Params<float>& p, const Net<float>& n, float* lds, int tid) {
    using L = LdsM<CH>;
    __syncthreads();                                   // the phase before has read its weights
    // Every word a phase reads is written here, the padding as zero where it is written at all: the W1 slots at or past n1
    // (the actor's n_in = D <= n1), the W3 rows and biases from n_out to 7, the W2a columns at or past n_act.  The columns 64 ..
    // 67 of the W2 / W3 rows, STD and the 8 floats after the block are read by nothing.
    for (int i = tid; i < H * L::S1; i += kBlock) {      // [unit][g][8], slot s of group g = element CH g + s
        const int u = i / L::S1, g = (i % L::S1) / 8, s = i % 8, e = CH * g + s;
        lds[L::W1 + i] = (s < CH && e < n.n1) ? n.W1[u * n.n1 + e] : 0.0f;
    }
    for (int i = tid; i < H * H; i += kBlock) lds[L::W2 + (i / H) * L::S2 + (i % H)] = n.W2[i];
    for (int i = tid; i < 8 * H; i += kBlock) lds[L::W3 + (i / H) * L::S2 + (i % H)] = i < n.n_out * H ? n.W3[i] : 0.0f;
    for (int i = tid; i < 8 * L::S2; i += kBlock) {      // rows 8 .. 15 of the W3 block: W2a [64][8], then zeros; zero for the actor
        const int u = i / 8, k = i % 8;
        lds[L::W2A + i] = (n.W2a && u < H && k < p.n_act) ? n.W2a[u * p.n_act + k] : 0.0f;
    }
    for (int i = tid; i < H; i += kBlock) { lds[L::B1 + i] = n.b1[i]; lds[L::B2 + i] = n.b2[i]; }
    for (int i = tid; i < 16; i += kBlock) lds[L::B3 + i] = i < n.n_out ? n.b3[i] : 0.0f;
    for (int i = tid; i < 32; i += kBlock) {             // [g][8] like W1; past the observation: shift 0, scale 1
        const int g = i / 8, s = i % 8, e = CH * g + s;
        const bool real = s < CH && e < p.n_obs;
        lds[L::SHIFT + i] = (real && n.shift) ? n.shift[e] : 0.0f;
        lds[L::SCALE + i] = (real && n.scale) ? n.scale[e] : 1.0f;
    }
    for (int i = tid; i < 8; i += kBlock) {
        const bool real = i < p.n_act;
        lds[L::AUX + i] = (real && n.act_scale) ? n.act_scale[i] : 1.0f;
        lds[L::AUX + 8 + i] = (real && p.low) ? p.low[i] : 0.0f;
        lds[L::AUX + 16 + i] = (real && p.high) ? p.high[i] : 0.0f;
    }
    __syncthreads();
}

// The rows of the wavefront -> the B operands of layer 1 (normalised) and of the action steps of layer 2.  Lane l owns row l
// of the tile; `cat` appends as to the row at n_obs (TD3: n_obs + n_act <= 4 CH).  as is zero past n_act.
template <int CH>
__device__ __forceinline__ void rows_to_operands(const float* __restrict__ net, float* __restrict__ stage, const float (&obs)[4 * CH],
                                                 const float (&as)[NK], int n_obs, int n_act, bool cat, int ka, int lane,
                                                 float (&xin)[4][CH], float (&aop)[4][2]) {
    using L = LdsM<CH>;
    using V4 = atacom::mfma_v4f;
    const int n16 = lane & 15, g = lane >> 4;
    float* row = stage + lane * 32;
    if (ka > 0) {
        *reinterpret_cast<V4*>(row) = V4{as[0], as[1], as[2], as[3]};
        *reinterpret_cast<V4*>(row + 4) = V4{as[4], as[5], as[6], as[7]};
    }
    atacom::wave_lds_fence();
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
        for (int j = 0; j < 2; ++j) aop[blk][j] = ka > 0 ? stage[(16 * blk + n16) * 32 + 4 * j + g] : 0.0f;
    atacom::wave_lds_fence();
#pragma unroll
    for (int q = 0; q < CH; ++q) *reinterpret_cast<V4*>(row + 4 * q) = V4{obs[4 * q], obs[4 * q + 1], obs[4 * q + 2], obs[4 * q + 3]};
    if (cat) {
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (k < n_act) row[n_obs + k] = as[k];
    }
    atacom::wave_lds_fence();
#pragma unroll
    for (int s = 0; s < CH; ++s) {
        const float sh = net[L::SHIFT + 8 * g + s], sc = net[L::SCALE + 8 * g + s];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) xin[blk][s] = (stage[(16 * blk + n16) * 32 + CH * g + s] - sh) * sc;
    }
    atacom::wave_lds_fence();
}

// The three layers on the matrix cores for the wavefront's four blocks of 16 rows, in the transposed form of
// atacom_policy.h (H^T = W X^T: the accumulator layout of a layer is the B-operand layout of the next): layer 2 takes `ka`
// further K-steps, A = W2a[unit][4 j + g], B = aop[blk][j] = as[4 j + g] of row 16 blk + n16.  out[o] = output o of this lane's
// row; the outputs travel through stage[row][8], which the caller lays over the operands (they are in registers by now).
template <int CH>
__device__ __forceinline__ void forward_mfma(const float* __restrict__ net, float* __restrict__ stage, const float (&xin)[4][CH],
                                             const float (&aop)[4][2], int ka, int activation, int lane, float (&out)[NK]) {
    using L = LdsM<CH>;
    using V4 = atacom::mfma_v4f;
    constexpr int NB = 4;
    const int n16 = lane & 15, g = lane >> 4;
    V4 h1[NB][4];
    float w1[4][8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const V4 bias = *reinterpret_cast<const V4*>(net + L::B1 + 16 * t + 4 * g);
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) h1[blk][t] = bias;
        const float* row = net + L::W1 + (16 * t + n16) * L::S1 + 8 * g;
        const V4 lo = *reinterpret_cast<const V4*>(row), hi = *reinterpret_cast<const V4*>(row + 4);
#pragma unroll
        for (int s = 0; s < 4; ++s) { w1[t][s] = lo[s]; w1[t][4 + s] = hi[s]; }
    }
#pragma unroll
    for (int s = 0; s < CH; ++s)
#pragma unroll
        for (int blk = 0; blk < NB; ++blk)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                h1[blk][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[t][s], xin[blk][s], h1[blk][t], 0, 0, 0);
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) atacom::mlp_act16(h1[blk], activation);
    // ---- layer 2: K-step (t, v) carries unit 16 t + 4 g + v, i.e. register v of h1[.][t]; then the action steps
    V4 h2[NB][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const V4 bias = *reinterpret_cast<const V4*>(net + L::B2 + 16 * u + 4 * g);
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) h2[blk][u] = bias;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        V4 w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = *reinterpret_cast<const V4*>(net + L::W2 + (16 * u + n16) * L::S2 + 16 * t + 4 * g);
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int blk = 0; blk < NB; ++blk)
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    h2[blk][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u][v], h1[blk][t][v], h2[blk][u], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j < ka) {                                   // wave-uniform
            float wa[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) wa[u] = net[L::W2A + (16 * u + n16) * 8 + 4 * j + g];
#pragma unroll
            for (int blk = 0; blk < NB; ++blk)
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    h2[blk][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[u], aop[blk][j], h2[blk][u], 0, 0, 0);
        }
    }
#pragma unroll
    for (int blk = 0; blk < NB; ++blk) atacom::mlp_act16(h2[blk], activation);
    // ---- output layer: only the rows < n_out of the W3 block are weights; what rows 8 .. 15 produce is not stored
    V4 o[NB];
    {
        const V4 bias = *reinterpret_cast<const V4*>(net + L::B3 + 4 * g);
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) o[blk] = bias;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const V4 w = *reinterpret_cast<const V4*>(net + L::W3 + n16 * L::S2 + 16 * t + 4 * g);
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int blk = 0; blk < NB; ++blk) o[blk] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[v], h2[blk][t][v], o[blk], 0, 0, 0);
    }
    // ---- back to the owners: lane (n16, g) holds outputs 4 g .. 4 g + 3 of row 16 blk + n16 -> [row][8]
    atacom::wave_lds_fence();
    if (g < 2) {
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) *reinterpret_cast<V4*>(stage + (16 * blk + n16) * 8 + 4 * g) = o[blk];
    }
    atacom::wave_lds_fence();
    const V4 m0 = *reinterpret_cast<const V4*>(stage + lane * 8), m1 = *reinterpret_cast<const V4*>(stage + lane * 8 + 4);
#pragma unroll
    for (int k = 0; k < NK; ++k) out[k] = k < 4 ? m0[k < 4 ? k : 0] : m1[k >= 4 ? k - 4 : 0];
    atacom::wave_lds_fence();
}

// ---- float64 (any T): MlpLds<4 CH, 64, 8> with run-time n1 / n_out, W2a [64][8] behind it
template <int CH>
struct LdsV : atacom::MlpLds<4 * CH, H, NK> {
    using L = atacom::MlpLds<4 * CH, H, NK>;
    static constexpr int AUX = L::EXPLORE;
    static constexpr int W2A = L::TOTAL;
    static constexpr int ALL = L::TOTAL + H * 8;
};

template <typename T, int CH>
__device__ __forceinline__ void stage_valu(const Params<T>& p, const Net<T>& n, T* lds, int tid) {
    using L = LdsV<CH>;
    __syncthreads();
    for (int i = tid; i < L::ALL; i += kBlock) lds[i] = T(0);
    __syncthreads();
    for (int i = tid; i < H * n.n1; i += kBlock) lds[L::W1 + (i / n.n1) * L::S1 + (i % n.n1)] = n.W1[i];
    for (int i = tid; i < H * H; i += kBlock) lds[L::W2 + (i / H) * L::S2 + (i % H)] = n.W2[i];
    for (int i = tid; i < n.n_out * H; i += kBlock) lds[L::W3T + (i % H) * L::S3 + (i / H)] = n.W3[i];
    if (n.W2a)
        for (int i = tid; i < H * p.n_act; i += kBlock) lds[L::W2A + (i / p.n_act) * 8 + (i % p.n_act)] = n.W2a[i];
    for (int i = tid; i < H; i += kBlock) { lds[L::B1 + i] = n.b1[i]; lds[L::B2 + i] = n.b2[i]; }
    for (int i = tid; i < n.n_out; i += kBlock) lds[L::B3 + i] = n.b3[i];
    for (int i = tid; i < 4 * CH; i += kBlock) {
        const bool real = i < p.n_obs;
        lds[L::SHIFT + i] = (real && n.shift) ? n.shift[i] : T(0);
        lds[L::SCALE + i] = (real && n.scale) ? n.scale[i] : T(1);
    }
    for (int i = tid; i < 8; i += kBlock) {
        const bool real = i < p.n_act;
        lds[L::AUX + i] = (real && n.act_scale) ? n.act_scale[i] : T(1);
        lds[L::AUX + 8 + i] = (real && p.low) ? p.low[i] : T(0);
        lds[L::AUX + 16 + i] = (real && p.high) ? p.high[i] : T(0);
    }
    __syncthreads();
}

template <typename T>
__device__ __forceinline__ T act_t(T v, int activation) {
    return activation == 0 ? atacom::num<T>::max(v, T(0)) : atacom::num<T>::tanh(v);
}

// Four lanes per row: lane lq of the quad owns the hidden units 4 m + lq, the quad exchanges a layer's outputs by shuffles and
// sums the output layer's partial dot products in a butterfly (the same bits in its four lanes).  `cat` (TD3) adds the columns
// n_obs .. n_obs + n_act - 1 of W1 against as; the observation is zero there.
template <typename T, int CH>
__device__ __forceinline__ void forward_valu(const T* __restrict__ lds, const T (&obs)[4 * CH], const T (&as)[NK], int n_obs,
                                             int n_act, bool cat, bool with_action, int activation, int lane, T (&out)[NK]) {
    using L = LdsV<CH>;
    using N = atacom::num<T>;
    constexpr int D = 4 * CH, U = H / 4;
    const int lq = lane & 3, base = lane & ~3;
    T x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = (obs[c] - lds[L::SHIFT + c]) * lds[L::SCALE + c];
    T h1[U], hf[H], h2[U];
#pragma unroll
    for (int m = 0; m < U; ++m) {
        const T* w = lds + L::W1 + (4 * m + lq) * L::S1;
        T acc = lds[L::B1 + 4 * m + lq];
#pragma unroll
        for (int c = 0; c < D; ++c) acc = N::fma(w[c], x[c], acc);
        if (cat) {
#pragma unroll
            for (int k = 0; k < NK; ++k)
                if (k < n_act) acc = N::fma(w[n_obs + k], as[k], acc);
        }
        h1[m] = act_t(acc, activation);
    }
#pragma unroll
    for (int m = 0; m < U; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) hf[4 * m + q] = __shfl(h1[m], base + q);
#pragma unroll
    for (int m = 0; m < U; ++m) {
        const T* w = lds + L::W2 + (4 * m + lq) * L::S2;
        T acc = lds[L::B2 + 4 * m + lq];
#pragma unroll
        for (int i = 0; i < H; ++i) acc = N::fma(w[i], hf[i], acc);
        if (with_action) {
            const T* wa = lds + L::W2A + (4 * m + lq) * 8;
#pragma unroll
            for (int k = 0; k < NK; ++k) acc = N::fma(wa[k], as[k], acc);
        }
        h2[m] = act_t(acc, activation);
    }
#pragma unroll
    for (int o = 0; o < NK; ++o) {
        T part = T(0);
#pragma unroll
        for (int m = 0; m < U; ++m) part = N::fma(lds[L::W3T + (4 * m + lq) * L::S3 + o], h2[m], part);
        part += __shfl_xor(part, 1);
        part += __shfl_xor(part, 2);
        out[o] = lds[L::B3 + o] + part;
    }
}

// a'' of a row from the actor's output m: aux = [act_scale | low | high] in LDS
template <typename T>
__device__ __forceinline__ void form_action(const Params<T>& p, const T* aux, int mean_mode, const T (&m)[NK], const T (&e)[NK],
                                            T (&a)[NK]) {
    using N = atacom::num<T>;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        T v = T(0);
        if (k < p.n_act) {
            v = mean_mode ? aux[k] * N::tanh(m[k]) : m[k];
            if (p.eps) v = v + N::min(N::max(p.noise_std * e[k], -p.noise_clip), p.noise_clip);
            if (p.low) v = N::min(N::max(v, aux[8 + k]), aux[16 + k]);
        }
        a[k] = v;
    }
}

// float: two wavefronts per SIMD, i.e. at most 256 registers; double takes what it needs
template <typename T> constexpr int kWavesPerSimd = std::is_same<T, float>::value ? 2 : 1;

template <typename T, int CH>
__global__ __launch_bounds__(kBlock, kWavesPerSimd<T>) void k_offpolicy_net(const Params<T> p) {
    constexpr int D = 4 * CH;
    constexpr bool f32 = std::is_same<T, float>::value;
    constexpr int kRows = f32 ? kRowsF32 : kRowsF64;
    using LM = LdsM<CH>;
    using LV = LdsV<CH>;
    constexpr int kStage = 64 * 32;
    constexpr int kLds = f32 ? LM::NET + kExtra + kWaves * kStage : LV::ALL;
    constexpr int kAux = f32 ? (int)LM::AUX : (int)LV::AUX;
    __shared__ __attribute__((aligned(32))) T lds[kLds];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool owner = f32 || (lane & 3) == 0;
    const int64_t n_tiles = (p.n_rows + kRows - 1) / kRows, step = (int64_t)gridDim.x * kWaves, last = p.n_rows - 1;
    const int64_t rounds = (n_tiles + step - 1) / step;
    for (int64_t round = 0; round < rounds; ++round) {
        const int64_t tile = round * step + (int64_t)blockIdx.x * kWaves + wave;
        const int64_t r = tile * kRows + (f32 ? lane : lane >> 2);
        const int64_t rc = r < last ? r : last;
        const int64_t row = p.idx ? p.idx[rc] : rc;
        T a[NK];
        {
            const T* ar = row_ptr(p.action, row, p.n_inner);          // not dereferenced with an actor
#pragma unroll
            for (int k = 0; k < NK; ++k) a[k] = (!p.has_actor && k < p.n_act) ? ar[k] : T(0);
        }
        T q = T(0);
        for (int n = 0; n < p.n_nets; ++n) {
            // (selected field by field, not indexed: a run-time index into the kernel's argument block would put it in scratch)
            Net<T> net;
#define OFFPOLICY_PICK(f) net.f = n == 0 ? p.net[0].f : n == 1 ? p.net[1].f : p.net[2].f
            OFFPOLICY_PICK(W1); OFFPOLICY_PICK(b1); OFFPOLICY_PICK(W2); OFFPOLICY_PICK(b2); OFFPOLICY_PICK(W2a); OFFPOLICY_PICK(W3);
            OFFPOLICY_PICK(b3); OFFPOLICY_PICK(shift); OFFPOLICY_PICK(scale); OFFPOLICY_PICK(act_scale); OFFPOLICY_PICK(n1);
            OFFPOLICY_PICK(n_out); OFFPOLICY_PICK(activation); OFFPOLICY_PICK(mean_mode);
#undef OFFPOLICY_PICK
            const bool actor = p.has_actor && n == 0, cat = !actor && p.kind == ATACOM_OFFPOLICY_TD3;
            if (p.n_nets > 1 || round == 0) {
                if constexpr (f32) stage_mfma<CH>(p, net, lds, threadIdx.x);
                else stage_valu<T, CH>(p, net, lds, threadIdx.x);
            }
            // the row is read again in every phase (it is in the cache by the second): 4 CH registers less across the networks
            T obs[D], as[NK], out[NK];
            const T* xr = row_ptr(p.obs, row, p.n_inner);
#pragma unroll
            for (int c = 0; c < D; ++c) obs[c] = c < p.n_obs ? xr[c] : T(0);
#pragma unroll
            for (int k = 0; k < NK; ++k) as[k] = (!actor && k < p.n_act) ? a[k] / lds[kAux + k] : T(0);
            if constexpr (f32) {
                float* stage = lds + LM::NET + kExtra + wave * kStage;
                const int ka = actor ? 0 : (p.n_act + 3) / 4;
                float xin[4][CH], aop[4][2];
                rows_to_operands<CH>(lds, stage, obs, as, p.n_obs, p.n_act, cat, ka, lane, xin, aop);
                forward_mfma<CH>(lds, stage, xin, aop, ka, net.activation, lane, out);
            } else {
                forward_valu<T, CH>(lds, obs, as, p.n_obs, p.n_act, cat, !actor, net.activation, lane, out);
            }
            if (actor) {
                T e[NK];
                const T* er = p.eps + rc * p.eps_stride;              // not dereferenced without eps
#pragma unroll
                for (int k = 0; k < NK; ++k) e[k] = (p.eps && k < p.n_act) ? er[k] : T(0);
                form_action<T>(p, lds + kAux, net.mean_mode, out, e, a);
                if (p.aout && owner && r <= last) {
                    T* ao = p.aout + r * p.aout_stride;
#pragma unroll
                    for (int k = 0; k < NK; ++k)
                        if (k < p.n_act) ao[k] = a[k];
                }
            } else {
                q = (n == p.has_actor) ? out[0] : atacom::num<T>::min(q, out[0]);
            }
        }
        T y = q;
        if (p.has_actor) {
            const T rew = *row_ptr(p.reward, row, p.n_inner), ab = *row_ptr(p.absorbing, row, p.n_inner);
            const T keep = ab > T(0.5) ? T(0) : T(1);
            const T t0 = keep * q;
            const T t1 = p.gamma * t0;
            y = rew + t1;
        }
        if (owner && r <= last) p.y[r * p.y_stride] = y;
    }
}

// One workgroup per pair walks its tensors; three individually rounded operations per value (-ffp-contract=off).
struct SoftPair {
    void* t[ATACOM_OFFPOLICY_TENSORS];
    const void* o[ATACOM_OFFPOLICY_TENSORS];
    int n[ATACOM_OFFPOLICY_TENSORS];
};

struct SoftLaunch {
    SoftPair pair[ATACOM_OFFPOLICY_MAX_PAIRS];
    double tau;
};

template <typename T>
__global__ __launch_bounds__(kSoftBlock) void k_soft_update(const SoftLaunch L) {
    const SoftPair& P = L.pair[blockIdx.x];
    const T a = (T)L.tau, b = (T)(1.0 - L.tau);
#pragma unroll
    for (int s = 0; s < ATACOM_OFFPOLICY_TENSORS; ++s) {
        T* t = (T*)P.t[s];
        const T* o = (const T*)P.o[s];
        const int n = P.n[s];
        for (int i = threadIdx.x; i < n; i += kSoftBlock) {
            const T x = a * o[i];
            const T z = b * t[i];
            t[i] = x + z;
        }
    }
}

namespace {

template <typename T>
Net<T> net_of(const NetDesc& d) {
    return Net<T>{(const T*)d.W1, (const T*)d.b1, (const T*)d.W2, (const T*)d.b2, (const T*)d.W2a, (const T*)d.W3, (const T*)d.b3,
                  (const T*)d.shift, (const T*)d.scale, (const T*)d.act_scale, d.n1, d.n_out, d.activation, d.mean_mode};
}

template <typename T>
Rows<T> rows_of(const atacom_evaluate_view& v) {
    return Rows<T>{(const T*)v.ptr, v.stride_outer, v.stride_inner};
}

template <typename T>
int launch(const Call& c, int blocks, hipStream_t s) {
    Params<T> p{};
    for (int n = 0; n < c.n_nets; ++n) p.net[n] = net_of<T>(c.net[n]);
    p.has_actor = c.has_actor; p.n_nets = c.n_nets; p.kind = c.kind; p.n_obs = c.n_obs; p.n_act = c.n_act;
    p.n_rows = c.n_rows; p.n_inner = c.n_inner; p.idx = c.idx;
    p.obs = rows_of<T>(c.obs); p.action = rows_of<T>(c.action); p.reward = rows_of<T>(c.reward); p.absorbing = rows_of<T>(c.absorbing);
    p.eps = (const T*)c.eps; p.eps_stride = c.eps_stride; p.low = (const T*)c.low; p.high = (const T*)c.high;
    p.noise_std = (T)c.noise_std; p.noise_clip = (T)c.noise_clip; p.gamma = (T)c.gamma;
    p.y = (T*)c.y; p.y_stride = c.y_stride; p.aout = (T*)c.action_out; p.aout_stride = c.action_out_stride;
    const int n1 = c.net[c.has_actor].n1;               // the critic's first layer: the widest of the call
#define OFFPOLICY_GO(CH) \
    case CH: hipLaunchKernelGGL((k_offpolicy_net<T, CH>), dim3(blocks), dim3(kBlock), 0, s, p); break
    switch ((n1 + 3) / 4) {
        OFFPOLICY_GO(1); OFFPOLICY_GO(2); OFFPOLICY_GO(3); OFFPOLICY_GO(4);
        OFFPOLICY_GO(5); OFFPOLICY_GO(6); OFFPOLICY_GO(7); OFFPOLICY_GO(8);
        default: return ATACOM_OFFPOLICY_E_UNSUPPORTED;
    }
#undef OFFPOLICY_GO
    return ATACOM_OFFPOLICY_OK;
}

}  // namespace

int net_launch(const Call& c, int blocks, hipStream_t s) {
    if (c.dtype == ATACOM_OFFPOLICY_F32) return launch<float>(c, blocks, s);
    if (c.dtype == ATACOM_OFFPOLICY_F64) return launch<double>(c, blocks, s);
    return ATACOM_OFFPOLICY_E_UNSUPPORTED;
}

void soft_update_launch(const atacom_offpolicy_soft_update_args& a, hipStream_t s) {
    SoftLaunch L = {};
    L.tau = a.tau;
    for (int k = 0; k < a.n_pairs; ++k) {
        pair_sizes(a.pairs[k], L.pair[k].n);
        for (int i = 0; i < ATACOM_OFFPOLICY_TENSORS; ++i) {
            L.pair[k].t[i] = a.pairs[k].target[i];
            L.pair[k].o[i] = a.pairs[k].online[i];
        }
    }
    if (a.dtype == ATACOM_OFFPOLICY_F64)
        hipLaunchKernelGGL(k_soft_update<double>, dim3(a.n_pairs), dim3(kSoftBlock), 0, s, L);
    else
        hipLaunchKernelGGL(k_soft_update<float>, dim3(a.n_pairs), dim3(kSoftBlock), 0, s, L);
}

}  // namespace atacom_offpolicy
