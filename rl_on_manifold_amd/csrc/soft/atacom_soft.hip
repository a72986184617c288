// Kernels of libatacom_soft.so (include/atacom_soft_hip.h states the arithmetic): k_soft_target<T, CH>, the fused soft TD target
// (mu, sigma, critic 1, critic 2 as phases of a workgroup); k_soft_critic<T, CH>, the forward and the backward pass of one or
// two critics; k_soft_actor<T, CH>, the gradients of the squashed-Gaussian actor's loss -- the four forward phases, the critics'
// input gradient, then the workgroup's own network (mu or sigma: the grid's second dimension) forward again and backward;
// k_soft_reduce<T>, which adds the workgroups' partial sums in a fixed order; and k_soft_alpha<T>, Adam on log_alpha.
//
// Borrowed from ../atacom_policy.h, which this unit includes and does not edit: the LDS layout MlpLdsM, the operand mapping of
// mlp_forward_mfma, mlp_act16, mlp_act, wave_lds_fence and num<T>.  From ../mlp/atacom_mlp_backward.h (namespace
// atacom_mlp_backward, shared with the fit, trust and offgrad units), which states the float32 mappings: the row access, layer 1,
// the transposition buffers, the backward pass from dy on, the accumulators with their hand-over and store, the float64
// backward loops, column pairs and accumulation, the slice sum of the reduction and the CH switch.  From
// ../mlp/atacom_mlp_forward.h (the same namespace, shared with the offgrad unit), without its WA branch: the block's layout LdsM
// with AUX, the staging of a network's weights (stage_weights), obs_elem, the float64 layers (normalise_f64, hidden_f64,
// head_f64), pick_fields and the launchers' RowView / rows_of.  This unit's own: its Net and the AUX words, forward_block, the
// critics' first-layer input [xn | a], the row arithmetic, and the critics' input gradient, which comes out like the deltas,
// element 4 g + v of row n16 in register v.
// LDS: one network block MlpLdsM<4 CH, 64, 8>::NET (act_scale and act_shift in its last 40 floats), 8 floats, and 8 KB of
// staging per wavefront: 63808 bytes, ONE network resident at a time.  Between the phases a row's values travel in the
// registers of the lane that owns it (lane l of a wavefront owns row l of its tile).
//
// The walk of the critic kernel is per wavefront; the walks of the target and actor kernels are uniform per workgroup, because
// they restage behind barriers.  Loads are not predicated per lane: a lane past the end reads the last row again, its dy is
// zero and its stores are guarded.  No atomics, plain vector stores.
// Compiled with -ffp-contract=off (build.UNIT_FLAGS): the row arithmetic is the individually rounded one the header writes;
// the fused multiply-adds of the float64 kernels are explicit.
#include "atacom_soft.h"
#include "../atacom_policy.h"

namespace atacom_soft {

constexpr int kExtra = 8;         // floats after the network block, unused: the block and the staging keep their offsets
constexpr int kOutA = 0, kOutB = 512, kOutQ = 1024;     // between the phases: [64][8], [64][8] and [64] per wavefront

template <typename T>
struct Net {
    const T *W1, *b1, *W2, *b2, *W3, *b3, *shift, *scale;
    int n1, n_out, activation;
};

// what the row arithmetic of a call needs besides the networks
template <typename T>
struct Squash {
    const T *eps, *act_scale, *act_shift, *log_alpha;
    int64_t eps_stride;
    T lmin, lmax;
};

template <typename T>
struct Head {
    int n_obs, n_act;
    int64_t n_rows, n_inner;
    const int64_t* idx;
    Rows<T> obs;
};

template <typename T>
struct TargetParams : Head<T> {
    Net<T> mu, sigma, critic[2];
    Squash<T> sq;
    Rows<T> reward, absorbing;
    T gamma;
    T *y, *aout, *lpout;
    int64_t y_stride, aout_stride, lpout_stride;
};

template <typename T>
struct CriticParams : Head<T> {
    Net<T> net[2];
    Rows<T> action;
    const T* target;
    int64_t target_stride;
    T* workspace;
};

template <typename T>
struct ActorParams : Head<T> {
    Net<T> mu, sigma, critic[2];
    Squash<T> sq;
    T target_entropy;
    T *aout, *lpout, *qout, *dqout;
    int64_t aout_stride, lpout_stride, qout_stride, dqout_stride;
    T* workspace;
};

// --------------------------------------------------------------------------------------------------- the row arithmetic
// What a row keeps of the header's lines: a, t, w, e = w + 1e-6, p = s eps, the clamp gate and logp.
template <typename T>
struct Sampled {
    T a[NK], t[NK], w[NK], e[NK], p[NK], logp;
    bool open[NK], clamped;
};

// m, lr: the outputs of Mu and Sig; er: the row's eps; sc, sh: act_scale and act_shift.  Elements at or past k: zeros.
template <typename T>
__device__ __forceinline__ void sample_row(const T (&m)[NK], const T (&lr)[NK], const T (&er)[NK], const T (&sc)[NK], const T (&sh)[NK], int k,
                                           T lmin, T lmax, Sampled<T>& o) {
    T G = T(0), C = T(0);
    o.clamped = false;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
        o.a[i] = o.t[i] = o.w[i] = o.p[i] = T(0);
        o.e[i] = T(1);
        o.open[i] = false;
        if (i < k) {
            T l = lr[i] < lmin ? lmin : lr[i];
            l = l > lmax ? lmax : l;
            o.open[i] = lmin < lr[i] && lr[i] < lmax;
            o.clamped = o.clamped || !o.open[i];
            const T s = atacom::num<T>::exp(l);
            o.p[i] = s * er[i];
            const T u = m[i] + o.p[i];
            o.t[i] = atacom::num<T>::tanh(u);
            T a = sc[i] * o.t[i];
            o.a[i] = a + sh[i];
            o.w[i] = atacom::num<T>::fma(-o.t[i], o.t[i], T(1));
            o.e[i] = o.w[i] + T(1e-6);
            const T c = atacom::num<T>::log(o.e[i]);
            T g = (T(-0.5) * er[i]) * er[i];
            g = g - l;
            g = g - T(0.91893853320467274178);
            G = i == 0 ? g : G + g;
            C = i == 0 ? c : C + c;
        }
    }
    o.logp = G - C;
}

// du, then dm = du and dl of the header, from dq/da of the selected critic
template <typename T>
__device__ __forceinline__ void actor_row(const Sampled<T>& s, const T (&dq)[NK], const T (&sc)[NK], int k, T alpha, T (&dm)[NK], T (&dl)[NK]) {
#pragma unroll
    for (int i = 0; i < NK; ++i) {
        dm[i] = dl[i] = T(0);
        if (i < k) {
            T r = (T(2) * s.t[i]) * s.w[i];
            r = r / s.e[i];
            const T du = alpha * r - dq[i] * (sc[i] * s.w[i]);
            dm[i] = du;
            const T v = du * s.p[i] - alpha;
            dl[i] = s.open[i] ? v : T(0);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ float32
// AUX of the block: act_scale [8], act_shift [8]
template <typename T>
__device__ __forceinline__ void pick_net(Net<T>& n, bool second, const Net<T>& a, const Net<T>& b) {
    using N = Net<T>;
    pick_fields(n, second, a, b, &N::W1, &N::b1, &N::W2, &N::b2, &N::W3, &N::b3, &N::shift, &N::scale, &N::n1, &N::n_out, &N::activation);
}

// The actor kernels select mu | sigma with the assignments written out: through pick_fields the same selection leaves all
// sixteen of them other code than they were, k_soft_actor<double>, which fills the register file and spills, 168 bytes longer
// (profiles/offpolicy_forward_shared.md).  The critic kernels are unchanged through pick_net.
#define SOFT_PICK_OWN(dst, second, A, B)                                                                                          \
    dst.W1 = second ? B.W1 : A.W1; dst.b1 = second ? B.b1 : A.b1; dst.W2 = second ? B.W2 : A.W2; dst.b2 = second ? B.b2 : A.b2;     \
    dst.W3 = second ? B.W3 : A.W3; dst.b3 = second ? B.b3 : A.b3; dst.shift = second ? B.shift : A.shift;                         \
    dst.scale = second ? B.scale : A.scale; dst.n1 = second ? B.n1 : A.n1; dst.n_out = second ? B.n_out : A.n_out;                 \
    dst.activation = second ? B.activation : A.activation

// the header's stage_weights (all 16 rows of the W3 block) and this unit's AUX words, between the two barriers of a phase
template <int CH>
__device__ __forceinline__ void stage_net(const Net<float>& n, int n_obs, const float* act_scale, const float* act_shift, int n_act, float* lds,
                                          int tid) {
    using L = LdsM<CH>;
    __syncthreads();                                   // the phase before has read its weights
    stage_weights<CH, false>(n, n_obs, n_act, lds, tid);
    for (int i = tid; i < 8; i += kBlock) {
        lds[L::AUX + i] = (i < n_act && act_scale) ? act_scale[i] : 1.0f;
        lds[L::AUX + 8 + i] = (i < n_act && act_shift) ? act_shift[i] : 0.0f;
    }
    __syncthreads();
}

// element e of a critic's first-layer input [xn | a], the action's row at ar (memory or LDS); 0 at or past n_obs + n_act
template <int CH>
__device__ __forceinline__ float x1_elem(const float* lds, const float* xr, const float* ar, int e, int n_obs, int n_act) {
    const int k = e - n_obs;
    const int kc = k < 0 ? 0 : (k < n_act ? k : n_act - 1);
    const float x = obs_elem<CH>(lds, xr, e, n_obs), a = ar[kc];
    return e < n_obs ? x : (k < n_act ? a : 0.0f);
}

// The forward pass of one block of 16 rows, keeping what the backward pass needs.  xin[s] = element CH g + s of the input of
// row n16.  h1, h2: the activations; o: register v = output 4 g + v of row n16 (real for 4 g + v < n_out).
template <int CH>
__device__ __forceinline__ void forward_block(const float* __restrict__ net, const float (&xin)[CH], int activation, int n16, int g,
                                              V4 (&h1)[4], V4 (&h2)[4], V4& o) {
    using L = LdsM<CH>;
    const V4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    layer1<CH>(net, xin, h1, n16, g);
    atacom::mlp_act16(h1, activation);
    // ---- layer 2: K-step (t, v) carries unit 16 t + 4 g + v, i.e. register v of h1[t]
#pragma unroll
    for (int u = 0; u < 4; ++u) h2[u] = *reinterpret_cast<const V4*>(net + L::B2 + 16 * u + 4 * g);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        V4 w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = *reinterpret_cast<const V4*>(net + L::W2 + (16 * u + n16) * L::S2 + 16 * t + 4 * g);
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int u = 0; u < 4; ++u) h2[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u][v], h1[t][v], h2[u], 0, 0, 0);
    }
    atacom::mlp_act16(h2, activation);
    // ---- output layer: rows >= n_out of W3 are zero
    V4 oa = *reinterpret_cast<const V4*>(net + L::B3 + 4 * g), ob = zero;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const V4 w = *reinterpret_cast<const V4*>(net + L::W3 + n16 * L::S2 + 16 * t + 4 * g);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            if ((t & 1) == 0) oa = __builtin_amdgcn_mfma_f32_16x16x4f32(w[v], h2[t][v], oa, 0, 0, 0);
            else ob = __builtin_amdgcn_mfma_f32_16x16x4f32(w[v], h2[t][v], ob, 0, 0, 0);
        }
    }
    o = oa + ob;
}

template <int CH>
__device__ __forceinline__ void critic_f32(const CriticParams<float>& p) {
    constexpr int NT = 4 * CH > 16 ? 2 : 1;
    using L = LdsM<CH>;
    constexpr int kLds = L::NET + kExtra + kWaves * kStage;
    __shared__ __attribute__((aligned(16))) float lds[kLds];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n16 = lane & 15, g = lane >> 4;
    Net<float> net;
    pick_net(net, blockIdx.y != 0, p.net[0], p.net[1]);
    stage_net<CH>(net, p.n_obs, nullptr, nullptr, p.n_act, lds, threadIdx.x);
    float* t_act = lds + L::NET + kExtra + wave * kStage;      // activations [16][64]
    float* t_del = t_act + 1024;                                // deltas [16][64]; before them: q [16][8], dy [16][8]

    Grads<NT> acc;
    acc.zero();
    float db3 = 0.0f, st = 0.0f;
    const int64_t n_tiles = (p.n_rows + kRowsF32 - 1) / kRowsF32, last = p.n_rows - 1;
    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wave; tile < n_tiles; tile += (int64_t)gridDim.x * kWaves) {
#pragma unroll 1
        for (int blk = 0; blk < kRowsF32 / 16; ++blk) {
            const int64_t r0 = tile * kRowsF32 + 16 * blk;
            if (r0 >= p.n_rows) break;                           // uniform: the whole block is past the end
            const int64_t r = r0 + n16;
            const bool live = r <= last;
            const int64_t fr = flat_row(p, r);
            const float* xr = row_ptr(p.obs, fr, p.n_inner);
            const float* ar = row_ptr(p.action, fr, p.n_inner);
            float xin[CH], xb[4][NT];
#pragma unroll
            for (int s = 0; s < CH; ++s) xin[s] = x1_elem<CH>(lds, xr, ar, CH * g + s, p.n_obs, p.n_act);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int64_t fs = flat_row(p, r0 + 4 * s + g);
                const float* xs = row_ptr(p.obs, fs, p.n_inner);
                const float* as = row_ptr(p.action, fs, p.n_inner);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) xb[s][nt] = x1_elem<CH>(lds, xs, as, 16 * nt + n16, p.n_obs, p.n_act);
            }
            V4 h1[4], h2[4], o;
            forward_block<CH>(lds, xin, net.activation, n16, g, h1, h2, o);
            // ---- q of the row to its four lanes; each of them forms the row's head (identically)
            if (g == 0) t_del[n16 * 8] = o[0];
            atacom::wave_lds_fence();
            const float q = t_del[n16 * 8];
            const float d = q - p.target[(r < last ? r : last) * p.target_stride];
            const float dy = live ? 2.0f * d : 0.0f;
            db3 += dy;
            st += live ? d * d : 0.0f;
            *reinterpret_cast<V4*>(t_del + 128 + n16 * 8) = V4{dy, 0.0f, 0.0f, 0.0f};
            *reinterpret_cast<V4*>(t_del + 128 + n16 * 8 + 4) = V4{0.0f, 0.0f, 0.0f, 0.0f};
            backward<CH, NT>(lds, t_act, t_del, h1, h2, xb, net.activation, n16, g, acc);
        }
    }
    sum_biases(acc);
    db3 = sum16(db3);
    st = sum16(st);
    static_assert((Grads<NT>::kSlots + 2) * 64 <= kLds, "the hand-over fits the workgroup's LDS");
    hand_over(acc, lds, wave, lane, [&](auto&& f, int q) {
        db3 = f(q++, db3);
        st = f(q++, st);
    });
    if (wave != 0) return;
    const int64_t Q = partial_size(net.n1, 1);
    float* out = p.workspace + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * Q;
    store_net(acc, out, net.n1, 1, n16, g);
    if (lane == 0) {
        const NetOffsets o = net_offsets(net.n1, 1);
        out[o.b3] = db3;
        out[o.end] = st;
        out[o.end + 1] = out[o.end + 2] = out[o.end + 3] = 0.0f;
    }
}

// One forward phase of a policy network over the wavefront's tile: its outputs -> dst [64][8] of the staging area.
template <int CH, typename P>
__device__ __forceinline__ void policy_phase(const P& p, const float* lds, float* dst, int64_t base, int activation, int n16, int g) {
#pragma unroll 1
    for (int blk = 0; blk < 4; ++blk) {
        const int64_t r0 = base + 16 * blk;
        if (r0 >= p.n_rows) break;
        const float* xr = row_ptr(p.obs, flat_row(p, r0 + n16), p.n_inner);
        float xin[CH];
#pragma unroll
        for (int s = 0; s < CH; ++s) xin[s] = obs_elem<CH>(lds, xr, CH * g + s, p.n_obs);
        V4 h1[4], h2[4], o;
        forward_block<CH>(lds, xin, activation, n16, g, h1, h2, o);
        if (g < 2) *reinterpret_cast<V4*>(dst + (16 * blk + n16) * 8 + 4 * g) = o;
    }
}

__device__ __forceinline__ void read8(const float* src, float (&v)[NK]) {
    const V4 a = *reinterpret_cast<const V4*>(src), b = *reinterpret_cast<const V4*>(src + 4);
#pragma unroll
    for (int k = 0; k < NK; ++k) v[k] = k < 4 ? a[k & 3] : b[k & 3];
}

// The phases mu and sigma and the row arithmetic of the lane's own row `ro`; afterwards the staged network is sigma and the
// rows' actions lie in the staging area, [64][8] at kOutA.
template <int CH, typename P>
__device__ __forceinline__ void sample_phase(const P& p, float* lds, float* stage, int64_t base, int lane, int n16, int g, float (&sc)[NK],
                                             Sampled<float>& s) {
    using L = LdsM<CH>;
    const int64_t last = p.n_rows - 1, ro = base + lane, rc = ro < last ? ro : last;
    float m[NK], lr[NK], er[NK], sh[NK];
    stage_net<CH>(p.mu, p.n_obs, p.sq.act_scale, p.sq.act_shift, p.n_act, lds, threadIdx.x);
    policy_phase<CH>(p, lds, stage + kOutA, base, p.mu.activation, n16, g);
    stage_net<CH>(p.sigma, p.n_obs, p.sq.act_scale, p.sq.act_shift, p.n_act, lds, threadIdx.x);
    policy_phase<CH>(p, lds, stage + kOutB, base, p.sigma.activation, n16, g);
    atacom::wave_lds_fence();
    read8(stage + kOutA + lane * 8, m);
    read8(stage + kOutB + lane * 8, lr);
    const float* ep = p.sq.eps + rc * p.sq.eps_stride;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        er[k] = ep[k < p.n_act ? k : p.n_act - 1];
        sc[k] = lds[L::AUX + k];
        sh[k] = lds[L::AUX + 8 + k];
    }
    sample_row<float>(m, lr, er, sc, sh, p.n_act, p.sq.lmin, p.sq.lmax, s);
    atacom::wave_lds_fence();
    *reinterpret_cast<V4*>(stage + kOutA + lane * 8) = V4{s.a[0], s.a[1], s.a[2], s.a[3]};
    *reinterpret_cast<V4*>(stage + kOutA + lane * 8 + 4) = V4{s.a[4], s.a[5], s.a[6], s.a[7]};
    atacom::wave_lds_fence();
}

// One critic over the wavefront's tile on [xn | a] with a from the staging area: q -> [64] at kOutQ and, with GRAD, the input
// gradient dq/da -> [64][8] at kOutB.
template <int CH, bool GRAD, typename P>
__device__ __forceinline__ void critic_phase(const P& p, const float* lds, float* stage, int64_t base, int activation, int n16, int g) {
    using L = LdsM<CH>;
    const V4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int blk = 0; blk < 4; ++blk) {
        const int64_t r0 = base + 16 * blk;
        if (r0 >= p.n_rows) break;
        const float* xr = row_ptr(p.obs, flat_row(p, r0 + n16), p.n_inner);
        const float* ar = stage + kOutA + (16 * blk + n16) * 8;
        float xin[CH];
#pragma unroll
        for (int s = 0; s < CH; ++s) xin[s] = x1_elem<CH>(lds, xr, ar, CH * g + s, p.n_obs, p.n_act);
        V4 h1[4], h2[4], o;
        forward_block<CH>(lds, xin, activation, n16, g, h1, h2, o);
        if (g == 0) stage[kOutQ + 16 * blk + n16] = o[0];
        if constexpr (GRAD) {
            // delta2 = W3^T * act'(h2) from dq = 1; delta1 = (W2^T delta2) * act'(h1)
            V4 d2[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) d2[u] = *reinterpret_cast<const V4*>(lds + L::W3 + 16 * u + 4 * g);
            times_act_prime(d2, h2, activation);
            V4 d1[4] = {zero, zero, zero, zero};
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float* wrow = lds + L::W2 + (16 * u + 4 * g + v) * L::S2 + n16;
#pragma unroll
                    for (int t = 0; t < 4; ++t) d1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wrow[16 * t], d2[u][v], d1[t], 0, 0, 0);
                }
            times_act_prime(d1, h1, activation);
            // dq/da[k] = sum_j W1[j][D + k] delta1[j]: M = k (n16 < 8), N = row n16, K-step (t, v) = unit 16 t + 4 g + v
            const int kk = (n16 & 7) < p.n_act ? (n16 & 7) : p.n_act - 1, e = p.n_obs + kk;   // the rows k >= n_act are not used
            const int slot = (e / CH) * 8 + e % CH;
            V4 gq = zero;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    gq = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[L::W1 + (16 * t + 4 * g + v) * L::S1 + slot], d1[t][v], gq, 0, 0, 0);
            if (g < 2) *reinterpret_cast<V4*>(stage + kOutB + (16 * blk + n16) * 8 + 4 * g) = gq;
        }
    }
    atacom::wave_lds_fence();
}

template <int CH>
__device__ __forceinline__ void target_f32(const TargetParams<float>& p) {
    using L = LdsM<CH>;
    constexpr int kLds = L::NET + kExtra + kWaves * kStage;
    __shared__ __attribute__((aligned(16))) float lds[kLds];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n16 = lane & 15, g = lane >> 4;
    float* stage = lds + L::NET + kExtra + wave * kStage;
    const float alpha = atacom::num<float>::exp(p.sq.log_alpha[0]);
    const int64_t n_tiles = (p.n_rows + kRowsF32 - 1) / kRowsF32, step = (int64_t)gridDim.x * kWaves, last = p.n_rows - 1;
    const int64_t rounds = (n_tiles + step - 1) / step;         // uniform per workgroup: every wavefront reaches every barrier
    for (int64_t round = 0; round < rounds; ++round) {
        const int64_t base = (round * step + (int64_t)blockIdx.x * kWaves + wave) * kRowsF32;
        const int64_t ro = base + lane;
        const bool live = ro <= last;
        float sc[NK];
        Sampled<float> s;
        sample_phase<CH>(p, lds, stage, base, lane, n16, g, sc, s);
        if (live) {
            if (p.aout) {
#pragma unroll
                for (int k = 0; k < NK; ++k)
                    if (k < p.n_act) p.aout[ro * p.aout_stride + k] = s.a[k];
            }
            if (p.lpout) p.lpout[ro * p.lpout_stride] = s.logp;
        }
        stage_net<CH>(p.critic[0], p.n_obs, nullptr, nullptr, p.n_act, lds, threadIdx.x);
        critic_phase<CH, false>(p, lds, stage, base, p.critic[0].activation, n16, g);
        const float q1 = stage[kOutQ + lane];
        atacom::wave_lds_fence();
        stage_net<CH>(p.critic[1], p.n_obs, nullptr, nullptr, p.n_act, lds, threadIdx.x);
        critic_phase<CH, false>(p, lds, stage, base, p.critic[1].activation, n16, g);
        const float q2 = stage[kOutQ + lane];
        atacom::wave_lds_fence();
        const float q = q2 < q1 ? q2 : q1;
        float z = alpha * s.logp;
        z = q - z;
        const int64_t fr = flat_row(p, ro);
        const float rew = *row_ptr(p.reward, fr, p.n_inner), ab = *row_ptr(p.absorbing, fr, p.n_inner);
        const float keep = ab > 0.5f ? 0.0f : 1.0f;
        const float y = rew + p.gamma * (keep * z);
        if (live) p.y[ro * p.y_stride] = y;
    }
}

template <int CH>
__device__ __forceinline__ void actor_f32(const ActorParams<float>& p) {
    constexpr int NT = 4 * CH > 16 ? 2 : 1;
    using L = LdsM<CH>;
    constexpr int kLds = L::NET + kExtra + kWaves * kStage;
    __shared__ __attribute__((aligned(16))) float lds[kLds];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n16 = lane & 15, g = lane >> 4;
    float* stage = lds + L::NET + kExtra + wave * kStage;
    float* t_act = stage;                                       // the last phase: the transposition buffers
    float* t_del = stage + 1024;
    const bool second = blockIdx.y != 0;                        // this workgroup's network: mu | sigma
    Net<float> own;
    SOFT_PICK_OWN(own, second, p.mu, p.sigma);
    const float alpha = atacom::num<float>::exp(p.sq.log_alpha[0]);

    Grads<NT> acc;
    acc.zero();
    float db3[NK], st[kStats];
#pragma unroll
    for (int k = 0; k < NK; ++k) db3[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < kStats; ++k) st[k] = 0.0f;

    const int64_t n_tiles = (p.n_rows + kRowsF32 - 1) / kRowsF32, step = (int64_t)gridDim.x * kWaves, last = p.n_rows - 1;
    const int64_t rounds = (n_tiles + step - 1) / step;
    for (int64_t round = 0; round < rounds; ++round) {
        const int64_t base = (round * step + (int64_t)blockIdx.x * kWaves + wave) * kRowsF32;
        const int64_t ro = base + lane;
        const bool live = ro <= last, writes = live && !second;
        float sc[NK], dy[NK];
        {
            Sampled<float> s;
            sample_phase<CH>(p, lds, stage, base, lane, n16, g, sc, s);
            float q1, q2, g1[NK], g2[NK];
            stage_net<CH>(p.critic[0], p.n_obs, nullptr, nullptr, p.n_act, lds, threadIdx.x);
            critic_phase<CH, true>(p, lds, stage, base, p.critic[0].activation, n16, g);
            q1 = stage[kOutQ + lane];
            read8(stage + kOutB + lane * 8, g1);
            atacom::wave_lds_fence();
            stage_net<CH>(p.critic[1], p.n_obs, nullptr, nullptr, p.n_act, lds, threadIdx.x);
            critic_phase<CH, true>(p, lds, stage, base, p.critic[1].activation, n16, g);
            q2 = stage[kOutQ + lane];
            read8(stage + kOutB + lane * 8, g2);
            atacom::wave_lds_fence();
            const bool two = q2 < q1;
            const float q = two ? q2 : q1;
            float dq[NK], dm[NK], dl[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) dq[k] = two ? g2[k] : g1[k];
            actor_row<float>(s, dq, sc, p.n_act, alpha, dm, dl);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                dy[k] = live ? (second ? dl[k] : dm[k]) : 0.0f;
                db3[k] += dy[k];
            }
            const float term = alpha * s.logp - q;
            st[0] += live ? term : 0.0f;
            st[1] += live ? s.logp : 0.0f;
            st[2] += live ? -(s.logp + p.target_entropy) : 0.0f;
            st[3] += (live && s.clamped) ? 1.0f : 0.0f;
            if (writes) {
#pragma unroll
                for (int k = 0; k < NK; ++k)
                    if (k < p.n_act) {
                        if (p.aout) p.aout[ro * p.aout_stride + k] = s.a[k];
                        if (p.dqout) p.dqout[ro * p.dqout_stride + k] = dq[k];
                    }
                if (p.lpout) p.lpout[ro * p.lpout_stride] = s.logp;
                if (p.qout) { p.qout[ro * p.qout_stride] = q1; p.qout[ro * p.qout_stride + 1] = q2; }
            }
        }
        // ---- the last phase: this workgroup's network forward again (its activations are recomputed, not kept) and backward
        stage_net<CH>(own, p.n_obs, nullptr, nullptr, p.n_act, lds, threadIdx.x);
#pragma unroll 1
        for (int blk = 0; blk < 4; ++blk) {
            const int64_t r0 = base + 16 * blk;
            if (r0 >= p.n_rows) break;
            if (g == blk) {                                      // the owners of the block's rows: dy [16][8]
                *reinterpret_cast<V4*>(t_del + 128 + n16 * 8) = V4{dy[0], dy[1], dy[2], dy[3]};
                *reinterpret_cast<V4*>(t_del + 128 + n16 * 8 + 4) = V4{dy[4], dy[5], dy[6], dy[7]};
            }
            const float* xr = row_ptr(p.obs, flat_row(p, r0 + n16), p.n_inner);
            float xin[CH], xb[4][NT];
#pragma unroll
            for (int s = 0; s < CH; ++s) xin[s] = obs_elem<CH>(lds, xr, CH * g + s, p.n_obs);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float* xs = row_ptr(p.obs, flat_row(p, r0 + 4 * s + g), p.n_inner);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) xb[s][nt] = obs_elem<CH>(lds, xs, 16 * nt + n16, p.n_obs);
            }
            V4 h1[4], h2[4], o;
            forward_block<CH>(lds, xin, own.activation, n16, g, h1, h2, o);
            backward<CH, NT>(lds, t_act, t_del, h1, h2, xb, own.activation, n16, g, acc);
        }
    }
    sum_biases(acc);
#pragma unroll
    for (int k = 0; k < NK; ++k) db3[k] = sum64(db3[k]);
#pragma unroll
    for (int k = 0; k < kStats; ++k) st[k] = sum64(st[k]);
    static_assert((Grads<NT>::kSlots + NK + kStats) * 64 <= kLds, "the hand-over fits the workgroup's LDS");
    hand_over(acc, lds, wave, lane, [&](auto&& f, int q) {
#pragma unroll
        for (int k = 0; k < NK; ++k) db3[k] = f(q++, db3[k]);
#pragma unroll
        for (int k = 0; k < kStats; ++k) st[k] = f(q++, st[k]);
    });
    if (wave != 0) return;
    const int64_t Q = partial_size(p.n_obs, p.n_act);
    float* out = p.workspace + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * Q;
    store_net(acc, out, p.n_obs, p.n_act, n16, g);
    if (lane == 0) {
        const NetOffsets o = net_offsets(p.n_obs, p.n_act);
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (k < p.n_act) out[o.b3 + k] = db3[k];
#pragma unroll
        for (int k = 0; k < kStats; ++k) out[o.end + k] = st[k];
    }
}

// ------------------------------------------------------------------------------------------------------------ float64
// A workgroup takes 16 rows at a time, sixteen threads a row; the weights are read from memory, the rows' activations and
// deltas lie in LDS as one record per row, and every thread owns the entries tid, tid + 256, ... of the partial, each the sum
// over rows of the product of two columns of the records (the header's backward_f64, net_columns and accumulate_f64).
// columns of a record: the network whose gradient is taken (h1 | h2 | delta1 | delta2 | its first-layer input | dy), the
// statistics, 1 and 0; the target and actor kernels append the policy's outputs, the action and their critics' columns
struct Rec {
    static constexpr int H1 = 0, H2 = H1 + H, D1 = H2 + H, D2 = D1 + H, X = D2 + H, DY = X + 32, ST = DY + NK, ONE = ST + kStats,
                         ZERO = ONE + 1, SIZE = ZERO + 1;
};

struct RecActor : Rec {
    static constexpr int CH1 = Rec::SIZE, CH2 = CH1 + H, CX = CH2 + H, M = CX + 32, LR = M + NK, A = LR + NK, G1 = A + NK, G2 = G1 + NK,
                         SIZE = G2 + NK;
};

// the two columns whose product, summed over the rows, is entry e of the partial: the gradient's, then the statistics; past its
// end: 0 * 1
__device__ __forceinline__ void entry_columns(int e, int n_in, const NetOffsets& o, int& ca, int& cb) {
    ca = Rec::ZERO;
    cb = Rec::ONE;
    if (!net_columns<Rec>(e, n_in, o, ca, cb) && e < o.end + kStats) ca = Rec::ST + (e - o.end);
}

constexpr int kMaxQ = H * 32 + H + H * H + H + H * NK + NK + kStats, kNQ = (kMaxQ + kBlock - 1) / kBlock;

__device__ __forceinline__ void critic_f64(const CriticParams<double>& p) {
    constexpr int R = kRowsF64;
    using C = Rec;
    __shared__ double rec[R * C::SIZE];
    const int tid = threadIdx.x, row = tid >> 4, c = tid & 15;
    Net<double> net;
    pick_net(net, blockIdx.y != 0, p.net[0], p.net[1]);
    const int Q = (int)partial_size(net.n1, 1);
    const NetOffsets o = net_offsets(net.n1, 1);
    int ca[kNQ], cb[kNQ];
    double acc[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) {
        acc[q] = 0.0;
        entry_columns(tid + kBlock * q, net.n1, o, ca[q], cb[q]);
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
            const double* xr = row_ptr(p.obs, fr, p.n_inner);
            const double* ar = row_ptr(p.action, fr, p.n_inner);
            normalise_f64(net, xr, me + C::X, p.n_obs, c);
            if (c < NK) {
                if (c < p.n_act) me[C::X + p.n_obs + c] = ar[c];
                me[C::DY + c] = 0.0;
            }
            if (c < kStats) me[C::ST + c] = 0.0;
            if (c == 0) { me[C::ONE] = 1.0; me[C::ZERO] = 0.0; }
        }
        __syncthreads();
        hidden_f64(net, me, C::X, C::H1, C::H2, live, c);
        if (live && c == 0) {
            const double d = head_f64(net, me, C::H2, 0) - p.target[r * p.target_stride];
            me[C::DY] = 2.0 * d;
            me[C::ST] = d * d;
        }
        __syncthreads();
        backward_f64<C>(net, me, live, c);
        accumulate_f64<C>(rec, rows, ca, cb, acc);
    }
    store_f64(p.workspace + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * Q, Q, tid, acc);
}

// mu and sigma of the thread's row into the columns M and LR (the policy's normalised observation lies in X), then thread 0 of
// the row runs the row arithmetic and leaves the action in the columns A
template <typename P>
__device__ __forceinline__ void sample_f64(const P& p, double* me, int64_t r, bool live, int c, double (&sc)[NK], Sampled<double>& s) {
    using C = RecActor;
    hidden_f64(p.mu, me, C::X, C::H1, C::H2, live, c);
    if (live && c < p.n_act) me[C::M + c] = head_f64(p.mu, me, C::H2, c);
    __syncthreads();
    hidden_f64(p.sigma, me, C::X, C::H1, C::H2, live, c);
    if (live && c < p.n_act) me[C::LR + c] = head_f64(p.sigma, me, C::H2, c);
    __syncthreads();
    if (live && c == 0) {
        double m[NK], lr[NK], er[NK], sh[NK];
        for (int k = 0; k < NK; ++k) {
            const bool real = k < p.n_act;
            m[k] = real ? me[C::M + k] : 0.0;
            lr[k] = real ? me[C::LR + k] : 0.0;
            er[k] = real ? p.sq.eps[r * p.sq.eps_stride + k] : 0.0;
            sc[k] = (real && p.sq.act_scale) ? p.sq.act_scale[k] : 1.0;
            sh[k] = (real && p.sq.act_shift) ? p.sq.act_shift[k] : 0.0;
        }
        sample_row<double>(m, lr, er, sc, sh, p.n_act, p.sq.lmin, p.sq.lmax, s);
        for (int k = 0; k < NK; ++k) me[C::A + k] = s.a[k];
    }
    __syncthreads();
}

// critic n on [xn | a] of the thread's row -> its activations in CH1, CH2; q in thread 0 of the row
__device__ __forceinline__ double critic_q_f64(const Net<double>& n, double* me, const double* xr, int D, int k, bool live, int c) {
    using C = RecActor;
    if (live) {
        normalise_f64(n, xr, me + C::CX, D, c);
        if (c < k) me[C::CX + D + c] = me[C::A + c];
    }
    __syncthreads();
    hidden_f64(n, me, C::CX, C::CH1, C::CH2, live, c);
    double q = 0.0;
    if (live && c == 0) q = head_f64(n, me, C::CH2, 0);
    return q;
}

__device__ __forceinline__ void target_f64(const TargetParams<double>& p) {
    constexpr int R = kRowsF64;
    using C = RecActor;
    __shared__ double rec[R * C::SIZE];
    const int tid = threadIdx.x, row = tid >> 4, c = tid & 15;
    const double alpha = ::exp(p.sq.log_alpha[0]);
    const int64_t n_tiles = (p.n_rows + R - 1) / R;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * R + row;
        const bool live = r < p.n_rows;
        const int64_t fr = flat_row(p, r);
        double* me = rec + row * C::SIZE;
        const double* xr = row_ptr(p.obs, fr, p.n_inner);
        if (live) normalise_f64(p.mu, xr, me + C::X, p.n_obs, c);
        __syncthreads();
        double sc[NK];
        Sampled<double> s;
        sample_f64(p, me, r, live, c, sc, s);
        const double q1 = critic_q_f64(p.critic[0], me, xr, p.n_obs, p.n_act, live, c);
        __syncthreads();
        const double q2 = critic_q_f64(p.critic[1], me, xr, p.n_obs, p.n_act, live, c);
        if (live && c == 0) {
            const double q = q2 < q1 ? q2 : q1;
            double z = alpha * s.logp;
            z = q - z;
            const double keep = *row_ptr(p.absorbing, fr, p.n_inner) > 0.5 ? 0.0 : 1.0;
            p.y[r * p.y_stride] = *row_ptr(p.reward, fr, p.n_inner) + p.gamma * (keep * z);
            if (p.aout)
                for (int k = 0; k < p.n_act; ++k) p.aout[r * p.aout_stride + k] = s.a[k];
            if (p.lpout) p.lpout[r * p.lpout_stride] = s.logp;
        }
        __syncthreads();
    }
}

// dq/da of critic n from its activations in CH1, CH2 into the columns `dst`
__device__ __forceinline__ void critic_dqda_f64(const Net<double>& n, double* me, int D, int k, int dst, bool live, int c) {
    using C = RecActor;
    __syncthreads();
    if (live)                                                // delta2 over h2, in place
        for (int j = c; j < H; j += 16) me[C::CH2 + j] = n.W3[j] * act_prime(me[C::CH2 + j], n.activation);
    __syncthreads();
    if (live)                                                // delta1 over h1, in place: thread c owns its units
        for (int i = c; i < H; i += 16) {
            double a = 0.0;
            for (int j = 0; j < H; ++j) a = __builtin_fma(n.W2[j * H + i], me[C::CH2 + j], a);
            me[C::CH1 + i] = a * act_prime(me[C::CH1 + i], n.activation);
        }
    __syncthreads();
    if (live && c < k) {
        double gs = 0.0;
        for (int j = 0; j < H; ++j) gs = __builtin_fma(n.W1[j * n.n1 + D + c], me[C::CH1 + j], gs);
        me[dst + c] = gs;
    }
    __syncthreads();
}

__device__ __forceinline__ void actor_f64(const ActorParams<double>& p) {
    constexpr int R = kRowsF64;
    using C = RecActor;
    __shared__ double rec[R * C::SIZE];
    const int tid = threadIdx.x, row = tid >> 4, c = tid & 15;
    const bool second = blockIdx.y != 0;
    Net<double> own;
    SOFT_PICK_OWN(own, second, p.mu, p.sigma);
    const double alpha = ::exp(p.sq.log_alpha[0]);
    const int k = p.n_act, D = p.n_obs;
    const int Q = (int)partial_size(D, k);
    const NetOffsets o = net_offsets(D, k);
    int ca[kNQ], cb[kNQ];
    double acc[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) {
        acc[q] = 0.0;
        entry_columns(tid + kBlock * q, D, o, ca[q], cb[q]);
    }
    const int64_t n_tiles = (p.n_rows + R - 1) / R;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t r = tile * R + row;
        const bool live = r < p.n_rows;
        const int64_t left = p.n_rows - tile * R;
        const int rows = left < R ? (int)left : R;
        const int64_t fr = flat_row(p, r);
        double* me = rec + row * C::SIZE;
        const double* xr = row_ptr(p.obs, fr, p.n_inner);
        if (live) {
            normalise_f64(p.mu, xr, me + C::X, D, c);
            if (c == 0) { me[C::ONE] = 1.0; me[C::ZERO] = 0.0; }
        }
        __syncthreads();
        double sc[NK];
        Sampled<double> s;
        sample_f64(p, me, r, live, c, sc, s);
        const double q1 = critic_q_f64(p.critic[0], me, xr, D, k, live, c);
        critic_dqda_f64(p.critic[0], me, D, k, C::G1, live, c);
        const double q2 = critic_q_f64(p.critic[1], me, xr, D, k, live, c);
        critic_dqda_f64(p.critic[1], me, D, k, C::G2, live, c);
        if (live && c == 0) {
            const bool two = q2 < q1;
            const double q = two ? q2 : q1;
            double dq[NK], dm[NK], dl[NK];
            for (int i = 0; i < NK; ++i) dq[i] = i < k ? me[(two ? C::G2 : C::G1) + i] : 0.0;
            actor_row<double>(s, dq, sc, k, alpha, dm, dl);
            for (int i = 0; i < NK; ++i) me[C::DY + i] = second ? dl[i] : dm[i];
            me[C::ST] = alpha * s.logp - q;
            me[C::ST + 1] = s.logp;
            me[C::ST + 2] = -(s.logp + p.target_entropy);
            me[C::ST + 3] = s.clamped ? 1.0 : 0.0;
            if (!second) {
                for (int i = 0; i < k; ++i) {
                    if (p.aout) p.aout[r * p.aout_stride + i] = s.a[i];
                    if (p.dqout) p.dqout[r * p.dqout_stride + i] = dq[i];
                }
                if (p.lpout) p.lpout[r * p.lpout_stride] = s.logp;
                if (p.qout) { p.qout[r * p.qout_stride] = q1; p.qout[r * p.qout_stride + 1] = q2; }
            }
        }
        __syncthreads();
        hidden_f64(own, me, C::X, C::H1, C::H2, live, c);
        backward_f64<C>(own, me, live, c);
        accumulate_f64<C>(rec, rows, ca, cb, acc);
    }
    store_f64(p.workspace + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * Q, Q, tid, acc);
}

// one wavefront per SIMD: the float32 kernels keep up to 144 accumulator registers next to their operands
template <typename T, int CH>
__global__ __launch_bounds__(kBlock, 1) void k_soft_target(const TargetParams<T> p) {
    if constexpr (std::is_same<T, float>::value) target_f32<CH>(p);
    else target_f64(p);
}

template <typename T, int CH>
__global__ __launch_bounds__(kBlock, 1) void k_soft_critic(const CriticParams<T> p) {
    if constexpr (std::is_same<T, float>::value) critic_f32<CH>(p);
    else critic_f64(p);
}

template <typename T, int CH>
__global__ __launch_bounds__(kBlock, 1) void k_soft_actor(const ActorParams<T> p) {
    if constexpr (std::is_same<T, float>::value) actor_f32<CH>(p);
    else actor_f64(p);
}

// grad and stats of network blockIdx.y from its partials: a workgroup takes kReduceValues consecutive values, each summed in the
// fixed order of sum_partials and divided by the number of rows.  A network without `stats` (the actor call's sigma half) leaves them unwritten.
template <typename T>
struct ReduceParams {
    const T* ws;
    T* grad[2];
    T* stats[2];
    int blocks, q_size;
    T m;
};

template <typename T>
__global__ __launch_bounds__(kReduceBlock) void k_soft_reduce(const ReduceParams<T> p) {
    const int i = blockIdx.x * kReduceValues + threadIdx.x % kReduceValues;
    T s;
    if (!sum_partials(p.ws + (int64_t)blockIdx.y * p.blocks * p.q_size, p.blocks, p.q_size, p.q_size, i, s)) return;
    s = s / p.m;
    T* grad = blockIdx.y ? p.grad[1] : p.grad[0];
    T* stats = blockIdx.y ? p.stats[1] : p.stats[0];
    const int n_grad = p.q_size - kStats;
    if (i < n_grad) grad[i] = s;
    else if (stats) stats[i - n_grad] = s;
}

// Adam on the one value log_alpha (the header's lines); one thread
template <typename T>
struct AlphaParams {
    T* x;
    const T* grad;
    void* state;
    double lr, beta1, beta2;
    T omb1, b2, omb2, eps;
};

__device__ inline float sqrt_t(float x) { return sqrtf(x); }
__device__ inline double sqrt_t(double x) { return sqrt(x); }

template <typename T>
__global__ __launch_bounds__(64) void k_soft_alpha(const AlphaParams<T> p) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t* step = (int64_t*)p.state;
    double* pw = (double*)p.state + 1;
    T* mv = (T*)((char*)p.state + 32);
    const int64_t t = step[0] + 1;
    const double b1p = pw[0] * p.beta1, b2p = pw[1] * p.beta2;
    const T step_size = (T)(p.lr / (1.0 - b1p)), bc2s = (T)sqrt(1.0 - b2p);
    const T g = p.grad[0];
    const T m = mv[0] + (g - mv[0]) * p.omb1;
    const T v = p.b2 * mv[1] + (p.omb2 * g) * g;
    p.x[0] = p.x[0] - step_size * (m / (sqrt_t(v) / bc2s + p.eps));
    mv[0] = m;
    mv[1] = v;
    step[0] = t;
    pw[0] = b1p;
    pw[1] = b2p;
}

namespace {

template <typename T>
Net<T> net_of(const NetDesc& d) {
    return Net<T>{(const T*)d.W1, (const T*)d.b1, (const T*)d.W2, (const T*)d.b2, (const T*)d.W3, (const T*)d.b3,
                  (const T*)d.shift, (const T*)d.scale, d.n1, d.n_out, d.activation};
}

template <typename T, typename P>
void head_of(const RowCall& c, P& p) {
    p.n_obs = c.n_obs; p.n_act = c.n_act; p.n_rows = c.n_rows; p.n_inner = c.n_inner; p.idx = c.idx; p.obs = rows_of<T>(c.obs);
}

template <typename T>
void reduce(const void* ws, void* const (&grad)[2], void* const (&stats)[2], int n_nets, int blocks, int q, int64_t rows, hipStream_t s) {
    ReduceParams<T> r{(const T*)ws, {(T*)grad[0], (T*)grad[1]}, {(T*)stats[0], (T*)stats[1]}, blocks, q, (T)rows};
    hipLaunchKernelGGL((k_soft_reduce<T>), dim3((q + kReduceValues - 1) / kReduceValues, n_nets), dim3(kReduceBlock), 0, s, r);
}

template <typename T>
int launch_target(const TargetCall& c, int blocks, hipStream_t s) {
    TargetParams<T> p{};
    head_of<T>(c, p);
    p.mu = net_of<T>(c.mu); p.sigma = net_of<T>(c.sigma); p.critic[0] = net_of<T>(c.critic[0]); p.critic[1] = net_of<T>(c.critic[1]);
    p.sq = Squash<T>{(const T*)c.eps, (const T*)c.act_scale, (const T*)c.act_shift, (const T*)c.log_alpha, c.eps_stride,
                     (T)c.log_std_min, (T)c.log_std_max};
    p.reward = rows_of<T>(c.reward); p.absorbing = rows_of<T>(c.absorbing);
    p.gamma = (T)c.gamma;
    p.y = (T*)c.y; p.aout = (T*)c.action_out; p.lpout = (T*)c.logp_out;
    p.y_stride = c.y_stride; p.aout_stride = c.action_out_stride; p.lpout_stride = c.logp_out_stride;
    return with_ch(c.critic[0].n1, [&](auto ch) {   // the critics' first layer: the widest of the call
               hipLaunchKernelGGL((k_soft_target<T, decltype(ch)::value>), dim3(blocks), dim3(kBlock), 0, s, p);
           }) ? ATACOM_SOFT_OK : ATACOM_SOFT_E_UNSUPPORTED;
}

template <typename T>
int launch_critic(const CriticCall& c, int blocks, hipStream_t s) {
    CriticParams<T> p{};
    head_of<T>(c, p);
    for (int n = 0; n < c.n_nets; ++n) p.net[n] = net_of<T>(c.net[n]);
    if (c.n_nets == 1) p.net[1] = p.net[0];
    p.action = rows_of<T>(c.action);
    p.target = (const T*)c.target; p.target_stride = c.target_stride; p.workspace = (T*)c.workspace;
    const int n1 = c.net[0].n1;
    if (!with_ch(n1, [&](auto ch) {
            hipLaunchKernelGGL((k_soft_critic<T, decltype(ch)::value>), dim3(blocks, c.n_nets), dim3(kBlock), 0, s, p);
        }))
        return ATACOM_SOFT_E_UNSUPPORTED;
    reduce<T>(c.workspace, c.grad, c.stats, c.n_nets, blocks, (int)partial_size(n1, 1), c.n_rows, s);
    return ATACOM_SOFT_OK;
}

template <typename T>
int launch_actor(const ActorCall& c, int blocks, hipStream_t s) {
    ActorParams<T> p{};
    head_of<T>(c, p);
    p.mu = net_of<T>(c.mu); p.sigma = net_of<T>(c.sigma); p.critic[0] = net_of<T>(c.critic[0]); p.critic[1] = net_of<T>(c.critic[1]);
    p.sq = Squash<T>{(const T*)c.eps, (const T*)c.act_scale, (const T*)c.act_shift, (const T*)c.log_alpha, c.eps_stride,
                     (T)c.log_std_min, (T)c.log_std_max};
    p.target_entropy = (T)c.target_entropy;
    p.aout = (T*)c.action_out; p.lpout = (T*)c.logp_out; p.qout = (T*)c.q_out; p.dqout = (T*)c.dqda_out;
    p.aout_stride = c.action_out_stride; p.lpout_stride = c.logp_out_stride; p.qout_stride = c.q_out_stride;
    p.dqout_stride = c.dqda_out_stride;
    p.workspace = (T*)c.workspace;
    if (!with_ch(c.critic[0].n1, [&](auto ch) {
            hipLaunchKernelGGL((k_soft_actor<T, decltype(ch)::value>), dim3(blocks, 2), dim3(kBlock), 0, s, p);
        }))
        return ATACOM_SOFT_E_UNSUPPORTED;
    void* const grad[2] = {c.grad_mu, c.grad_sigma};
    void* const stats[2] = {c.stats, nullptr};
    reduce<T>(c.workspace, grad, stats, 2, blocks, (int)partial_size(c.n_obs, c.n_act), c.n_rows, s);
    return ATACOM_SOFT_OK;
}

template <typename T>
void launch_alpha(const AlphaCall& c, hipStream_t s) {
    AlphaParams<T> p{(T*)c.log_alpha, (const T*)c.grad, c.state, c.lr, c.beta1, c.beta2,
                     (T)(1.0 - c.beta1), (T)c.beta2, (T)(1.0 - c.beta2), (T)c.eps};
    hipLaunchKernelGGL((k_soft_alpha<T>), dim3(1), dim3(64), 0, s, p);
}

}  // namespace

int target_launch(const TargetCall& c, int blocks, hipStream_t s) {
    if (c.dtype == ATACOM_SOFT_F32) return launch_target<float>(c, blocks, s);
    if (c.dtype == ATACOM_SOFT_F64) return launch_target<double>(c, blocks, s);
    return ATACOM_SOFT_E_UNSUPPORTED;
}

int critic_launch(const CriticCall& c, int blocks, hipStream_t s) {
    if (c.dtype == ATACOM_SOFT_F32) return launch_critic<float>(c, blocks, s);
    if (c.dtype == ATACOM_SOFT_F64) return launch_critic<double>(c, blocks, s);
    return ATACOM_SOFT_E_UNSUPPORTED;
}

int actor_launch(const ActorCall& c, int blocks, hipStream_t s) {
    if (c.dtype == ATACOM_SOFT_F32) return launch_actor<float>(c, blocks, s);
    if (c.dtype == ATACOM_SOFT_F64) return launch_actor<double>(c, blocks, s);
    return ATACOM_SOFT_E_UNSUPPORTED;
}

int alpha_launch(const AlphaCall& c, hipStream_t s) {
    if (c.dtype == ATACOM_SOFT_F32) launch_alpha<float>(c, s);
    else if (c.dtype == ATACOM_SOFT_F64) launch_alpha<double>(c, s);
    else return ATACOM_SOFT_E_UNSUPPORTED;
    return ATACOM_SOFT_OK;
}

}  // namespace atacom_soft
