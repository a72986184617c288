// Kernels of libatacom_offgrad.so (include/atacom_offgrad_hip.h states the arithmetic): k_offgrad_critic<T, CH>, the forward and
// the backward pass of one or two two-branch critics over the rows of a minibatch; k_offgrad_actor<T, CH>, the deterministic
// policy gradient -- actor forward, critic forward and input gradient, actor forward again and backward, as phases of a
// workgroup; and k_offgrad_reduce<T>, which adds the workgroups' partial sums in a fixed order.
//
// Borrowed from ../atacom_policy.h, which this unit includes and does not edit: the LDS layout MlpLdsM, the operand mapping of
// mlp_forward_mfma, mlp_act16, mlp_act, wave_lds_fence and num<T>.  From ../mlp/atacom_mlp_backward.h (namespace
// atacom_mlp_backward, shared with the fit, trust and soft units), which states the float32 mappings: the row access,
// the transposition buffers, the backward pass from dy on, the accumulators with their hand-over and store, the float64
// backward loops, column pairs and accumulation, the slice sum of the reduction and the CH switch.  From
// ../mlp/atacom_mlp_forward.h (the same namespace, shared with the soft unit): the block's layout LdsM with W2A and AUX, the
// staging of a network's weights (stage_weights), obs_elem, the float64 layers (normalise_f64, hidden_f64, head_f64),
// pick_fields and the launchers' RowView / rows_of.  Layer 2 of the critic has two branches, so staging and gradient take the
// headers' WA flag (dW2a = sum delta2 as^T rides on dW2's A operands).  This unit's own: its Net and the AUX words,
// forward_block, the scaled action as and TD3's first-layer input [xn | as], and the critic's INPUT gradient, W2a^T delta2
// (+ W1[:, D:]^T delta1), which the actor call needs and no weight-gradient pass produces; it comes out like the deltas,
// element 4 g + v of row n16 in register v.
// LDS: one network block MlpLdsM<4 CH, 64, 8>::NET with W2a [64][8] in rows 8 .. 15 of its W3 block (whose outputs are never
// stored), 8 floats, and 8 KB of staging per wavefront: 63808 bytes.  The kernels are bound to one wavefront per SIMD.
//
// The walk of the critic kernel is per wavefront (no barrier between staging and hand-over); the walk of the actor kernel is
// uniform per workgroup, because it restages behind barriers.  Loads are not predicated per lane: a lane past the end reads the
// last row again, its dy is zero and its stores are guarded.  No atomics, plain vector stores.
// Compiled with -ffp-contract=off (build.UNIT_FLAGS): the row arithmetic is the individually rounded one the header writes;
// the fused multiply-adds of the float64 kernels are explicit.
#include "atacom_offgrad.h"
#include "../atacom_policy.h"

namespace atacom_offgrad {

constexpr int kExtra = 8;         // floats after the network block, unused: the block and the staging keep their offsets

template <typename T>
struct Net {
    const T *W1, *b1, *W2, *b2, *W2a, *W3, *b3, *shift, *scale, *act_scale;
    int n1, n_out, activation, mean_mode;
};

template <typename T>
struct CriticParams {
    Net<T> net[2];
    int kind, n_obs, n_act;
    int64_t n_rows, n_inner;
    const int64_t* idx;
    Rows<T> obs, action;
    const T* target;
    int64_t target_stride;
    T* workspace;
};

template <typename T>
struct ActorParams {
    Net<T> actor, critic;
    int kind, n_obs, n_act;
    int64_t n_rows, n_inner;
    const int64_t* idx;
    Rows<T> obs;
    T *aout, *dqout;
    int64_t aout_stride, dqout_stride;
    T* workspace;
};

// ------------------------------------------------------------------------------------------------------------ float32
// AUX of the block: act_scale [8]
template <typename T>
__device__ __forceinline__ void pick_net(Net<T>& n, bool second, const Net<T>& a, const Net<T>& b) {
    using N = Net<T>;
    pick_fields(n, second, a, b, &N::W1, &N::b1, &N::W2, &N::b2, &N::W2a, &N::W3, &N::b3, &N::shift, &N::scale, &N::act_scale, &N::n1,
                &N::n_out, &N::activation, &N::mean_mode);
}

// the header's stage_weights (W2a: all zero for the actor) and this unit's AUX words, between the two barriers of a phase
template <int CH>
__device__ __forceinline__ void stage_net(const Net<float>& n, int n_obs, int n_act, float* lds, int tid) {
    using L = LdsM<CH>;
    __syncthreads();                                   // the phase before has read its weights
    stage_weights<CH, true>(n, n_obs, n_act, lds, tid);
    for (int i = tid; i < 8; i += kBlock) lds[L::AUX + i] = (i < n_act && n.act_scale) ? n.act_scale[i] : 1.0f;
    __syncthreads();
}

// element k of as = a / act_scale of the row at ar; 0 outside 0 .. n_act - 1
template <int CH>
__device__ __forceinline__ float as_elem(const float* lds, const float* ar, int k, int n_act) {
    using L = LdsM<CH>;
    const int kc = k < 0 ? 0 : (k < n_act ? k : n_act - 1);
    const float v = ar[kc] / lds[L::AUX + kc];
    return (k >= 0 && k < n_act) ? v : 0.0f;
}

// element e of the critic's first-layer input x1 = xn (DDPG) | [xn | as] (TD3, `cat`)
template <int CH>
__device__ __forceinline__ float x1_elem(const float* lds, const float* xr, const float* ar, int e, int n_obs, int n_act, bool cat) {
    const float x = obs_elem<CH>(lds, xr, e, n_obs), a = as_elem<CH>(lds, ar, cat ? e - n_obs : -1, n_act);
    return e < n_obs ? x : a;
}

// The forward pass of one block of 16 rows, keeping what the backward pass needs.  xin[s] = element CH g + s of the input of
// row n16; aop[j] = as[4 j + g] of row n16, the B operand of the `ka` action steps of layer 2 (0 for the actor).  h1, h2: the
// activations; o: register v = output 4 g + v of row n16 (real for 4 g + v < n_out).
template <int CH>
__device__ __forceinline__ void forward_block(const float* __restrict__ net, const float (&xin)[CH], const float (&aop)[2], int ka,
                                              int activation, int n16, int g, V4 (&h1)[4], V4 (&h2)[4], V4& o) {
    using L = LdsM<CH>;
    const V4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    // layer 1 is the header's layer1 followed by mlp_act16, written out: called as a function it leaves the same instructions
    // in another schedule, and k_offgrad_actor<float, 6> measured 1.7 % slower (profiles/offpolicy_backward_shared.md); as it
    // stands the float32 actor kernels are the code they were before the backward pass was shared, byte for byte
    float w1[4][8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        h1[t] = *reinterpret_cast<const V4*>(net + L::B1 + 16 * t + 4 * g);
        const float* row = net + L::W1 + (16 * t + n16) * L::S1 + 8 * g;
        const V4 lo = *reinterpret_cast<const V4*>(row), hi = *reinterpret_cast<const V4*>(row + 4);
#pragma unroll
        for (int s = 0; s < 4; ++s) { w1[t][s] = lo[s]; w1[t][4 + s] = hi[s]; }
    }
#pragma unroll
    for (int s = 0; s < CH; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t) h1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[t][s], xin[s], h1[t], 0, 0, 0);
    atacom::mlp_act16(h1, activation);
    // ---- layer 2: K-step (t, v) carries unit 16 t + 4 g + v, i.e. register v of h1[t]; then the action steps
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
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j < ka) {                                   // wave-uniform
#pragma unroll
            for (int u = 0; u < 4; ++u)
                h2[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(net[L::W2A + (16 * u + n16) * 8 + 4 * j + g], aop[j], h2[u], 0, 0, 0);
        }
    }
    atacom::mlp_act16(h2, activation);
    // ---- output layer: rows >= n_out of W3 are zero, rows 8 .. 15 hold W2a and their outputs are not used
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
    stage_net<CH>(net, p.n_obs, p.n_act, lds, threadIdx.x);
    float* t_act = lds + L::NET + kExtra + wave * kStage;      // activations [16][64]
    float* t_del = t_act + 1024;                                // deltas [16][64]; before them: q [16][8], dy [16][8]
    const bool cat = p.kind == ATACOM_OFFGRAD_TD3;
    const int ka = (p.n_act + 3) / 4;

    Grads<NT, true> acc;
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
            float xin[CH], aop[2], xb[4][NT], asb[4];
#pragma unroll
            for (int s = 0; s < CH; ++s) xin[s] = x1_elem<CH>(lds, xr, ar, CH * g + s, p.n_obs, p.n_act, cat);
#pragma unroll
            for (int j = 0; j < 2; ++j) aop[j] = as_elem<CH>(lds, ar, 4 * j + g, p.n_act);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int64_t fs = flat_row(p, r0 + 4 * s + g);
                const float* xs = row_ptr(p.obs, fs, p.n_inner);
                const float* as = row_ptr(p.action, fs, p.n_inner);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) xb[s][nt] = x1_elem<CH>(lds, xs, as, 16 * nt + n16, p.n_obs, p.n_act, cat);
                asb[s] = as_elem<CH>(lds, as, n16, p.n_act);
            }
            V4 h1[4], h2[4], o;
            forward_block<CH>(lds, xin, aop, ka, net.activation, n16, g, h1, h2, o);
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
            backward<CH, NT, true>(lds, t_act, t_del, h1, h2, xb, asb, net.activation, n16, g, acc);
        }
    }
    sum_biases(acc);
    db3 = sum16(db3);
    st = sum16(st);
    static_assert((Grads<NT, true>::kSlots + 2) * 64 <= kLds, "the hand-over fits the workgroup's LDS");
    hand_over(acc, lds, wave, lane, [&](auto&& f, int q) {
        db3 = f(q++, db3);
        st = f(q++, st);
    });
    if (wave != 0) return;
    const int64_t Q = partial_size(net.n1, 1, p.n_act);
    float* out = p.workspace + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * Q;
    store_net(acc, out, net.n1, 1, n16, g, p.n_act);
    if (lane == 0) {
        out[net_offsets(net.n1, 1).b3] = db3;
        float* stats = out + (Q - kStats);
        stats[0] = st;
        stats[1] = stats[2] = stats[3] = 0.0f;
    }
}

template <int CH>
__device__ __forceinline__ void actor_f32(const ActorParams<float>& p) {
    constexpr int NT = 4 * CH > 16 ? 2 : 1;
    using L = LdsM<CH>;
    constexpr int kLds = L::NET + kExtra + kWaves * kStage;
    __shared__ __attribute__((aligned(16))) float lds[kLds];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n16 = lane & 15, g = lane >> 4;
    float* stage = lds + L::NET + kExtra + wave * kStage;      // phases A, B: [64][8] outputs / as, then [64][8] dq/das
    float* t_act = stage;                                       // phase C: the transposition buffers
    float* t_del = stage + 1024;
    const bool cat = p.kind == ATACOM_OFFGRAD_TD3;
    const int ka = (p.n_act + 3) / 4;
    const V4 zero = {0.0f, 0.0f, 0.0f, 0.0f};

    Grads<NT> acc;
    acc.zero();
    float db3[NK], st = 0.0f;
#pragma unroll
    for (int k = 0; k < NK; ++k) db3[k] = 0.0f;
    const float noa[2] = {0.0f, 0.0f};

    const int64_t n_tiles = (p.n_rows + kRowsF32 - 1) / kRowsF32, step = (int64_t)gridDim.x * kWaves, last = p.n_rows - 1;
    const int64_t rounds = (n_tiles + step - 1) / step;         // uniform per workgroup: every wavefront reaches every barrier
    stage_net<CH>(p.actor, p.n_obs, p.n_act, lds, threadIdx.x);
    for (int64_t round = 0; round < rounds; ++round) {
        const int64_t base = (round * step + (int64_t)blockIdx.x * kWaves + wave) * kRowsF32;
        const int64_t ro = base + lane;                          // the row this lane owns between the phases
        const bool live_o = ro <= last;
        // ---- phase A: the actor's outputs m of the tile -> [64][8], then a and d a / d m at the owners
#pragma unroll 1
        for (int blk = 0; blk < 4; ++blk) {
            const int64_t r0 = base + 16 * blk;
            if (r0 >= p.n_rows) break;
            const float* xr = row_ptr(p.obs, flat_row(p, r0 + n16), p.n_inner);
            float xin[CH];
#pragma unroll
            for (int s = 0; s < CH; ++s) xin[s] = obs_elem<CH>(lds, xr, CH * g + s, p.n_obs);
            V4 h1[4], h2[4], o;
            forward_block<CH>(lds, xin, noa, 0, p.actor.activation, n16, g, h1, h2, o);
            if (g < 2) *reinterpret_cast<V4*>(stage + (16 * blk + n16) * 8 + 4 * g) = o;
        }
        atacom::wave_lds_fence();
        float a[NK], gm[NK];
        {
            const V4 m0 = *reinterpret_cast<const V4*>(stage + lane * 8), m1 = *reinterpret_cast<const V4*>(stage + lane * 8 + 4);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const float m = k < 4 ? m0[k & 3] : m1[k & 3];
                a[k] = 0.0f;
                gm[k] = 0.0f;
                if (k < p.n_act && live_o) {
                    if (p.actor.mean_mode) {
                        const float s = lds[L::AUX + k], t = atacom::num<float>::tanh(m);
                        a[k] = s * t;
                        gm[k] = s * __builtin_fmaf(-t, t, 1.0f);
                    } else {
                        a[k] = m;
                        gm[k] = 1.0f;
                    }
                }
            }
        }
        atacom::wave_lds_fence();
        if (p.aout && live_o) {
            float* ao = p.aout + ro * p.aout_stride;
#pragma unroll
            for (int k = 0; k < NK; ++k)
                if (k < p.n_act) ao[k] = a[k];
        }
        // ---- phase B: the critic on (obs, a) and its input gradient -> [64][8] behind the rows' as
        stage_net<CH>(p.critic, p.n_obs, p.n_act, lds, threadIdx.x);
        {
            float as[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) as[k] = k < p.n_act ? a[k] / lds[L::AUX + k] : 0.0f;
            *reinterpret_cast<V4*>(stage + lane * 8) = V4{as[0], as[1], as[2], as[3]};
            *reinterpret_cast<V4*>(stage + lane * 8 + 4) = V4{as[4], as[5], as[6], as[7]};
        }
        atacom::wave_lds_fence();
#pragma unroll 1
        for (int blk = 0; blk < 4; ++blk) {
            const int64_t r0 = base + 16 * blk;
            if (r0 >= p.n_rows) break;
            const bool live = r0 + n16 <= last;
            const float* xr = row_ptr(p.obs, flat_row(p, r0 + n16), p.n_inner);
            const float* asr = stage + (16 * blk + n16) * 8;
            float xin[CH], aop[2];
#pragma unroll
            for (int s = 0; s < CH; ++s) {
                const int e = CH * g + s, k = e - p.n_obs;
                const float x = obs_elem<CH>(lds, xr, e, p.n_obs), av = asr[k < 0 ? 0 : (k < NK ? k : NK - 1)];
                xin[s] = e < p.n_obs ? x : ((cat && k < p.n_act) ? av : 0.0f);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) aop[j] = asr[4 * j + g];
            V4 h1[4], h2[4], o;
            forward_block<CH>(lds, xin, aop, ka, p.critic.activation, n16, g, h1, h2, o);
            st += (live && g == 0) ? -o[0] : 0.0f;
            // delta2 = W3^T * act'(h2) from dq = 1
            V4 d2[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) d2[u] = *reinterpret_cast<const V4*>(lds + L::W3 + 16 * u + 4 * g);
            times_act_prime(d2, h2, p.critic.activation);
            // dq/das[k] = sum_j W2a[j][k] delta2[j]: M = k (n16 < 8), N = row n16, K-step (u, v) = unit 16 u + 4 g + v
            V4 gq = zero;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    gq = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[L::W2A + (16 * u + 4 * g + v) * 8 + (n16 & 7)], d2[u][v], gq, 0, 0, 0);
            if (cat) {                                           // wave-uniform: + sum_j W1[j][D + k] delta1[j]
                V4 d1[4] = {zero, zero, zero, zero};
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const float* wrow = lds + L::W2 + (16 * u + 4 * g + v) * L::S2 + n16;
#pragma unroll
                        for (int t = 0; t < 4; ++t) d1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wrow[16 * t], d2[u][v], d1[t], 0, 0, 0);
                    }
                times_act_prime(d1, h1, p.critic.activation);
                const int kk = (n16 & 7) < p.n_act ? (n16 & 7) : p.n_act - 1, e = p.n_obs + kk;   // the rows k >= n_act are not stored
                const int slot = (e / CH) * 8 + e % CH;
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        gq = __builtin_amdgcn_mfma_f32_16x16x4f32(lds[L::W1 + (16 * t + 4 * g + v) * L::S1 + slot], d1[t][v], gq, 0, 0, 0);
            }
            if (g < 2) *reinterpret_cast<V4*>(stage + 512 + (16 * blk + n16) * 8 + 4 * g) = gq;
        }
        atacom::wave_lds_fence();
        float dm[NK];
        {
            const V4 g0 = *reinterpret_cast<const V4*>(stage + 512 + lane * 8), g1 = *reinterpret_cast<const V4*>(stage + 512 + lane * 8 + 4);
            float dq[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const float gs = k < 4 ? g0[k & 3] : g1[k & 3];
                dq[k] = (k < p.n_act && live_o) ? gs / lds[L::AUX + k] : 0.0f;
                dm[k] = (k < p.n_act && live_o) ? -(dq[k] * gm[k]) : 0.0f;
                db3[k] += dm[k];
            }
            if (p.dqout && live_o) {
                float* dqo = p.dqout + ro * p.dqout_stride;
#pragma unroll
                for (int k = 0; k < NK; ++k)
                    if (k < p.n_act) dqo[k] = dq[k];
            }
        }
        atacom::wave_lds_fence();
        // ---- phase C: the actor again, forward (its activations are recomputed, not kept) and backward from dm
        stage_net<CH>(p.actor, p.n_obs, p.n_act, lds, threadIdx.x);
#pragma unroll 1
        for (int blk = 0; blk < 4; ++blk) {
            const int64_t r0 = base + 16 * blk;
            if (r0 >= p.n_rows) break;
            if (g == blk) {                                      // the owners of the block's rows: dy [16][8]
                *reinterpret_cast<V4*>(t_del + 128 + n16 * 8) = V4{dm[0], dm[1], dm[2], dm[3]};
                *reinterpret_cast<V4*>(t_del + 128 + n16 * 8 + 4) = V4{dm[4], dm[5], dm[6], dm[7]};
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
            forward_block<CH>(lds, xin, noa, 0, p.actor.activation, n16, g, h1, h2, o);
            backward<CH, NT>(lds, t_act, t_del, h1, h2, xb, p.actor.activation, n16, g, acc);
        }
    }
    sum_biases(acc);
#pragma unroll
    for (int k = 0; k < NK; ++k) db3[k] = sum64(db3[k]);
    st = sum16(st);
    static_assert((Grads<NT>::kSlots + NK + 1) * 64 <= kLds, "the hand-over fits the workgroup's LDS");
    hand_over(acc, lds, wave, lane, [&](auto&& f, int q) {
#pragma unroll
        for (int k = 0; k < NK; ++k) db3[k] = f(q++, db3[k]);
        st = f(q++, st);
    });
    if (wave != 0) return;
    const int64_t Q = partial_size(p.n_obs, p.n_act, 0);
    float* out = p.workspace + (int64_t)blockIdx.x * Q;
    store_net(acc, out, p.n_obs, p.n_act, n16, g);
    if (lane == 0) {
        const NetOffsets o = net_offsets(p.n_obs, p.n_act);
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (k < p.n_act) out[o.b3 + k] = db3[k];
        out[o.end] = st;
        out[o.end + 1] = out[o.end + 2] = out[o.end + 3] = 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------------------ float64
// A workgroup takes 16 rows at a time, sixteen threads a row; the weights are read from memory, the rows' activations and
// deltas lie in LDS as one record per row, and every thread owns the entries tid, tid + 256, ... of the partial, each the sum
// over rows of the product of two columns of the records (the header's backward_f64, net_columns and accumulate_f64).
// columns of a record: the network whose gradient is taken (h1 | h2 | delta1 | delta2 | its first-layer input | as | dy), the
// statistic, 1 and 0; the actor kernel appends its critic's columns
struct Rec {
    static constexpr int H1 = 0, H2 = H1 + H, D1 = H2 + H, D2 = D1 + H, X = D2 + H, AS = X + 32, DY = AS + NK, ST = DY + NK,
                         ONE = ST + 1, ZERO = ONE + 1, SIZE = ZERO + 1;
};

struct RecActor : Rec {
    static constexpr int CH1 = Rec::SIZE, CH2 = CH1 + H, CX = CH2 + H, GM = CX + 32, SIZE = GM + NK;
};

// the two columns whose product, summed over the rows, is entry e of the partial: the gradient's, then the statistic; past its
// end: 0 * 1
__device__ __forceinline__ void entry_columns(int e, int n_in, int n_act, const NetOffsets& o, int& ca, int& cb) {
    ca = Rec::ZERO;
    cb = Rec::ONE;
    if (!net_columns<Rec>(e, n_in, n_act, o, ca, cb) && e == o.end + H * n_act) ca = Rec::ST;
}

constexpr int kMaxQ = H * 32 + H + H * H + H + H * NK + NK + H * NK + kStats, kNQ = (kMaxQ + kBlock - 1) / kBlock;

__device__ __forceinline__ void critic_f64(const CriticParams<double>& p) {
    constexpr int R = kRowsF64;
    using C = Rec;
    __shared__ double rec[R * C::SIZE];
    const int tid = threadIdx.x, row = tid >> 4, c = tid & 15;
    Net<double> net;
    pick_net(net, blockIdx.y != 0, p.net[0], p.net[1]);
    const bool cat = p.kind == ATACOM_OFFGRAD_TD3;
    const int Q = (int)partial_size(net.n1, 1, p.n_act);
    const NetOffsets o = net_offsets(net.n1, 1);
    int ca[kNQ], cb[kNQ];
    double acc[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) {
        acc[q] = 0.0;
        entry_columns(tid + kBlock * q, net.n1, p.n_act, o, ca[q], cb[q]);
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
                const double as = c < p.n_act ? ar[c] / (net.act_scale ? net.act_scale[c] : 1.0) : 0.0;
                me[C::AS + c] = as;
                if (cat && c < p.n_act) me[C::X + p.n_obs + c] = as;
                me[C::DY + c] = 0.0;
            }
            if (c == 0) { me[C::ONE] = 1.0; me[C::ZERO] = 0.0; }
        }
        __syncthreads();
        hidden_f64<true>(net, me, C::X, C::H1, C::H2, p.n_act, C::AS, live, c);
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

__device__ __forceinline__ void actor_f64(const ActorParams<double>& p) {
    constexpr int R = kRowsF64;
    using C = RecActor;
    __shared__ double rec[R * C::SIZE];
    const int tid = threadIdx.x, row = tid >> 4, c = tid & 15;
    const Net<double>& A = p.actor;
    const Net<double>& Qn = p.critic;
    const bool cat = p.kind == ATACOM_OFFGRAD_TD3;
    const int k = p.n_act, D = p.n_obs;
    const int Q = (int)partial_size(D, k, 0);
    const NetOffsets o = net_offsets(D, k);
    int ca[kNQ], cb[kNQ];
    double acc[kNQ];
#pragma unroll
    for (int q = 0; q < kNQ; ++q) {
        acc[q] = 0.0;
        entry_columns(tid + kBlock * q, D, 0, o, ca[q], cb[q]);
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
            for (int e = c; e < D; e += 16) {                    // the header's normalise_f64 for both networks, the row read once
                me[C::X + e] = (xr[e] - (A.shift ? A.shift[e] : 0.0)) * (A.scale ? A.scale[e] : 1.0);
                me[C::CX + e] = (xr[e] - (Qn.shift ? Qn.shift[e] : 0.0)) * (Qn.scale ? Qn.scale[e] : 1.0);
            }
            if (c == 0) { me[C::ONE] = 1.0; me[C::ZERO] = 0.0; }
        }
        __syncthreads();
        hidden_f64<true>(A, me, C::X, C::H1, C::H2, 0, C::AS, live, c);
        if (live && c < NK) {
            double a = 0.0, gm = 0.0;
            if (c < k) {
                double m = A.b3[c];                              // head_f64, in place: as the call it moves an instruction of this kernel
                for (int j = 0; j < H; ++j) m = __builtin_fma(A.W3[c * H + j], me[C::H2 + j], m);
                if (A.mean_mode) {
                    const double s = A.act_scale ? A.act_scale[c] : 1.0, t = ::tanh(m);
                    a = s * t;
                    gm = s * __builtin_fma(-t, t, 1.0);
                } else {
                    a = m;
                    gm = 1.0;
                }
                if (p.aout) p.aout[r * p.aout_stride + c] = a;
            }
            const double as = c < k ? a / (Qn.act_scale ? Qn.act_scale[c] : 1.0) : 0.0;
            me[C::AS + c] = as;
            me[C::GM + c] = gm;
            if (cat && c < k) me[C::CX + D + c] = as;
        }
        __syncthreads();
        hidden_f64<true>(Qn, me, C::CX, C::CH1, C::CH2, k, C::AS, live, c);
        if (live && c == 0) me[C::ST] = -head_f64(Qn, me, C::CH2, 0);
        __syncthreads();
        if (live)                                                // delta2 of the critic over its h2, in place
            for (int j = c; j < H; j += 16) me[C::CH2 + j] = Qn.W3[j] * act_prime(me[C::CH2 + j], Qn.activation);
        __syncthreads();
        if (live && cat)                                         // delta1 over h1, in place: thread c owns its units
            for (int i = c; i < H; i += 16) {
                double a = 0.0;
                for (int j = 0; j < H; ++j) a = __builtin_fma(Qn.W2[j * H + i], me[C::CH2 + j], a);
                me[C::CH1 + i] = a * act_prime(me[C::CH1 + i], Qn.activation);
            }
        __syncthreads();
        if (live && c < NK) {
            double dm = 0.0;
            if (c < k) {
                double gs = 0.0;
                for (int j = 0; j < H; ++j) gs = __builtin_fma(Qn.W2a[j * k + c], me[C::CH2 + j], gs);
                if (cat)
                    for (int j = 0; j < H; ++j) gs = __builtin_fma(Qn.W1[j * Qn.n1 + D + c], me[C::CH1 + j], gs);
                const double dq = gs / (Qn.act_scale ? Qn.act_scale[c] : 1.0);
                if (p.dqout) p.dqout[r * p.dqout_stride + c] = dq;
                dm = -(dq * me[C::GM + c]);
            }
            me[C::DY + c] = dm;
        }
        __syncthreads();
        backward_f64<C>(A, me, live, c);
        accumulate_f64<C>(rec, rows, ca, cb, acc);
    }
    store_f64(p.workspace + (int64_t)blockIdx.x * Q, Q, tid, acc);
}

// one wavefront per SIMD: the float32 kernels keep up to 160 accumulator registers next to their operands
template <typename T, int CH>
__global__ __launch_bounds__(kBlock, 1) void k_offgrad_critic(const CriticParams<T> p) {
    if constexpr (std::is_same<T, float>::value) critic_f32<CH>(p);
    else critic_f64(p);
}

template <typename T, int CH>
__global__ __launch_bounds__(kBlock, 1) void k_offgrad_actor(const ActorParams<T> p) {
    if constexpr (std::is_same<T, float>::value) actor_f32<CH>(p);
    else actor_f64(p);
}

// grad and stats of network blockIdx.y from its partials: a workgroup takes kReduceValues consecutive values, each summed in the
// fixed order of sum_partials and divided by the number of rows
template <typename T>
struct ReduceParams {
    const T* ws;
    T* grad[2];
    T* stats[2];
    int blocks, q_size;
    T m;
};

template <typename T>
__global__ __launch_bounds__(kReduceBlock) void k_offgrad_reduce(const ReduceParams<T> p) {
    const int i = blockIdx.x * kReduceValues + threadIdx.x % kReduceValues;
    T s;
    if (!sum_partials(p.ws + (int64_t)blockIdx.y * p.blocks * p.q_size, p.blocks, p.q_size, p.q_size, i, s)) return;
    s = s / p.m;
    T* grad = blockIdx.y ? p.grad[1] : p.grad[0];
    T* stats = blockIdx.y ? p.stats[1] : p.stats[0];
    const int n_grad = p.q_size - kStats;
    if (i < n_grad) grad[i] = s;
    else stats[i - n_grad] = s;
}

namespace {

template <typename T>
Net<T> net_of(const NetDesc& d) {
    return Net<T>{(const T*)d.W1, (const T*)d.b1, (const T*)d.W2, (const T*)d.b2, (const T*)d.W2a, (const T*)d.W3, (const T*)d.b3,
                  (const T*)d.shift, (const T*)d.scale, (const T*)d.act_scale, d.n1, d.n_out, d.activation, d.mean_mode};
}

template <typename T>
void reduce(const void* ws, void* const (&grad)[2], void* const (&stats)[2], int n_nets, int blocks, int q, int64_t rows, hipStream_t s) {
    ReduceParams<T> r{(const T*)ws, {(T*)grad[0], (T*)grad[1]}, {(T*)stats[0], (T*)stats[1]}, blocks, q, (T)rows};
    hipLaunchKernelGGL((k_offgrad_reduce<T>), dim3((q + kReduceValues - 1) / kReduceValues, n_nets), dim3(kReduceBlock), 0, s, r);
}

template <typename T>
int launch_critic(const CriticCall& c, int blocks, hipStream_t s) {
    CriticParams<T> p{};
    for (int n = 0; n < c.n_nets; ++n) p.net[n] = net_of<T>(c.net[n]);
    if (c.n_nets == 1) p.net[1] = p.net[0];
    p.kind = c.kind; p.n_obs = c.n_obs; p.n_act = c.n_act; p.n_rows = c.n_rows; p.n_inner = c.n_inner; p.idx = c.idx;
    p.obs = rows_of<T>(c.obs); p.action = rows_of<T>(c.action);
    p.target = (const T*)c.target; p.target_stride = c.target_stride; p.workspace = (T*)c.workspace;
    const int n1 = c.net[0].n1;
    if (!with_ch(n1, [&](auto ch) {
            hipLaunchKernelGGL((k_offgrad_critic<T, decltype(ch)::value>), dim3(blocks, c.n_nets), dim3(kBlock), 0, s, p);
        }))
        return ATACOM_OFFGRAD_E_UNSUPPORTED;
    reduce<T>(c.workspace, c.grad, c.stats, c.n_nets, blocks, (int)partial_size(n1, 1, c.n_act), c.n_rows, s);
    return ATACOM_OFFGRAD_OK;
}

template <typename T>
int launch_actor(const ActorCall& c, int blocks, hipStream_t s) {
    ActorParams<T> p{};
    p.actor = net_of<T>(c.actor); p.critic = net_of<T>(c.critic);
    p.kind = c.kind; p.n_obs = c.n_obs; p.n_act = c.n_act; p.n_rows = c.n_rows; p.n_inner = c.n_inner; p.idx = c.idx;
    p.obs = rows_of<T>(c.obs);
    p.aout = (T*)c.action_out; p.aout_stride = c.action_out_stride; p.dqout = (T*)c.dqda_out; p.dqout_stride = c.dqda_out_stride;
    p.workspace = (T*)c.workspace;
    if (!with_ch(c.critic.n1, [&](auto ch) {   // the critic's first layer: the widest of the call
            hipLaunchKernelGGL((k_offgrad_actor<T, decltype(ch)::value>), dim3(blocks), dim3(kBlock), 0, s, p);
        }))
        return ATACOM_OFFGRAD_E_UNSUPPORTED;
    void* const grad[2] = {c.grad, c.grad};
    void* const stats[2] = {c.stats, c.stats};
    reduce<T>(c.workspace, grad, stats, 1, blocks, (int)partial_size(c.n_obs, c.n_act, 0), c.n_rows, s);
    return ATACOM_OFFGRAD_OK;
}

}  // namespace

int critic_launch(const CriticCall& c, int blocks, hipStream_t s) {
    if (c.dtype == ATACOM_OFFGRAD_F32) return launch_critic<float>(c, blocks, s);
    if (c.dtype == ATACOM_OFFGRAD_F64) return launch_critic<double>(c, blocks, s);
    return ATACOM_OFFGRAD_E_UNSUPPORTED;
}

int actor_launch(const ActorCall& c, int blocks, hipStream_t s) {
    if (c.dtype == ATACOM_OFFGRAD_F32) return launch_actor<float>(c, blocks, s);
    if (c.dtype == ATACOM_OFFGRAD_F64) return launch_actor<double>(c, blocks, s);
    return ATACOM_OFFGRAD_E_UNSUPPORTED;
}

}  // namespace atacom_offgrad
