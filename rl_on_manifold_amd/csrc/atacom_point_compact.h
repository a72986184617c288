// The collision-avoidance task's T-step kernel writing COMPACT records (libatacom_point_compact.so,
// include/atacom_point_compact_hip.h): the packed record of k_point_rollout_mlp without next_obs, which repeats the next
// step's obs except where an in-kernel reset came between -- what atacom_rollout_compact (atacom_kernels.h) is for the
// air-hockey tasks.  Rows 0..T-1 are records [obs | action(2) | reward | absorbing | last], row T the tail [obs after step
// T-1 | zeros]; every episode end at t < T-1 of an auto-resetting handle appends one row [t, b, terminal obs] to a list.
//
// Nothing of the environment or of the format is restated here: point_step, point_reset_generated, load_state / store_state
// and the generator keys are those of atacom_point.h; the record layout, the exception list and the slot of the observation
// after a step are RecordCompact, CompactEnds and compact_next_obs_slot of atacom_kernels.h, instantiated on the two numbers
// of this task they read (PointEnv); the network and its LDS layout are atacom_policy.h through PolicyLds of
// atacom_point_policy.h.  The one restatement is the exploration block (policy_action below, which says why).  The two
// kernels are compared bit for bit (tests/test_gpu_point_compact.py).
//
//   POLICY = false  pre-generated actions [T, B, 2]: the loop of k_point_rollout (next action fetched while the step computes),
//                   one environment per lane, no LDS, no staging, no matrix cores; lanes past the batch return at once.
//   POLICY = true   the actor network in the kernel, structured as k_point_rollout_mlp: float = matrix cores with shadow lanes
//                   in the last live wave (every store, the append included, masked off), double = the VALU form.
//
// Stores.  A record has 4 (1 + N) + 5 = 17 or 25 values: its base is aligned to ONE element only, so its fields are written
// element by element as PRecord's are; a wave's 64 records are one contiguous span which the L2 merges.  Exception rows are
// appended by an ordinary per-lane atomicAdd on the counter and written only below the capacity.  The tail's address is
// derived from the step's record pointer and (t, b) are converted inside the append branch (compact_next_obs_slot): as loop
// invariants they would be held in registers across the step loop (profiles/compact_collection.md).
#pragma once
#include "atacom_point_policy.h"

namespace atacom_point {

using atacom::CompactEnds;

// what RecordCompact and compact_next_obs_slot (atacom_kernels.h) read of an environment
template <int N>
struct PointEnv {
    static constexpr int OBS = Layout<N>::OBS, NK = 2;
};

// One step's action from the network: exploration (first half), the forward passes, exploration (second half), operation for
// operation and in the order of k_point_rollout_mlp (atacom_point_policy.h), whose block this RESTATES.  Lifting the block out
// of that kernel into a function both call was tried and dropped: the four kernels of libatacom_point_policy.so did not come out
// instruction-identical (float: +12 bytes of code each; double: +8 bytes of scratch, +0.3 / +7.8 KB of code;
// profiles/point_compact.md), and that library's device code stays as it is.  eps holds the step's noise on entry (the
// Ornstein-Uhlenbeck state after its update on exit); ep_step: the environment's episode step counter before the step.
template <typename T, int N>
__device__ __forceinline__ void policy_action(const MlpArgs<T>& net, T* lds, T* stage, const T* xc, const T* stdc, int ep_step,
                                              int b, bool valid, int lane, const T (&o)[Layout<N>::OBS], T (&eps)[2], T (&act)[2]) {
    using PL = PolicyLds<T, N>;
    using LM = typename PL::LM;
    using LV = typename PL::LV;
    constexpr bool MFMA = PL::MFMA;
    constexpr int D = PL::D, H = PL::H, NK = PL::NK, NB = PL::NB;
    // ---- exploration, first half (atacom_point_policy.h, atacom_kernels.h: k_rollout_mlp)
    if (net.explore == 2) {
        int bx = b;
        asm volatile("" : "+v"(bx));       // the address is formed anew each step, not held across the solver
        T* const xp = net.ou_state + (size_t)bx * NK;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const T x = ep_step == 0 ? xc[24 + k] : xp[k];
            eps[k] = num<T>::fma(xc[32 + k], eps[k], x - net.ou_theta_dt * x);
        }
        if (valid) {
#pragma unroll
            for (int k = 0; k < NK; ++k) xp[k] = eps[k];
        }
    }
    T sig[NK];
    if constexpr (MFMA) {
        float xin[NB][LM::CH];
        atacom::mlp_obs_to_operand<D, H, NK, NB>(lds, stage, o, lane, lane, xin);
        atacom::mlp_forward_mfma<D, H, NK, NB>(lds, stage, xin, net.activation, lane, lane, act);
        if (net.sW1) atacom::mlp_forward_mfma<D, H, NK, NB>(lds + LM::NET, stage, xin, net.activation, lane, lane, sig);
    } else {
        atacom::mlp_forward<T, D, H, NK, 1>(lds, lds, o, net.activation, 0, act);
        if (net.sW1) atacom::mlp_forward<T, D, H, NK, 1>(lds + LV::TOTAL, lds, o, net.activation, 0, sig);
    }
    // ---- exploration, second half
    if (net.sW1) {
#pragma unroll
        for (int k = 0; k < NK; ++k)
            sig[k] = num<T>::exp(num<T>::min(num<T>::max(sig[k], net.log_std_min), net.log_std_max));
    } else {
#pragma unroll
        for (int k = 0; k < NK; ++k) sig[k] = stdc[k];
    }
    if (net.mean_mode) {
#pragma unroll
        for (int k = 0; k < NK; ++k) act[k] = xc[k] * num<T>::tanh(act[k]);
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        act[k] = num<T>::fma(sig[k], eps[k], act[k]);
        if (net.squash) act[k] = num<T>::tanh(act[k]);
    }
    if (net.explore == 1) {
#pragma unroll
        for (int k = 0; k < NK; ++k) act[k] = num<T>::clamp(act[k], xc[8 + k], xc[16 + k]);
    } else if (net.explore == 2) {
#pragma unroll
        for (int k = 0; k < NK; ++k) act[k] += eps[k];
    }
}

// the step's reward and flags, then the observation after the step where the format wants it (committing lanes only)
template <typename T, int N>
__device__ __forceinline__ void compact_close_step(const PParams<T>& P, const CompactEnds<T>& cx, const PState<T, N>& st,
                                                   T* rrow, int rec_ld, int n_steps, int t, int b, T r, bool lst) {
    using RC = atacom::RecordCompact<PointEnv<N>>;
    rrow[RC::REW] = r;
    rrow[RC::ABS] = T(0);                                                               // base:80: never absorbing
    rrow[RC::LAST] = lst ? T(1) : T(0);
    T* const nd = atacom::compact_next_obs_slot<T, PointEnv<N>>(cx, rrow, rec_ld, n_steps, t, b, P.auto_reset && lst);
    if (nd) {
        T on[Layout<N>::OBS];
        state_to_obs<T, N>(st, on);
#pragma unroll
        for (int i = 0; i < Layout<N>::OBS; ++i) nd[i] = on[i];
    }
}

// actions_in [T, B, 2] (POLICY = false) or the network `net` with noise [T, B, 2] (nullable = zeros); draws [T, B, N, 2]
// (nullable = the generator, the keys of k_point_rollout); rec [T + 1, rec_ld, RecordCompact::F]; cx the exception list.
template <typename T, int N, bool POLICY>
__global__ void __launch_bounds__(BLOCK) k_point_rollout_compact(const PParams<T> P, const MlpArgs<T> net, int n_steps,
                                                                 T* __restrict__ f, int* __restrict__ ip,
                                                                 const T* __restrict__ actions_in,
                                                                 const T* __restrict__ noise, const T* __restrict__ draws,
                                                                 T* __restrict__ rec, int rec_ld, const CompactEnds<T> cx) {
    using L = Layout<N>;
    using RC = atacom::RecordCompact<PointEnv<N>>;
    constexpr int D = L::OBS, NK = 2;
    const int B = P.batch;
    const int gt = blockIdx.x * BLOCK + threadIdx.x;
    if constexpr (!POLICY) {
        const int b = gt;
        if (b >= B) return;
        PState<T, N> st;
        load_state<T, N>(f, ip, B, b, st);
        T ssum = T(0), scmax = pl(f, L::SCMAX, B, b);
        // the actions of step t + 1 are fetched while step t computes (k_point_rollout)
        T act_next[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) act_next[k] = (n_steps > 0) ? actions_in[(size_t)b * NK + k] : T(0);
#pragma unroll 1
        for (int t = 0; t < n_steps; ++t) {
            const size_t row = (size_t)t * B + b;
            const T alpha[2] = {act_next[0], act_next[1]};
            {
                const size_t nrow = (size_t)((t + 1 < n_steps) ? t + 1 : t) * B + b;    // last step: a harmless re-read
                act_next[0] = actions_in[nrow * NK];
                act_next[1] = actions_in[nrow * NK + 1];
            }
            T* const rrow = rec + ((size_t)t * rec_ld + b) * RC::F;
            {
                T o[D];
                state_to_obs<T, N>(st, o);
#pragma unroll
                for (int i = 0; i < D; ++i) rrow[RC::OBS + i] = o[i];
#pragma unroll
                for (int k = 0; k < NK; ++k) rrow[RC::ACT + k] = alpha[k];
            }
            T r, cmax;
            const int t0 = st.t, ep = st.ep - 1;
            if (draws) point_step<T, N>(P, st, alpha, [&](int i, int c) { return draws[(row * N + i) * 2 + c]; }, r, cmax);
            else point_step<T, N>(P, st, alpha, [&](int i, int c) {
                    return num<T>::fma(T(2), atacom::device_uniform<T>(P.seed, b, ep, 2 * N + 2 * (N * t0 + i) + c), T(-1));
                }, r, cmax);
            const bool lst = st.t >= P.horizon;
            compact_close_step<T, N>(P, cx, st, rrow, rec_ld, n_steps, t, b, r, lst);
            ssum += cmax;
            scmax = num<T>::max(scmax, cmax);
            if (P.auto_reset && lst) point_reset_generated<T, N>(P, b, st);
        }
        pl(f, L::SSUM, B, b) += ssum;
        pl(f, L::SCMAX, B, b) = scmax;
        ip[(size_t)b * 4 + L::I_CNT] += n_steps;
        store_state<T, N>(f, ip, B, b, st);
    } else {
        using PL = PolicyLds<T, N>;
        using LM = typename PL::LM;
        using LV = typename PL::LV;
        constexpr bool MFMA = PL::MFMA;
        constexpr int H = PL::H, NB = PL::NB;
        extern __shared__ __attribute__((aligned(16))) char smem[];
        T* lds = reinterpret_cast<T*>(smem);
        // the whole workgroup stages and passes every barrier before any lane leaves
        if constexpr (MFMA) atacom::mlp_stage_mfma<D, H, NK>(net, lds, threadIdx.x, BLOCK, PL::STAGE);
        else atacom::mlp_stage<T, D, H, NK>(net, lds, threadIdx.x, BLOCK);
        const bool valid = gt < B;
        if constexpr (MFMA) {
            // a lane past the batch in a live wave supplies operand slices of its GEMM block and takes part in the wave's
            // staging: it shadows the last environment with every store masked off (k_point_rollout_mlp)
            if ((gt & ~(WAVE - 1)) >= B) return;
        } else {
            if (!valid) return;
        }
        const int b = valid ? gt : B - 1;
        const int lane = threadIdx.x & (WAVE - 1);
        T* stage = lds + 2 * LM::NET + (threadIdx.x / WAVE) * LM::wave_stage(NB);      // MFMA path only
        PState<T, N> st;
        load_state<T, N>(f, ip, B, b, st);
        T ssum = T(0), scmax = pl(f, L::SCMAX, B, b);
        const T* const xc = lds + (MFMA ? (int)LM::EXPLORE : (int)LV::EXPLORE);
        const T* const stdc = lds + (MFMA ? (int)LM::STD : (int)LV::STD);
#pragma unroll 1
        for (int t = 0; t < n_steps; ++t) {
            const size_t row = (size_t)t * B + b;
            // everything the step reads from memory is requested before the network runs (k_point_rollout_mlp)
            T eps[NK], dr[N][2];
#pragma unroll
            for (int k = 0; k < NK; ++k) eps[k] = noise ? noise[row * NK + k] : T(0);
#pragma unroll
            for (int i = 0; i < N; ++i)
#pragma unroll
                for (int c = 0; c < 2; ++c) dr[i][c] = draws ? draws[(row * N + i) * 2 + c] : T(0);
            T o[D];
            state_to_obs<T, N>(st, o);
            T act[NK];
            policy_action<T, N>(net, lds, stage, xc, stdc, st.t, b, valid, lane, o, eps, act);
            // the value recorded IS the value the step receives (k_point_rollout_mlp: nothing of the exploration may be
            // contracted into the chart's first products)
#pragma unroll
            for (int k = 0; k < NK; ++k) asm volatile("" : "+v"(act[k]));
            T* const rrow = rec + ((size_t)t * rec_ld + b) * RC::F;
            if (valid) {
#pragma unroll
                for (int i = 0; i < D; ++i) rrow[RC::OBS + i] = o[i];
#pragma unroll
                for (int k = 0; k < NK; ++k) rrow[RC::ACT + k] = act[k];
            }
            const T alpha[2] = {act[0], act[1]};
            T r, cmax;
            const int t0 = st.t, ep = st.ep - 1;
            if (draws) point_step<T, N>(P, st, alpha, [&](int i, int c) { return dr[i][c]; }, r, cmax);
            else point_step<T, N>(P, st, alpha, [&](int i, int c) {
                    return num<T>::fma(T(2), atacom::device_uniform<T>(P.seed, b, ep, 2 * N + 2 * (N * t0 + i) + c), T(-1));
                }, r, cmax);
            const bool lst = st.t >= P.horizon;
            if (valid) compact_close_step<T, N>(P, cx, st, rrow, rec_ld, n_steps, t, b, r, lst);
            ssum += cmax;
            scmax = num<T>::max(scmax, cmax);
            if (P.auto_reset && lst) point_reset_generated<T, N>(P, b, st);
        }
        if (!valid) return;
        pl(f, L::SSUM, B, b) += ssum;
        pl(f, L::SCMAX, B, b) = scmax;
        ip[(size_t)b * 4 + L::I_CNT] += n_steps;
        store_state<T, N>(f, ip, B, b, st);
    }
}

}  // namespace atacom_point
