// The collision-avoidance task's T-step kernel with the actor network evaluated INSIDE it (libatacom_point_policy.so,
// include/atacom_point_policy_hip.h): observation -> 2 x 64 MLP -> exploration -> point_step, T times, the environment's
// state in registers -- what k_rollout_mlp (atacom_kernels.h) is for the air-hockey tasks.  Replaces the per-step loop of
// mushroom_rl.core.Core around examples/collision_avoidance_exp.py's agents (policy.draw_action + mdp.step).
//
// Nothing of the environment is restated here: point_step, point_reset_generated, the state layout and the row writer are
// those of atacom_point.h, so the env arithmetic is the same source as k_point_rollout and the two kernels are compared bit
// for bit (tests/test_gpu_point_policy.py).  The network is atacom_policy.h as it is:
//   float   one environment per lane, a wave = four GEMM blocks of 16 environments: mlp_stage_mfma once per workgroup,
//           mlp_obs_to_operand + mlp_forward_mfma<4 (1 + N), 64, 2, 4> per step (second pass for SAC's sigma network);
//   double  mlp_stage + the VALU form mlp_forward<..., LANES = 1>.
// The exploration block mirrors that of k_rollout_mlp (atacom_kernels.h), operation for operation and in its order.  It is
// restated and not lifted into shared forced-inline device functions because such a lift changes the generated code of every
// k_rollout_mlp instantiation (measured on the planar unit: -66 to +120 instructions per kernel): it needs an A/B on hardware.
//
// LDS.  float: [mean net | sigma net | per-wave staging] = 2 x 31 008 B + 40 960 B = 102 976 B, the layout mlp_stage_mfma
// zeroes and fills (the sigma block is reserved whether or not there is one: the staging helper addresses the per-wave area
// behind two blocks).  double: one or two MlpLds blocks, 40 - 53 KB each.  Either way one workgroup per CU -- which is
// also what the registers allow (the float kernels hold the four blocks' accumulators: one wave per SIMD).
//
// Output.  Arrays: obs / next_obs rows are the 16-byte row stores of atacom_point.h (plain, not non-temporal: see there).
// Packed records [obs | action(2) | reward | next_obs | absorbing | last] have 2 * 4 (1 + N) + 5 = 29 or 45 values: a record's
// base is aligned to ONE element only, so its fields are written element by element like the main library's packed writer
// (atacom_kernels.h:1455-1478); a wave's 64 records are one contiguous span which the L2 merges.  Rows batch..stride-1 of a
// padded record buffer are never written.
#pragma once
#include "atacom_point.h"
#include "atacom_policy.h"

namespace atacom_point {

using atacom::MlpArgs;
using atacom::MlpLds;
using atacom::MlpLdsM;

template <int N>
struct PRecord {
    static constexpr int OBS = 0, ACT = Layout<N>::OBS, REW = ACT + 2, NOBS = REW + 1, ABS = NOBS + Layout<N>::OBS,
                         LAST = ABS + 1, F = LAST + 1;
};

constexpr int WAVE = 64;

template <typename T, int N>
struct PolicyLds {
    static constexpr int D = Layout<N>::OBS, H = 64, NK = 2, NB = 4;          // NB: blocks of 16 environments per wave
    static constexpr bool MFMA = std::is_same<T, float>::value;
    using LM = MlpLdsM<D, H, NK>;
    using LV = MlpLds<D, H, NK>;
    static constexpr int STAGE = (BLOCK / WAVE) * LM::wave_stage(NB);         // floats of per-wave staging per workgroup
    static size_t bytes(bool sigma_net) {
        const size_t n = MFMA ? (size_t)(2 * LM::NET + STAGE) : (size_t)((sigma_net ? 2 : 1) * LV::TOTAL);
        return sizeof(T) * (((n + 3) / 4) * 4);
    }
};

template <typename T, int N>
__device__ __forceinline__ void state_to_obs(const PState<T, N>& st, T (&o)[Layout<N>::OBS]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = st.r[c];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) o[4 * (1 + i) + c] = st.o[i][c];
}

// actions_in != nullptr: pre-generated actions [T, B, 2], no network (the packed-record form of k_point_rollout; `net` is
// not read and nothing is staged).  Otherwise the network draws the action.  noise [T, B, 2] (nullable = zeros), draws
// [T, B, N, 2] (nullable = the generator, the keys of k_point_rollout).  rec != nullptr: packed records
// [T, rec_ld, PRecord::F] instead of the six arrays.
template <typename T, int N>
__global__ void __launch_bounds__(BLOCK) k_point_rollout_mlp(const PParams<T> P, const MlpArgs<T> net, int n_steps,
                                                             T* __restrict__ f, int* __restrict__ ip,
                                                             const T* __restrict__ actions_in,
                                                             const T* __restrict__ noise, const T* __restrict__ draws,
                                                             T* __restrict__ obs, T* __restrict__ next_obs,
                                                             T* __restrict__ actions_out, T* __restrict__ reward,
                                                             uint8_t* __restrict__ absorbing, uint8_t* __restrict__ last,
                                                             T* __restrict__ rec, int rec_ld) {
    using L = Layout<N>;
    using R = PRecord<N>;
    using PL = PolicyLds<T, N>;
    using LM = typename PL::LM;
    using LV = typename PL::LV;
    constexpr bool MFMA = PL::MFMA;
    constexpr int D = PL::D, H = PL::H, NK = PL::NK, NB = PL::NB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* lds = reinterpret_cast<T*>(smem);
    // the whole workgroup stages and passes every barrier before any lane leaves (launch-uniform branch)
    if (!actions_in) {
        if constexpr (MFMA) atacom::mlp_stage_mfma<D, H, NK>(net, lds, threadIdx.x, BLOCK, PL::STAGE);
        else atacom::mlp_stage<T, D, H, NK>(net, lds, threadIdx.x, BLOCK);
    }
    const int B = P.batch;
    const int gt = blockIdx.x * BLOCK + threadIdx.x;
    const bool valid = gt < B;
    if constexpr (MFMA) {
        // a lane past the batch in a live wave supplies operand slices of its GEMM block and takes part in the wave's
        // staging: it shadows the last environment with every store masked off
        if ((gt & ~(WAVE - 1)) >= B) return;
    } else {
        if (!valid) return;
    }
    const int b = valid ? gt : B - 1;
    const int lane = threadIdx.x & (WAVE - 1);
    T* stage = lds + 2 * LM::NET + (threadIdx.x / WAVE) * LM::wave_stage(NB);          // MFMA path only
    PState<T, N> st;
    load_state<T, N>(f, ip, B, b, st);
    T ssum = T(0), scmax = pl(f, L::SCMAX, B, b);
    // [act_scale | act_low | act_high | x0 | std sqrt(dt)] of the TD3 / DDPG modes (atacom_policy.h: mlp_stage_explore)
    const T* const xc = lds + (MFMA ? (int)LM::EXPLORE : (int)LV::EXPLORE);
    const T* const stdc = lds + (MFMA ? (int)LM::STD : (int)LV::STD);
#pragma unroll 1
    for (int t = 0; t < n_steps; ++t) {
        const size_t row = (size_t)t * B + b;
        // everything the step reads from memory is requested before the network runs (its wave fences would pin the loads
        // behind it): the noise, the supplied draws, or the pre-generated action
        T eps[NK], dr[N][2];
#pragma unroll
        for (int k = 0; k < NK; ++k) eps[k] = actions_in ? actions_in[row * NK + k] : (noise ? noise[row * NK + k] : T(0));
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int c = 0; c < 2; ++c) dr[i][c] = draws ? draws[(row * N + i) * 2 + c] : T(0);
        T o[D];
        state_to_obs<T, N>(st, o);
        T act[NK];
        if (actions_in) {
#pragma unroll
            for (int k = 0; k < NK; ++k) act[k] = eps[k];
        } else {
            // ---- exploration, first half: mirrors atacom_kernels.h:1394-1413
            if (net.explore == 2) {
                int bx = b;
                asm volatile("" : "+v"(bx));       // the address is formed anew each step, not held across the solver
                T* const xp = net.ou_state + (size_t)bx * NK;
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const T x = st.t == 0 ? xc[24 + k] : xp[k];
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
            // ---- exploration, second half: mirrors atacom_kernels.h:1426-1453
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
        // the value recorded IS the value the step receives: no operation of the exploration above can be contracted into
        // the chart's first products (k_point_rollout reads its action from memory; the two must agree bit for bit)
#pragma unroll
        for (int k = 0; k < NK; ++k) asm volatile("" : "+v"(act[k]));
        T* const rrow = rec ? rec + ((size_t)t * rec_ld + b) * R::F : nullptr;
        if (valid) {
            if (rec) {
#pragma unroll
                for (int i = 0; i < D; ++i) rrow[R::OBS + i] = o[i];
#pragma unroll
                for (int k = 0; k < NK; ++k) rrow[R::ACT + k] = act[k];
            } else {
                write_row<T, N>(st, obs + row * L::OBS);
#pragma unroll
                for (int k = 0; k < NK; ++k) actions_out[row * NK + k] = act[k];
            }
        }
        const T alpha[2] = {act[0], act[1]};
        T r, cmax;
        const int t0 = st.t, ep = st.ep - 1;
        if (draws) point_step<T, N>(P, st, alpha, [&](int i, int c) { return dr[i][c]; }, r, cmax);
        else point_step<T, N>(P, st, alpha, [&](int i, int c) {
                return num<T>::fma(T(2), atacom::device_uniform<T>(P.seed, b, ep, 2 * N + 2 * (N * t0 + i) + c), T(-1));
            }, r, cmax);
        const bool lst = st.t >= P.horizon;
        if (valid) {
            if (rec) {
                T on[D];
                state_to_obs<T, N>(st, on);
#pragma unroll
                for (int i = 0; i < D; ++i) rrow[R::NOBS + i] = on[i];
                rrow[R::REW] = r;
                rrow[R::ABS] = T(0);                                                    // base:80: never absorbing
                rrow[R::LAST] = lst ? T(1) : T(0);
            } else {
                if (next_obs) write_row<T, N>(st, next_obs + row * L::OBS);
                reward[row] = r;
                absorbing[row] = 0;
                last[row] = lst ? 1 : 0;
            }
        }
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

}  // namespace atacom_point
