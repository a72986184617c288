// Instantiates the kernels of atacom_kernels.h for one environment and fills its EnvOps tables.
#pragma once
#include "atacom_kernels.h"
#include "atacom_mlp_host.h"
#include "atacom_ops.h"

namespace atacom {

template <typename T>
static Params<T> make_params(const atacom_config& c) {
    Params<T> P;
    P.batch = c.batch; P.substeps = c.substeps; P.horizon = c.horizon; P.hold_q = c.hold_q;
    P.bias_mode = c.bias_mode; P.auto_reset = c.auto_reset;
    P.random_init = c.random_init; P.seed = (unsigned int)c.seed; P.dynamics_mode = c.dynamics_mode; P.task = c.task;
    P.dt = (T)c.dt; P.dt_base = (T)(c.dt_base > 0 ? c.dt_base : c.dt); P.rref_tol = (T)c.rref_tol; P.action_penalty = (T)c.action_penalty;
    double amax = c.acc_max[0];
    for (int i = 0; i < ATACOM_MAX_C; ++i) { P.K[i] = (T)c.K[i]; P.Kc[i] = (T)c.Kc[i]; }
    for (int i = 0; i < ATACOM_MAX_Q; ++i) {
        P.vel_max[i] = (T)c.vel_max[i]; P.acc_max[i] = (T)c.acc_max[i]; P.Kq[i] = (T)c.Kq[i];
        P.pos_limit[i] = (T)c.pos_limit[i];
    }
    const int nq = c.env_id == ATACOM_ENV_PLANAR ? 3 : (c.env_id == ATACOM_ENV_IIWA ? 6 : 2);
    for (int i = 1; i < nq; ++i) amax = c.acc_max[i] > amax ? c.acc_max[i] : amax;
    P.alpha_max = (T)amax;                       // atacom.py:71
    P.base_x = (T)c.base_xy[0]; P.base_y = (T)c.base_xy[1];
    for (int i = 0; i < 3; ++i) P.link[i] = (T)c.link[i];
    // env_base.py:155-159, env_hitting.py:11-12, iiwa_hit_atacom.py:104-105
    const double table_l = 1.96, table_w = 1.02, mallet_r = 0.05;
    P.table_bx = (T)(table_l / 2 - mallet_r); P.table_by = (T)(table_w / 2 - mallet_r);
    P.table_hx = (T)(table_l / 2); P.table_hy = (T)(table_w / 2);
    P.goal_x = (T)0.98; P.goal_y = (T)0.0; P.goal_w = (T)0.25;
    P.ee_height = (T)0.1505; P.z4_min = (T)0.36; P.z7_min = (T)0.25;
    P.puck_r = (T)0.03165; P.mallet_r = (T)mallet_r; P.e_mallet = (T)0.8; P.e_rim = (T)0.8;
    P.term_tol = (T)c.term_tol;
    P.noise = (c.obs_noise ? NOISE_OBS : 0) | (c.obs_delay ? NOISE_DELAY : 0) | (c.env_noise ? NOISE_ENV : 0);
    P.obs_noise_std = (T)0.001;                                               // env_single.py:105-107
    P.env_noise_dv = (T)(0.0005 * c.dt / (c.puck_mass > 0 ? c.puck_mass : 0.01));   // env_base.py:176-180
    return P;
}

static inline int nblk(int n, int per) { return (n + per - 1) / per; }

template <typename T>
static CompactEnds<T> compact_ends(const CompactArgs* cx) {
    return cx ? CompactEnds<T>{(T*)cx->ends, cx->count, cx->cap} : CompactEnds<T>{nullptr, nullptr, 0};
}

// ------------------------------------------------------------------ the census of lane mappings (round 6)
// Which "lanes per environment" forms of the stepping kernels are INSTANTIATED for a (scalar type, environment, variant).
// One rule, shared by the dispatchers below and -- through lanes_run in the launch tables -- by the C ABI, so that
// atacom_get_lanes reports what really runs:
//   * circle family: one environment per lane only (its step is launch-bound, wider groups were never selected);
//   * rigid-body kernels: lane and quad (the dynamics are computed redundantly by a group's lanes: wider groups buy nothing);
//   * float64: 1, 4 and (iiwa) 8 lanes -- the mappings the float64 policy picks (atacom_capi.cpp) and the parity tests hold
//     to 1e-8; the lane pair exists in float32 only; the float64 policy kernel exists on the quad and the lane;
//   * float32: 1, 2, 4, 8; the 8-lane policy kernel in its matrix-core form only.
// A request for a mapping that is not instantiated runs the widest narrower one.
enum { KIND_STEP = 0, KIND_ROLLOUT = 1, KIND_MLP = 2 };
template <typename T, typename E, bool DYN>
constexpr bool has_mapping(int lanes, int kind) {
    if (lanes == 1) return true;
    if (E::ID == 0) return false;
    if (DYN) return lanes == 4;
    if (std::is_same<T, double>::value) {
        if (kind == KIND_MLP) return lanes == 4;
        return lanes == 4 || (lanes == 8 && E::ID == 2);
    }
    if (kind == KIND_MLP && lanes == 8) return MlpPath<T, E, 8, 64>::MFMA;
    return lanes == 2 || lanes == 4 || lanes == 8;
}
template <typename T, typename E, bool DYN>
constexpr int mapping_run(int lanes, int kind) {
    for (int l = 8; l > 1; l /= 2)
        if (l <= lanes && has_mapping<T, E, DYN>(l, kind)) return l;
    return 1;
}

// The step / rollout / policy-rollout launchers of one kernel VARIANT: kinematic or rigid-body dynamics (DYN, iiwa, row
// N4), the reference's chart or the canonical one (CHART, atacom_chart.h).  Mappings: LANES in {1, 2, 4, 8}, x HOLD; the
// rigid-body kernels exist for one environment per lane and per quad (the dynamics are computed redundantly by the lanes of
// a group: wider groups buy nothing), atacom_capi.cpp clamps the mapping accordingly.
// NOISE: the kernels with the domain-randomisation options compiled in (planar / iiwa, kinematic mode; atacom_noise_*.hip).
template <typename T, typename E, bool DYN, int CHART, bool NOISE = false>
struct Variant {
    static_assert(!NOISE || (E::PUCK && !DYN), "noise kernels: air-hockey environments, kinematic mode");
    // (kind: KIND_STEP / KIND_ROLLOUT share their mappings; the policy kernel has its own list, see rollout_mlp)
    template <int KIND, typename F>
    static void with_mapping(int lanes, bool hold, F&& f) {
        auto go = [&](auto lc) {
            if (hold) f(lc, std::true_type{});
            else f(lc, std::false_type{});
        };
        const int l = mapping_run<T, E, DYN>(lanes, KIND);
        if constexpr (has_mapping<T, E, DYN>(8, KIND)) { if (l == 8) return go(std::integral_constant<int, 8>{}); }
        if constexpr (has_mapping<T, E, DYN>(4, KIND)) { if (l == 4) return go(std::integral_constant<int, 4>{}); }
        if constexpr (has_mapping<T, E, DYN>(2, KIND)) { if (l == 2) return go(std::integral_constant<int, 2>{}); }
        return go(std::integral_constant<int, 1>{});
    }
    static int lanes_run(int kind, int lanes) { return mapping_run<T, E, DYN>(lanes, kind); }
    static void step(const atacom_config& c, int lanes, void* f, int* ip, const void* act, void* obs, void* rew,
                     uint8_t* ab, uint8_t* last, const uint8_t* mask, hipStream_t s) {
        with_mapping<KIND_STEP>(lanes, c.hold_q != 0, [&](auto lc, auto hc) {
            constexpr int LANES = decltype(lc)::value;
            constexpr bool HOLD = decltype(hc)::value;
            hipLaunchKernelGGL((k_step<T, E, LANES, HOLD, DYN, CHART, NOISE>), dim3(nblk(c.batch * LANES, BLOCK<LANES>)),
                               dim3(BLOCK<LANES>), 0, s, make_params<T>(c), (T*)f, ip, (const T*)act, (T*)obs, (T*)rew, ab,
                               last, mask);
        });
    }
    static void rollout(const atacom_config& c, int lanes, int n_steps, void* f, int* ip, const void* acts, void* obs,
                        void* nobs, void* rew, uint8_t* ab, uint8_t* last, void* rec, int rec_ld, const CompactArgs* cx,
                        hipStream_t s) {
        with_mapping<KIND_ROLLOUT>(lanes, c.hold_q != 0, [&](auto lc, auto hc) {
            constexpr int LANES = decltype(lc)::value;
            constexpr bool HOLD = decltype(hc)::value;
            hipLaunchKernelGGL((k_rollout<T, E, LANES, HOLD, DYN, CHART, NOISE>), dim3(nblk(c.batch * LANES, BLOCK<LANES>)),
                               dim3(BLOCK<LANES>), 0, s, make_params<T>(c), n_steps, (T*)f, ip, (const T*)acts, (T*)obs,
                               (T*)nobs, (T*)rew, ab, last, (T*)rec, rec_ld, compact_ends<T>(cx));
        });
    }
    template <int LANES, bool HOLD>
    static void launch_mlp(const atacom_config& c, int n_steps, const MlpArgs<T>& a, void* f, int* ip,
                           const void* noise, void* obs, void* nobs, void* acts, void* rew, uint8_t* ab,
                           uint8_t* last, void* rec, int rec_ld, const CompactArgs* cx, hipStream_t s) {
        constexpr int H = 64;
        size_t lds_floats = 2 * MlpLds<E::OBS, H, E::NK>::TOTAL;
        if constexpr (MlpPath<T, E, LANES, H>::MFMA) {
            using MP = MlpPath<T, E, LANES, H>;
            lds_floats = 2 * MP::LM::NET + MP::STAGE;
        }
        const size_t lds_bytes = sizeof(T) * (((lds_floats + 3) / 4) * 4);
        constexpr int THREADS = MlpPath<T, E, LANES, H>::THREADS;
        hipLaunchKernelGGL((k_rollout_mlp<T, E, LANES, HOLD, H, DYN, CHART, NOISE>), dim3(nblk(c.batch * LANES, THREADS)),
                           dim3(THREADS), lds_bytes, s, make_params<T>(c), a, n_steps, (T*)f, ip, (const T*)noise, (T*)obs,
                           (T*)nobs, (T*)acts, (T*)rew, ab, last, (T*)rec, rec_ld, compact_ends<T>(cx));
    }
    static int rollout_mlp(const atacom_config& c, int lanes, int n_steps, const atacom_mlp& net, void* f, int* ip,
                           const void* noise, void* obs, void* nobs, void* acts, void* rew, uint8_t* ab, uint8_t* last,
                           void* rec, int rec_ld, const CompactArgs* cx, hipStream_t s) {
        if (E::ID == 0 || net.hidden != 64) return ATACOM_E_UNSUPPORTED;
        const MlpArgs<T> a = mlp_args<T>(net);
        if constexpr (E::ID != 0) {
            // float64 (the parity build): the policy kernel exists for the default variant only -- reference chart, kinematic,
            // no domain randomisation -- which is what the 1e-8 parity tests of row N2 run (tests/test_gpu_parity.py)
            // float32: every variant except the canonical chart TOGETHER WITH the noise options or the rigid-body mode (two
            // opt-ins on top of the opt-in chart; never selected by a test or a bench record -- pruned in round 6)
            if constexpr ((std::is_same<T, double>::value && (DYN || CHART != 0 || NOISE)) || (CHART != 0 && (DYN || NOISE)))
                return ATACOM_E_UNSUPPORTED;
            else
            with_mapping<KIND_MLP>(lanes, c.hold_q != 0, [&](auto lc, auto hc) {
                launch_mlp<decltype(lc)::value, decltype(hc)::value>(c, n_steps, a, f, ip, noise, obs, nobs, acts, rew, ab,
                                                                     last, rec, rec_ld, cx, s);
            });
        }
        return ATACOM_OK;
    }
    static void chart_mu(int n, const void* A, const void* sl, const void* y, const void* alpha, double tol, void* mu,
                         hipStream_t s) {
        if constexpr (E::MODE == 0 && !DYN && !NOISE)
            hipLaunchKernelGGL((k_chart<T, E>), dim3(nblk(n, WAVE)), dim3(WAVE), 0, s, n, (const T*)A, (const T*)sl,
                               (const T*)y, (const T*)alpha, (T)tol, (T*)mu);
    }
    static const VariantOps* table() {
        static const VariantOps ops = {&step, &rollout, &rollout_mlp, &chart_mu, &lanes_run};
        return &ops;
    }
};

template <typename T, typename E>
struct Ops {
    using L = Planes<E>;
    using V = Variant<T, E, false, 0>;
    static void reset(const atacom_config& c, void* f, int* ip, const uint8_t* mask, const void* init, void* obs,
                      hipStream_t s) {
        hipLaunchKernelGGL((k_reset<T, E>), dim3(nblk(c.batch, WAVE)), dim3(WAVE), 0, s, make_params<T>(c), (T*)f, ip,
                           mask, (const T*)init, (T*)obs);
    }
    static void fill_init(const atacom_config& c, void* f, int* ip, const void* row, hipStream_t s) {
        hipLaunchKernelGGL((k_fill_init<T, E>), dim3(nblk(c.batch, 256)), dim3(256), 0, s, c.batch, (T*)f, ip,
                           (const T*)row);
    }
    static void clear_stats(const atacom_config& c, void* f, int* ip, hipStream_t s) {
        hipLaunchKernelGGL((k_clear_stats<T, E>), dim3(nblk(c.batch, 256)), dim3(256), 0, s, c.batch, (T*)f, ip);
    }
    static void stats(const atacom_config& c, const void* f, const int* ip, double* partial, int nblocks,
                      hipStream_t s) {
        hipLaunchKernelGGL((k_stats<T, E>), dim3(nblocks), dim3(256), 0, s, c.batch, (const T*)f, ip, partial);
    }
    static void get_state(const atacom_config& c, const void* f, const int* ip, void* out, hipStream_t s) {
        hipLaunchKernelGGL((k_get_state<T, E>), dim3(nblk(c.batch, 256)), dim3(256), 0, s, c.batch, (const T*)f, ip,
                           (T*)out);
    }
    static void set_state(const atacom_config& c, void* f, int* ip, const void* in, hipStream_t s) {
        hipLaunchKernelGGL((k_set_state<T, E>), dim3(nblk(c.batch, 256)), dim3(256), 0, s, c.batch, (T*)f, ip,
                           (const T*)in);
    }
    static void nullspace(int lanes, int n, const void* Jc, const void* rhs, double tol, void* x, void* nullb,
                          void* rref, hipStream_t s) {
        // the lane-group solver as a primitive, on the mappings of the stepping kernels (has_mapping)
        const int l = mapping_run<T, E, false>(lanes, KIND_STEP);
        auto quad = [&](auto lc) {
            constexpr int LN = decltype(lc)::value;
            hipLaunchKernelGGL((k_nullspace_quad<T, E, LN>), dim3(nblk(n * LN, WAVE)), dim3(WAVE), 0, s, n, (const T*)Jc,
                               (const T*)rhs, (T)tol, (T*)x, (T*)nullb, (T*)rref);
        };
        if constexpr (has_mapping<T, E, false>(8, KIND_STEP)) { if (l == 8) return quad(std::integral_constant<int, 8>{}); }
        if constexpr (has_mapping<T, E, false>(4, KIND_STEP)) { if (l == 4) return quad(std::integral_constant<int, 4>{}); }
        if constexpr (has_mapping<T, E, false>(2, KIND_STEP)) { if (l == 2) return quad(std::integral_constant<int, 2>{}); }
        hipLaunchKernelGGL((k_nullspace<T, E>), dim3(nblk(n, WAVE)), dim3(WAVE), 0, s, n, (const T*)Jc,
                           (const T*)rhs, (T)tol, (T*)x, (T*)nullb, (T*)rref);
    }
    static void terms(const atacom_config& c, int n, const void* q, const void* dq, void* fun, void* J, void* b,
                      hipStream_t s) {
        hipLaunchKernelGGL((k_terms<T, E>), dim3(nblk(n, WAVE)), dim3(WAVE), 0, s, make_params<T>(c), n,
                           (const T*)q, (const T*)dq, (T*)fun, (T*)J, (T*)b);
    }
    static void filter_io(const atacom_config& c, void* f, void* buf, int set, hipStream_t s) {
        hipLaunchKernelGGL((k_filter_io<T, E>), dim3(nblk(c.batch, 256)), dim3(256), 0, s, c.batch, (T*)f, (T*)buf, set);
    }
    static const EnvOps* table() {
        static const EnvOps ops = {L::VALUES_PER_ENV, L::ICOUNT, L::STATE_DIM, L::INIT_DIM, E::OBS, E::NQ, E::NF, E::NG, E::NK,
                                   sizeof(T), &V::step, &V::rollout, &V::rollout_mlp, &reset, &fill_init, &clear_stats, &stats,
                                   &get_state, &set_state, &nullspace, &terms, &filter_io, &V::lanes_run};
        return &ops;
    }
};

}  // namespace atacom
