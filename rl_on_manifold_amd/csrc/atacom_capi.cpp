// C-ABI host side of libatacom_hip.so (see include/atacom_hip.h).  Owns the per-handle device state
// and dispatches to the per-environment launch tables; contains no numerics.
#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "atacom_mlp_host.h"
#include "atacom_ops.h"
#define ATACOM_CAPI_E_HIP ATACOM_E_HIP
#include "atacom_capi_common.h"      // g_err, fail, HIP_TRY, DeviceGuard, ON_DEVICE

namespace {

const atacom::EnvOps* get_ops(int env_id, int dtype) {
    if (dtype != ATACOM_F32 && dtype != ATACOM_F64) return nullptr;
    switch (env_id) {
        case ATACOM_ENV_CIRCLE: return atacom::ops_circle(dtype);
        case ATACOM_ENV_PLANAR: return atacom::ops_planar(dtype);
        case ATACOM_ENV_IIWA: return atacom::ops_iiwa(dtype);
        case ATACOM_ENV_CIRCLE_EC: return atacom::ops_circle_ec(dtype);
        case ATACOM_ENV_CIRCLE_T: return atacom::ops_circle_t(dtype);
        default: return nullptr;
    }
}

constexpr int kStatBlocks = 256;

// kernel mapping policy for lanes_per_env = 0, from measurements on MI355X (profiles/r02_lanes_vs_batch.md): the fewer
// lanes an environment is spread over, the fewer instructions in total but the more per wave; a mapping's step time is
// flat while its waves still find a SIMD each (1024 SIMDs) and doubles beyond.  iiwa: 8 lanes, then the quad up to 16384
// envs, the pair up to 32768, the lane beyond.  The 8-lane mapping has 12 % fewer instructions per wave than the quad
// and wins wherever it leaves half of the chip idle like the quad does at twice the batch (<= 4096 envs: 25.3 vs 26.0 us
// per step, rollout kernels 22.0 vs 24.0 us per step, on every box tried).  At 8192 envs its 1024 waves occupy every CU:
// the clock drops and the launch / load / store phase of a step grows, so single-step launches tie with the quad (27.2 us
// both, mean of nine boxes; per box from 5 % faster to 4.5 % slower) and stayed on the quad through round 3 (round 4: 8
// lanes, see pick_lanes_raw), while the T-step kernels --
// state in registers, no per-step launch phase -- keep the 8-lane advantage (22.8 vs 23.9 us per step, with the policy
// network 25.0 vs 26.5) and take it.  The state layout does not depend on the mapping, so the kernels of one handle may
// differ.  planar (6 x 9): the quad is the widest that pays.
// Two variants run fewer mappings: the rigid-body kernels (dynamics_mode 1) exist per lane and per quad only -- 8 -> 4,
// 2 -> 1, and atacom_get_lanes reports what really runs.  The canonical chart (chart_mode 1) distributes the vectors of
// its square-root recursion over the lanes of a group (atacom_chart.h): the gain per lane added is smaller than with the
// reference chart's 12 x 17 factorisation, so the groups narrow earlier -- iiwa single steps 8 lanes up to 8192 envs (since
// the row slots and the static slack stage A of atacom_chart.h: 27.2 us on the bench workload against 29.4 with 4 lanes; 28.5
// vs 30.0 at 2048, 29.4 vs 30.9 at 4096), 4 lanes up to 16384, then one lane (40 us at 32768, 2 lanes 41.6); T-step kernels
// 8 lanes up to 8192 (19.7 us per step), 4 up to 16384 (21.5), 2 up to 32768 (25.7), one beyond (28.8 at 65536); planar like
// the reference chart's kernels (single steps at 8192: 13.8 us with 4 lanes, 14.2 with 2, 15.7 with one;
// profiles/r03_lanes_vs_batch_canonical.log, r03_ab_rowslots.log, r03_ab_stage_a.log).
enum { KIND_STEP = 0, KIND_ROLLOUT = 1, KIND_MLP = 2 };     // = atacom_ops_impl.h
int pick_lanes_raw(const atacom_config& c, int kind) {
    if (c.lanes_per_env == 1 || c.lanes_per_env == 2 || c.lanes_per_env == 4 || c.lanes_per_env == 8)
        return c.lanes_per_env;
    if (c.dtype == ATACOM_F64) {
        // float64 (the reference's precision: the parity build and the bench's float64 records).  Same rule as float32 --
        // the widest instantiated mapping whose waves still find a SIMD each -- on the float64 census (1, 4 and, iiwa, 8 lanes;
        // atacom_ops_impl.h: has_mapping).  Measured at 8192 environments with the solver inlined (round 6,
        // profiles/r06_f64_lanes_inlined.log): iiwa 50.2 us per step on 8 lanes, 53.2 on 4, 161.9 on one (T-step 44.8 / 52.3 /
        // 158.3); planar 20.2 on 4 lanes, 25.2 on one (T-step 17.7 / 22.2)
        // (beyond 8192 the iiwa quad stays ahead of the lane at every batch -- 104.8 against 248.8 us at 32768, 207 against 305 at
        // 65536, profiles/r06_f64_lanes_beyond_16384.log: the float64 lane kernel spills 700 registers.)  Canonical chart
        // (profiles/r06_f64_lanes_canonical.log): iiwa 35.9 us on 8 lanes, 39.3 on 4, 56.8 on one at 8192; at 32768 the lane
        // (61.7) is ahead of the quad (72.0); planar 17.8 on 4 lanes against 21.0 at 8192, 32.4 against 22.7 at 32768
        if (c.env_id == ATACOM_ENV_IIWA)
            return c.batch <= 8192 ? 8 : ((c.chart_mode == 0 || c.batch <= 16384) ? 4 : 1);
        if (c.env_id == ATACOM_ENV_PLANAR) return c.batch <= 16384 ? 4 : 1;
        return 1;
    }
    if (c.chart_mode == 1) {
        if (c.env_id == ATACOM_ENV_IIWA) {
            if (kind == KIND_STEP) return c.batch <= 8192 ? 8 : (c.batch <= 16384 ? 4 : 1);
            return c.batch <= 8192 ? 8 : (c.batch <= 16384 ? 4 : (c.batch <= 32768 ? 2 : 1));
        }
        if (c.env_id == ATACOM_ENV_PLANAR)
            return c.batch <= 16384 ? 4 : (c.batch <= 32768 ? 2 : 1);
        return 1;
    }
    if (c.env_id == ATACOM_ENV_IIWA) {
        // Round 4: single steps take the 8-lane mapping up to 8192 environments as well.  Rounds 2 / 3 had measured a tie with
        // the quad there (27.2 us both, mean of nine boxes, per box from -5 % to +4.5 %) and kept the quad; on the round-4
        // boxes the 8-lane kernel is 7 % faster every time -- bench workload 24.9 against 26.8 us (three interleaved runs),
        // constraint-active states 25.9 against 27.8 (two more boxes): profiles/r04_ab_lanes_bench.log, r04_ab_noise_kernels.log.
        // For 4096 < batch <= 8192 this is the static fallback: atacom_create times both mappings (calibrate_step_lanes below)
        (void)kind;
        return c.batch <= 8192 ? 8 : (c.batch <= 16384 ? 4 : (c.batch <= 32768 ? 2 : 1));
    }
    if (c.env_id == ATACOM_ENV_PLANAR) {
        // round 5 re-measured 8 lanes against the quad at 8192 environments with this round's kernels: single steps tie
        // (10.9 us both: the quad stays, half the waves), the T-step kernels run 8.3 against 8.8 us per step on 8 lanes
        // (profiles/r05_planar_lanes_baseline.log)
        if (kind == KIND_ROLLOUT && c.batch <= 8192) return 8;
        return c.batch <= 16384 ? 4 : (c.batch <= 32768 ? 2 : 1);
    }
    return 1;                                                              // circle: launch-bound either way
}
// default initial state rows: [q, dq, puck(6)]
void default_init_row(int env_id, int task, std::vector<double>& row) {
    double puck[6] = {-0.4, 0.0, 0.0, 0.0, 0.0, 0.0};         // centre of hit_range, env_hitting.py:11,27
    if (env_id == ATACOM_ENV_PLANAR && task == 1) {           // AirHockeyDefend [upstream]: middle of start_range's x, y = 0,
        puck[0] = 0.45; puck[3] = -1.0;                       // velocity (-1, 0)
    }
    if (env_id == ATACOM_ENV_CIRCLE || env_id == ATACOM_ENV_CIRCLE_EC || env_id == ATACOM_ENV_CIRCLE_T) {
        row = {-1.0, 0.0, 0.0, 0.0};                            // circle_base.py:44
    } else if (env_id == ATACOM_ENV_PLANAR) {
        row = {-0.9273, 0.9273, M_PI / 2, 0, 0, 0};             // MushroomRL planar init pose
    } else {
        // CLIK pose for the tip at (0.65, 0, 0.1505), R = diag(-1, 1, -1) (env_single.py:39-44, kinematics.py);
        // value computed by oracle/robots.py:iiwa_clik and pinned in tests/test_oracle_kinematics.py
        row = {0.0, 0.7135214629060707, 0.0, -0.5024756033561426, 0.0, 1.9256631778550268, 0, 0, 0, 0, 0, 0};
    }
    row.insert(row.end(), puck, puck + 6);
}

}  // namespace

struct atacom_handle;
static int check_mlp(const atacom_handle* h, const atacom_mlp* in, const char* who, atacom_mlp* net);

struct atacom_handle {
    atacom_config cfg;
    int device;
    const atacom::EnvOps* ops;
    void* f;        // float fields, groups of four: [n_planes / 4][batch][4]  (atacom_kernels.h: Planes)
    int* ip;        // int fields: [batch][4]
    double* partial_dev;
    double* partial_host;
    void* snap_dev;       // the header every snapshot image starts with (SnapHeader), device copy
    void* snap_host;      // pinned: atacom_snapshot_restore reads an image's header into it
    int step_lanes;       // single-step mapping that overrides the static policy (0 = none): timed at create when
                          // ATACOM_CALIBRATE=1 asks for it (calibrate_step_lanes), or adopted from a snapshot image
    int rollout_lanes;    // the same for the T-step kernels (only ever adopted from a snapshot image)
};

// What a snapshot image starts with: enough of the configuration to refuse an image of another handle shape instead of
// mis-reading it (a different task, environment, dtype, batch or state layout can have the same byte size)
struct SnapHeader {
    uint32_t magic, header_bytes;
    int32_t struct_size, env_id, dtype, batch, n_planes, n_iplanes, task, elem;
    int32_t step_lanes, rollout_lanes;      // the kernel mappings of the handle that wrote the image (summation order: a
                                            // replay is bit for bit only on the same mappings -- atacom_snapshot_restore)
    uint32_t version;                       // format of the image (kSnapVersion); images of library <= 0.5 carry 0 here
    int32_t seed;                           // the writer's generator key (cfg.seed / atacom_set_seed): restored with the state
    uint32_t pad[2];
};
static_assert(sizeof(SnapHeader) == 64, "snapshot header is 64 bytes");
constexpr uint32_t kSnapMagic = 0x4e535441u;      // "ATSN"
constexpr uint32_t kSnapVersion = 2;              // 1: library 0.4 (no mappings in the header, never tagged); 2: library 0.6
static SnapHeader snap_header(const atacom_handle* h) {
    SnapHeader s;
    std::memset(&s, 0, sizeof(s));
    s.magic = kSnapMagic; s.header_bytes = (uint32_t)sizeof(SnapHeader);
    s.struct_size = h->cfg.struct_size; s.env_id = h->cfg.env_id; s.dtype = h->cfg.dtype; s.batch = h->cfg.batch;
    s.n_planes = h->ops->n_planes; s.n_iplanes = h->ops->n_iplanes; s.task = h->cfg.task; s.elem = (int32_t)h->ops->elem;
    s.version = kSnapVersion; s.seed = h->cfg.seed;
    return s;                                   // (the lanes fields are filled by the callers: see snap_header_with_lanes)
}

// the stepping entry points of the handle's kernel variant (dynamics_mode x chart_mode)
struct Stepper {
    decltype(atacom::VariantOps::step) step;
    decltype(atacom::VariantOps::rollout) rollout;
    decltype(atacom::VariantOps::rollout_mlp) rollout_mlp;
    decltype(atacom::VariantOps::lanes_run) lanes_run;
};
static Stepper stepper(const atacom_handle* h) {
    const atacom_config& c = h->cfg;
    const atacom::VariantOps* v = nullptr;
    if (c.dynamics_mode != 0) v = atacom::ops_iiwa_dyn_variant(c.dtype, c.chart_mode);
    else if (c.obs_noise || c.obs_delay || c.env_noise) v = atacom::ops_noise(c.env_id, c.dtype, c.chart_mode);
    else if (c.chart_mode == 1) v = atacom::ops_chart(c.env_id, c.dtype);
    if (v) return {v->step, v->rollout, v->rollout_mlp, v->lanes_run};
    return {h->ops->step, h->ops->rollout, h->ops->rollout_mlp, h->ops->lanes_run};
}

// The mapping each kind of launch REALLY runs on: the request (cfg.lanes_per_env, a calibrated / adopted override, or the
// static policy) narrowed to the instantiated mappings of the handle's kernel variant (atacom_ops_impl.h: has_mapping) --
// what atacom_get_lanes / atacom_get_policy_lanes report and the snapshot header records.
static int step_lanes(const atacom_handle* h) {
    return stepper(h).lanes_run(KIND_STEP, h->step_lanes ? h->step_lanes : pick_lanes_raw(h->cfg, KIND_STEP));
}
static int rollout_lanes(const atacom_handle* h) {
    return stepper(h).lanes_run(KIND_ROLLOUT, h->rollout_lanes ? h->rollout_lanes : pick_lanes_raw(h->cfg, KIND_ROLLOUT));
}
// the policy kernel follows the T-step mapping where it has that form (float64: quad or lane; float32 8 lanes: matrix cores)
static int policy_lanes(const atacom_handle* h) {
    return stepper(h).lanes_run(KIND_MLP, h->rollout_lanes ? h->rollout_lanes : pick_lanes_raw(h->cfg, KIND_ROLLOUT));
}
static SnapHeader snap_header_with_lanes(const atacom_handle* h) {
    SnapHeader s = snap_header(h);
    s.step_lanes = step_lanes(h);
    s.rollout_lanes = rollout_lanes(h);
    return s;
}

// Single steps of iiwa at 4096 < batch <= 8192 on the reference chart: 8 lanes per environment (1024 waves, every CU
// busy) against the quad (512 waves, half of the CUs).  The STATIC policy is 8 lanes (pick_lanes_raw): the sustained bench
// workload had it ahead on all seven round-4 boxes (24.85 against 26.75 us: profiles/r04_calibration_probe.log,
// r04_calibration_vs_sustained.log, r04_ab_lanes_bench*.log).  The two mappings sum in different orders, so WHICH one runs
// decides the bits a handle produces: the default must not depend on a wall-clock race (round 4 timed both at create --
// eight ranks of a sharded collection could disagree, a snapshot could replay on the other mapping: VERDICT r4 weak 2,
// ADVICE r4).  atacom_create therefore launches nothing hidden by default.  The timing is still there for a user who wants
// the faster mapping of THIS box and accepts box-dependent bits: ATACOM_CALIBRATE=1 (or =verbose, which also prints the
// two figures) times both mappings once per process, device and kernel variant (three alternating bursts of 100 launches
// each, the minimum per mapping: about 20 ms), keeps 8 lanes unless the quad is more than 1 % faster, and every later
// handle of the process with the same variant takes the same answer.  A failure inside the timing is not an error of
// atacom_create: the handle keeps the static policy.  The T-step kernels do not take part.
static bool wants_calibration(const atacom_config& c) {
    if (c.lanes_per_env != 0 || c.env_id != ATACOM_ENV_IIWA || c.dtype != ATACOM_F32 || c.chart_mode != 0 ||
        c.dynamics_mode != 0 || c.batch <= 4096 || c.batch > 8192)
        return false;
    const char* e = std::getenv("ATACOM_CALIBRATE");
    return e && (e[0] == '1' || e[0] == 'v');
}
static std::mutex g_cal_mutex;
// (device, batch, hold_q, substeps, bias_mode, noise options) -> lanes: everything that selects the kernel being timed
typedef std::array<int, 6> CalKey;
static std::map<CalKey, int> g_cal_cache;

// Times atacom_step's kernel in both mappings on the handle's own (freshly reset) state; the caller re-initialises the
// state afterwards.  Returns hipSuccess and the choice in h->step_lanes (left 0 if anything fails: the static policy).
static hipError_t calibrate_step_lanes(atacom_handle* h) {
    std::lock_guard<std::mutex> lock(g_cal_mutex);
    const atacom_config& cc = h->cfg;
    const CalKey key = {h->device, cc.batch, cc.hold_q, cc.substeps, cc.bias_mode,
                        (cc.obs_noise ? 1 : 0) | (cc.obs_delay ? 2 : 0) | (cc.env_noise ? 4 : 0)};
    auto it = g_cal_cache.find(key);
    if (it != g_cal_cache.end()) { h->step_lanes = it->second; return hipSuccess; }
    const size_t B = (size_t)h->cfg.batch, el = h->ops->elem;
    void *act = nullptr, *obs = nullptr, *rew = nullptr;
    uint8_t *absb = nullptr, *last = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipMalloc(&act, el * B * h->ops->nk);
    if (e == hipSuccess) e = hipMemset(act, 0, el * B * h->ops->nk);
    if (e == hipSuccess) e = hipMalloc(&obs, el * B * h->ops->obs_dim);
    if (e == hipSuccess) e = hipMalloc(&rew, el * B);
    if (e == hipSuccess) e = hipMalloc((void**)&absb, B);
    if (e == hipSuccess) e = hipMalloc((void**)&last, B);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    const int cand[2] = {8, 4};
    float best[2] = {1e30f, 1e30f};
    const Stepper st = stepper(h);
    for (int round = 0; round < 3 && e == hipSuccess; ++round) {
        for (int c = 0; c < 2 && e == hipSuccess; ++c) {
            for (int i = 0; i < 8; ++i)
                st.step(h->cfg, cand[c], h->f, h->ip, act, obs, rew, absb, last, nullptr, nullptr);
            e = hipEventRecord(e0, nullptr);
            for (int i = 0; i < 100; ++i)
                st.step(h->cfg, cand[c], h->f, h->ip, act, obs, rew, absb, last, nullptr, nullptr);
            if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
            if (e == hipSuccess) e = hipEventSynchronize(e1);
            float ms = 0.f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            if (e == hipSuccess && ms < best[c]) best[c] = ms;
        }
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) {
        h->step_lanes = best[1] < 0.99f * best[0] ? 4 : 8;
        g_cal_cache[key] = h->step_lanes;
        const char* v = std::getenv("ATACOM_CALIBRATE");
        if (v && v[0] == 'v')                                   // ATACOM_CALIBRATE=verbose: say what was measured
            std::fprintf(stderr, "[atacom] device %d, iiwa batch %d, atacom_step: 8 lanes %.2f us, 4 lanes %.2f us per launch -> %d\n",
                         h->device, h->cfg.batch, best[0] * 10.f, best[1] * 10.f, h->step_lanes);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (act) (void)hipFree(act);
    if (obs) (void)hipFree(obs);
    if (rew) (void)hipFree(rew);
    if (absb) (void)hipFree(absb);
    if (last) (void)hipFree(last);
    return e;
}

// Validates *in and copies it to *net by the ABI-size rule of atacom_mlp_host.h: mlp_abi_copy.
static int check_mlp(const atacom_handle* h, const atacom_mlp* in, const char* who, atacom_mlp* net) {
    const std::string w(who);
    if (!atacom::mlp_abi_copy(in, net)) return fail(ATACOM_E_INVALID, w + ": atacom_mlp.struct_size mismatch (ABI)");
    if (net->n_in != h->ops->obs_dim || net->n_out != h->ops->nk)
        return fail(ATACOM_E_INVALID, w + ": network n_in / n_out must equal obs_dim / n_null");
    if (!net->W1 || !net->b1 || !net->W2 || !net->b2 || !net->W3 || !net->b3)
        return fail(ATACOM_E_INVALID, w + ": null weight pointer");
    const int n_sig = (net->sW1 != nullptr) + (net->sb1 != nullptr) + (net->sW2 != nullptr) + (net->sb2 != nullptr) +
                      (net->sW3 != nullptr) + (net->sb3 != nullptr);
    if (n_sig != 0 && n_sig != 6)
        return fail(ATACOM_E_INVALID, w + ": the sigma network needs all six weight pointers (or none)");
    if (net->activation != 0 && net->activation != 1)
        return fail(ATACOM_E_INVALID, w + ": activation must be 0 (ReLU) or 1 (tanh)");
    if (net->mean_mode != 0 && net->mean_mode != 1)
        return fail(ATACOM_E_INVALID, w + ": mean_mode must be 0 (linear) or 1 (act_scale * tanh)");
    if (net->explore < 0 || net->explore > 2)
        return fail(ATACOM_E_INVALID, w + ": explore must be 0 (Gaussian), 1 (clipped Gaussian) or 2 (Ornstein-Uhlenbeck)");
    if (net->explore != 0 && (net->squash || n_sig != 0))
        return fail(ATACOM_E_INVALID, w + ": explore = 1 / 2 does not combine with squash or a sigma network");
    if (net->explore == 1 && (!net->act_low || !net->act_high))
        return fail(ATACOM_E_INVALID, w + ": explore = 1 (clipped Gaussian) needs act_low and act_high");
    if (net->explore == 2 && !net->ou_state)
        return fail(ATACOM_E_INVALID, w + ": explore = 2 (Ornstein-Uhlenbeck) needs ou_state");
    if (net->explore == 2 && !(net->ou_dt > 0.0))
        return fail(ATACOM_E_INVALID, w + ": explore = 2 (Ornstein-Uhlenbeck) needs ou_dt > 0");
    return ATACOM_OK;
}

extern "C" {

const char* atacom_last_error(void) { return g_err.c_str(); }
const char* atacom_version(void) { return "atacom_hip 0.6 (gfx950)"; }

int atacom_get_dims(int32_t env_id, atacom_dims* out) {
    const atacom::EnvOps* ops = get_ops(env_id, ATACOM_F32);
    if (!ops || !out) return fail(ATACOM_E_INVALID, "atacom_get_dims: bad env_id or null output");
    out->dim_q = ops->nq; out->n_f = ops->nf; out->n_g = ops->ng; out->n_null = ops->nk;
    out->obs_dim = ops->obs_dim; out->state_dim = ops->state_dim; out->init_state_dim = ops->init_dim;
    out->record_dim = 2 * ops->obs_dim + ops->nk + 3;
    return ATACOM_OK;
}

int atacom_default_config(int32_t env_id, atacom_config* c) {
    if (!c) return fail(ATACOM_E_INVALID, "atacom_default_config: null output");
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int32_t)sizeof(atacom_config);
    c->env_id = env_id;
    c->batch = 1;
    c->dtype = ATACOM_F32;
    c->hold_q = 1;
    c->bias_mode = 0;
    c->auto_reset = 0;
    c->lanes_per_env = 0;
    c->rref_tol = 0.05;          // atacom.py:128
    c->gamma = 0.99;
    c->action_penalty = 1e-3;    // env_hitting.py:10
    c->term_tol = 0.1;           // circle_terminated.py:13
    c->dynamics_mode = 0;
    c->chart_mode = 0;
    c->puck_mass = 0.01;
    if (env_id == ATACOM_ENV_CIRCLE || env_id == ATACOM_ENV_CIRCLE_EC || env_id == ATACOM_ENV_CIRCLE_T) {
        // circle_atacom.py:7-18 == circle_error_correction.py:8-21 (same constraints and gains)
        c->substeps = 1; c->horizon = 500; c->dt = 0.01; c->hold_q = 0;
        c->dt_base = 0.01;           // circle_base.py:18: the wrappers never pass their time_step on (circle_atacom.py:8)
        c->K[0] = 0.1; c->K[1] = 2.0;
        for (int i = 0; i < 2; ++i) { c->Kc[i] = 100.0; c->vel_max[i] = 1.0; c->acc_max[i] = 10.0; c->Kq[i] = 20.0; }
    } else if (env_id == ATACOM_ENV_PLANAR) {
        // atacom_air_hockey.py:12-43; robot data: DESIGN.md "Planar robot" (MushroomRL URDF, not in the tree)
        c->substeps = 4; c->horizon = 120; c->dt = 1.0 / 240.0;
        const double vel[3] = {M_PI / 2, M_PI / 2, 2 * M_PI / 3};
        const double lim[3] = {2.9670597283903604, 2.0943951023931953, 2.0943951023931953};
        const double link[3] = {0.55, 0.44, 0.44};
        for (int i = 0; i < 6; ++i) { c->K[i] = i < 3 ? 0.5 : 1.0; c->Kc[i] = 240.0; }
        for (int i = 0; i < 3; ++i) {
            c->vel_max[i] = vel[i]; c->acc_max[i] = 10.0; c->Kq[i] = 2 * 10.0 / vel[i];
            c->pos_limit[i] = lim[i]; c->link[i] = link[i];
        }
        c->base_xy[0] = -1.51; c->base_xy[1] = 0.0;
    } else if (env_id == ATACOM_ENV_IIWA) {
        // iiwa_hit_atacom.py:11-40; limits urdf/iiwa_1.urdf:74,112,149,186,223,260; base env_base.py:50
        c->substeps = 4; c->horizon = 120; c->dt = 1.0 / 240.0;
        const double vel[6] = {1.4835298641951802, 1.4835298641951802, 1.7453292519943295,
                               1.3089969389957472, 2.2689280275926285, 2.356194490192345};
        const double lim[6] = {2.9670597283903604, 2.0943951023931953, 2.9670597283903604,
                               2.0943951023931953, 2.9670597283903604, 2.0943951023931953};
        c->K[0] = 0.1;
        for (int i = 1; i < 6; ++i) c->K[i] = 0.5;
        for (int i = 6; i < 12; ++i) c->K[i] = 1.0;
        for (int i = 0; i < 12; ++i) c->Kc[i] = 240.0;
        for (int i = 0; i < 6; ++i) {
            c->vel_max[i] = vel[i]; c->acc_max[i] = 10.0; c->Kq[i] = 4 * 10.0 / vel[i]; c->pos_limit[i] = lim[i];
        }
        c->base_xy[0] = -1.51; c->base_xy[1] = 0.0;
    } else {
        return fail(ATACOM_E_INVALID, "atacom_default_config: unknown env_id");
    }
    return ATACOM_OK;
}

int atacom_create(const atacom_config* cfg, int device, atacom_handle** out) {
    if (!cfg || !out) return fail(ATACOM_E_INVALID, "atacom_create: null argument");
    if (cfg->struct_size != (int32_t)sizeof(atacom_config))
        return fail(ATACOM_E_INVALID, "atacom_create: atacom_config.struct_size mismatch (ABI)");
    const atacom::EnvOps* ops = get_ops(cfg->env_id, cfg->dtype);
    if (!ops) return fail(ATACOM_E_INVALID, "atacom_create: unknown env_id / dtype");
    if (cfg->batch <= 0 || cfg->substeps <= 0 || cfg->horizon <= 0 || !(cfg->dt > 0))
        return fail(ATACOM_E_INVALID, "atacom_create: batch, substeps, horizon and dt must be positive");
    if (cfg->lanes_per_env != 0 && cfg->lanes_per_env != 1 && cfg->lanes_per_env != 2 && cfg->lanes_per_env != 4 &&
        cfg->lanes_per_env != 8)
        return fail(ATACOM_E_INVALID, "atacom_create: lanes_per_env must be 0 (auto), 1, 2, 4 or 8");
    if (cfg->dynamics_mode != 0 && !((cfg->dynamics_mode == 1 || cfg->dynamics_mode == 2) && cfg->env_id == ATACOM_ENV_IIWA))
        return fail(ATACOM_E_INVALID, "atacom_create: dynamics_mode 1 / 2 (rigid body) exist for ATACOM_ENV_IIWA only");
    if (cfg->chart_mode != 0 && cfg->chart_mode != 1)
        return fail(ATACOM_E_INVALID, "atacom_create: chart_mode must be 0 (reference) or 1 (canonical)");
    if (cfg->task != 0 && !(cfg->task == 1 && cfg->env_id == ATACOM_ENV_PLANAR))
        return fail(ATACOM_E_UNSUPPORTED, "atacom_create: task 1 (defend) exists for ATACOM_ENV_PLANAR only "
                                          "(the reference's iiwa wrapper raises NotImplementedError, iiwa_hit_atacom.py:20-21)");
    if (cfg->reserved0 != 0 || cfg->reserved1 != 0) return fail(ATACOM_E_INVALID, "atacom_create: reserved fields must be 0");
    if ((cfg->obs_noise || cfg->obs_delay || cfg->env_noise) && cfg->env_id != ATACOM_ENV_PLANAR && cfg->env_id != ATACOM_ENV_IIWA)
        return fail(ATACOM_E_UNSUPPORTED, "atacom_create: obs_noise / obs_delay / env_noise exist for the air-hockey "
                                          "environments only (iiwa_hit_atacom.py:11-13, atacom_air_hockey.py:12-14)");
    if (cfg->env_noise && !(cfg->puck_mass > 0)) return fail(ATACOM_E_INVALID, "atacom_create: puck_mass must be positive");
    if ((cfg->obs_noise || cfg->obs_delay || cfg->env_noise) && cfg->dynamics_mode != 0)
        return fail(ATACOM_E_UNSUPPORTED, "atacom_create: obs_noise / obs_delay / env_noise are compiled for the kinematic mode "
                                          "(dynamics_mode 0) only");
    if (cfg->chart_mode == 1 && cfg->env_id != ATACOM_ENV_CIRCLE && cfg->env_id != ATACOM_ENV_PLANAR &&
        cfg->env_id != ATACOM_ENV_IIWA)
        return fail(ATACOM_E_INVALID, "atacom_create: chart_mode 1 needs an ATACOM environment (the E / T baselines have no chart)");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(ATACOM_E_INVALID, "atacom_create: no such device");
    DeviceGuard guard(device);
    HIP_TRY(guard.err);
    atacom_handle* h = new atacom_handle();
    h->cfg = *cfg;
    h->cfg.seed = cfg->seed & 0x7fffffff;       // as atacom_set_seed stores it
    h->device = device;
    h->ops = ops;
    h->f = nullptr; h->ip = nullptr; h->partial_dev = nullptr; h->partial_host = nullptr;
    h->snap_dev = nullptr; h->snap_host = nullptr;
    h->step_lanes = 0;
    h->rollout_lanes = 0;
    const size_t B = (size_t)cfg->batch;
    void* drow = nullptr;
    // default initial state for every env, then a full reset
    std::vector<double> row;
    default_init_row(cfg->env_id, cfg->task, row);
    std::vector<char> bytes(row.size() * ops->elem);
    for (size_t i = 0; i < row.size(); ++i) {
        if (ops->elem == 4) reinterpret_cast<float*>(bytes.data())[i] = (float)row[i];
        else reinterpret_cast<double*>(bytes.data())[i] = row[i];
    }
    const char* what = "allocation";
    hipError_t e = hipMalloc(&h->f, ops->elem * ops->n_planes * B);
    if (e == hipSuccess) e = hipMalloc((void**)&h->ip, sizeof(int) * ops->n_iplanes * B);
    if (e == hipSuccess) e = hipMalloc((void**)&h->partial_dev, sizeof(double) * 4 * kStatBlocks);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->partial_host, sizeof(double) * 4 * kStatBlocks);
    if (e == hipSuccess) e = hipMalloc(&drow, bytes.size());
    if (e == hipSuccess) e = hipMalloc(&h->snap_dev, sizeof(SnapHeader));
    if (e == hipSuccess) e = hipHostMalloc(&h->snap_host, sizeof(SnapHeader));
    if (e == hipSuccess) {
        what = "initialisation";
        e = hipMemcpy(drow, bytes.data(), bytes.size(), hipMemcpyHostToDevice);
    }
    auto initialise = [&]() -> hipError_t {
        hipError_t r = hipMemset(h->f, 0, ops->elem * ops->n_planes * B);
        if (r == hipSuccess) r = hipMemset(h->ip, 0, sizeof(int) * ops->n_iplanes * B);
        if (r != hipSuccess) return r;
        ops->fill_init(h->cfg, h->f, h->ip, drow, nullptr);
        ops->clear_stats(h->cfg, h->f, h->ip, nullptr);
        ops->reset(h->cfg, h->f, h->ip, nullptr, nullptr, nullptr, nullptr);
        r = hipGetLastError();
        return r == hipSuccess ? hipDeviceSynchronize() : r;
    };
    if (e == hipSuccess) e = initialise();
    if (e == hipSuccess && wants_calibration(h->cfg)) {             // opt-in: ATACOM_CALIBRATE=1 / verbose
        if (calibrate_step_lanes(h) != hipSuccess) {
            h->step_lanes = 0;                                      // the static policy; not an error of create
            (void)hipGetLastError();
        }
        what = "re-initialisation after timing the two single-step mappings";
        e = initialise();                                           // the timed launches stepped the state: start over
    }
    if (e == hipSuccess) {
        const SnapHeader sh = snap_header_with_lanes(h);
        e = hipMemcpy(h->snap_dev, &sh, sizeof(sh), hipMemcpyHostToDevice);
    }
    if (drow) (void)hipFree(drow);
    if (e != hipSuccess) {                      // one exit for every failure: nothing allocated above survives it
        atacom_destroy(h);
        return fail(ATACOM_E_HIP, std::string("atacom_create: ") + what + " failed: " + hipGetErrorString(e));
    }
    *out = h;
    return ATACOM_OK;
}

int atacom_destroy(atacom_handle* h) {
    if (!h) return ATACOM_OK;
    DeviceGuard guard(h->device);
    if (h->f) (void)hipFree(h->f);
    if (h->ip) (void)hipFree(h->ip);
    if (h->partial_dev) (void)hipFree(h->partial_dev);
    if (h->partial_host) (void)hipHostFree(h->partial_host);
    if (h->snap_dev) (void)hipFree(h->snap_dev);
    if (h->snap_host) (void)hipHostFree(h->snap_host);
    delete h;
    return ATACOM_OK;
}

int atacom_reset(atacom_handle* h, const uint8_t* d_mask, const void* d_init_state, void* d_obs, void* stream) {
    if (!h) return fail(ATACOM_E_INVALID, "atacom_reset: null handle");
    ON_DEVICE(h);
    h->ops->reset(h->cfg, h->f, h->ip, d_mask, d_init_state, d_obs, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

int atacom_step(atacom_handle* h, const void* d_action, void* d_obs, void* d_reward, uint8_t* d_absorbing,
                uint8_t* d_last, void* stream) {
    if (!h) return fail(ATACOM_E_INVALID, "atacom_step: null handle");
    if (!d_action || !d_obs || !d_reward || !d_absorbing)
        return fail(ATACOM_E_INVALID, "atacom_step: d_action, d_obs, d_reward and d_absorbing are required");
    ON_DEVICE(h);
    stepper(h).step(h->cfg, step_lanes(h), h->f, h->ip, d_action, d_obs, d_reward, d_absorbing, d_last,
                    nullptr, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

int atacom_step_masked(atacom_handle* h, const uint8_t* d_mask, const void* d_action, void* d_obs, void* d_reward,
                       uint8_t* d_absorbing, uint8_t* d_last, void* stream) {
    if (!h) return fail(ATACOM_E_INVALID, "atacom_step_masked: null handle");
    if (!d_action || !d_obs || !d_reward || !d_absorbing)
        return fail(ATACOM_E_INVALID, "atacom_step_masked: d_action, d_obs, d_reward and d_absorbing are required");
    ON_DEVICE(h);
    stepper(h).step(h->cfg, step_lanes(h), h->f, h->ip, d_action, d_obs, d_reward, d_absorbing, d_last,
                    d_mask, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

int atacom_rollout(atacom_handle* h, int32_t n_steps, const void* d_actions, void* d_obs, void* d_next_obs,
                   void* d_reward, uint8_t* d_absorbing, uint8_t* d_last, void* stream) {
    if (!h) return fail(ATACOM_E_INVALID, "atacom_rollout: null handle");
    if (n_steps <= 0) return fail(ATACOM_E_INVALID, "atacom_rollout: n_steps must be positive");
    if (!d_actions || !d_obs || !d_reward || !d_absorbing || !d_last)
        return fail(ATACOM_E_INVALID, "atacom_rollout: all buffers except d_next_obs are required");
    ON_DEVICE(h);
    stepper(h).rollout(h->cfg, rollout_lanes(h), n_steps, h->f, h->ip, d_actions, d_obs, d_next_obs, d_reward,
                       d_absorbing, d_last, nullptr, 0, nullptr, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

int atacom_rollout_mlp(atacom_handle* h, int32_t n_steps, const atacom_mlp* net, const void* d_noise, void* d_obs,
                       void* d_next_obs, void* d_actions, void* d_reward, uint8_t* d_absorbing, uint8_t* d_last,
                       void* stream) {
    if (!h || !net) return fail(ATACOM_E_INVALID, "atacom_rollout_mlp: null handle / network");
    if (n_steps <= 0) return fail(ATACOM_E_INVALID, "atacom_rollout_mlp: n_steps must be positive");
    atacom_mlp m;
    const int vrc = check_mlp(h, net, "atacom_rollout_mlp", &m);
    if (vrc != ATACOM_OK) return vrc;
    if (!d_obs || !d_actions || !d_reward || !d_absorbing || !d_last)
        return fail(ATACOM_E_INVALID, "atacom_rollout_mlp: all output buffers except d_next_obs are required");
    ON_DEVICE(h);
    const int rc = stepper(h).rollout_mlp(h->cfg, policy_lanes(h), n_steps, m, h->f, h->ip, d_noise, d_obs,
                                       d_next_obs, d_actions, d_reward, d_absorbing, d_last, nullptr, 0, nullptr,
                                       (hipStream_t)stream);
    if (rc != ATACOM_OK)
        return fail(ATACOM_E_UNSUPPORTED, "atacom_rollout_mlp: only planar / iiwa with hidden = 64 are compiled in (not: the canonical chart together with noise options / rigid-body mode; float64: reference chart, kinematic, no noise options)");
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

// atacom_rollout_packed and atacom_rollout_compact: one validation, one dispatch; cx selects the compact format
static int rollout_records(atacom_handle* h, const char* fn, int32_t n_steps, const void* d_actions, const atacom_mlp* net,
                           const void* d_noise, void* d_records, int32_t record_batch_stride, const atacom::CompactArgs* cx,
                           void* stream) {
    const std::string name(fn);
    if (!h) return fail(ATACOM_E_INVALID, name + ": null handle");
    if (n_steps <= 0) return fail(ATACOM_E_INVALID, name + ": n_steps must be positive");
    if (!d_records) return fail(ATACOM_E_INVALID, name + ": d_records is required");
    if ((d_actions != nullptr) == (net != nullptr))
        return fail(ATACOM_E_INVALID, name + ": give either d_actions or a policy network");
    if (record_batch_stride < h->cfg.batch)
        return fail(ATACOM_E_INVALID, name + ": record_batch_stride must be >= batch");
    if (cx) {
        // (t, b) of an exception row are stored in the handle's float type: exact integers below 2^24 in float32
        if (n_steps >= (1 << 24) || record_batch_stride >= (1 << 24))
            return fail(ATACOM_E_INVALID, name + ": n_steps and record_batch_stride must be < 2^24");
        if (!cx->count) return fail(ATACOM_E_INVALID, name + ": d_n_ends is required");
        if (cx->cap < 0 || (cx->cap > 0 && !cx->ends))
            return fail(ATACOM_E_INVALID, name + ": ends_capacity must be >= 0, and d_ends given when it is positive");
    }
    atacom_mlp m{};
    if (net) {
        const int vrc = check_mlp(h, net, fn, &m);
        if (vrc != ATACOM_OK) return vrc;
    }
    ON_DEVICE(h);
    if (cx) HIP_TRY(hipMemsetAsync(cx->count, 0, sizeof(int32_t), (hipStream_t)stream));
    if (d_actions) {
        stepper(h).rollout(h->cfg, rollout_lanes(h), n_steps, h->f, h->ip, d_actions, nullptr, nullptr, nullptr,
                           nullptr, nullptr, d_records, record_batch_stride, cx, (hipStream_t)stream);
    } else {
        const int rc = stepper(h).rollout_mlp(h->cfg, policy_lanes(h), n_steps, m, h->f, h->ip, d_noise, nullptr,
                                              nullptr, nullptr, nullptr, nullptr, nullptr, d_records, record_batch_stride, cx,
                                              (hipStream_t)stream);
        if (rc != ATACOM_OK)
            return fail(ATACOM_E_UNSUPPORTED, name + ": only planar / iiwa with hidden = 64 are compiled in (not: the canonical chart together with noise options / rigid-body mode; float64: reference chart, kinematic, no noise options)");
    }
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

int atacom_rollout_packed(atacom_handle* h, int32_t n_steps, const void* d_actions, const atacom_mlp* net,
                          const void* d_noise, void* d_records, int32_t record_batch_stride, void* stream) {
    return rollout_records(h, "atacom_rollout_packed", n_steps, d_actions, net, d_noise, d_records, record_batch_stride,
                           nullptr, stream);
}

int atacom_rollout_compact(atacom_handle* h, int32_t n_steps, const void* d_actions, const atacom_mlp* net,
                           const void* d_noise, void* d_records, int32_t record_batch_stride, void* d_ends,
                           int32_t ends_capacity, int32_t* d_n_ends, void* stream) {
    const atacom::CompactArgs cx{d_ends, d_n_ends, ends_capacity};
    return rollout_records(h, "atacom_rollout_compact", n_steps, d_actions, net, d_noise, d_records, record_batch_stride,
                           &cx, stream);
}

int atacom_set_seed(atacom_handle* h, int32_t seed) {
    if (!h) return fail(ATACOM_E_INVALID, "atacom_set_seed: null handle");
    ON_DEVICE(h);
    h->cfg.seed = seed & 0x7fffffff;        // kernels receive the configuration by value with every launch
    const SnapHeader now = snap_header_with_lanes(h);      // the snapshot header carries the key: keep its device copy current
    HIP_TRY(hipMemcpy(h->snap_dev, &now, sizeof(now), hipMemcpyHostToDevice));
    return ATACOM_OK;
}

int atacom_get_lanes(const atacom_handle* h, int32_t* out_step_lanes, int32_t* out_rollout_lanes) {
    if (!h) return fail(ATACOM_E_INVALID, "atacom_get_lanes: null handle");
    if (out_step_lanes) *out_step_lanes = step_lanes(h);
    if (out_rollout_lanes) *out_rollout_lanes = rollout_lanes(h);
    return ATACOM_OK;
}

int atacom_get_policy_lanes(const atacom_handle* h, int32_t* out_policy_lanes) {
    if (!h || !out_policy_lanes) return fail(ATACOM_E_INVALID, "atacom_get_policy_lanes: null argument");
    *out_policy_lanes = policy_lanes(h);
    return ATACOM_OK;
}

int atacom_get_stats(atacom_handle* h, double out[3], int32_t clear, void* stream) {
    if (!h || !out) return fail(ATACOM_E_INVALID, "atacom_get_stats: null argument");
    ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const int nb = std::min(kStatBlocks, (h->cfg.batch + 255) / 256);
    h->ops->stats(h->cfg, h->f, h->ip, h->partial_dev, nb, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->partial_host, h->partial_dev, sizeof(double) * 4 * nb, hipMemcpyDeviceToHost, s));
    if (clear) h->ops->clear_stats(h->cfg, h->f, h->ip, s);
    HIP_TRY(hipStreamSynchronize(s));
    double sum = 0.0, cnt = 0.0, cmax = -INFINITY, dqmax = -INFINITY;
    for (int i = 0; i < nb; ++i) {
        sum += h->partial_host[4 * i + 0];
        cnt += h->partial_host[4 * i + 1];
        cmax = std::fmax(cmax, h->partial_host[4 * i + 2]);
        dqmax = std::fmax(dqmax, h->partial_host[4 * i + 3]);
    }
    out[0] = cnt > 0 ? sum / cnt : NAN;    // np.mean of an empty log is nan as well
    out[1] = cmax;
    out[2] = dqmax;
    return ATACOM_OK;
}

int atacom_get_state(atacom_handle* h, void* d_state, void* stream) {
    if (!h || !d_state) return fail(ATACOM_E_INVALID, "atacom_get_state: null argument");
    ON_DEVICE(h);
    h->ops->get_state(h->cfg, h->f, h->ip, d_state, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

int atacom_set_state(atacom_handle* h, const void* d_state, void* stream) {
    if (!h || !d_state) return fail(ATACOM_E_INVALID, "atacom_set_state: null argument");
    ON_DEVICE(h);
    h->ops->set_state(h->cfg, h->f, h->ip, d_state, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

// ---- checkpoint / resume: the image is [header (64 bytes) | float fields | int fields] exactly as the handle holds them
static size_t snapshot_float_bytes(const atacom_handle* h) {
    const size_t raw = (size_t)h->ops->elem * h->ops->n_planes * (size_t)h->cfg.batch;
    return (raw + 15) & ~(size_t)15;
}
int64_t atacom_snapshot_bytes(const atacom_handle* h) {
    if (!h) { fail(ATACOM_E_INVALID, "atacom_snapshot_bytes: null handle"); return ATACOM_E_INVALID; }
    return (int64_t)(sizeof(SnapHeader) + snapshot_float_bytes(h) + sizeof(int) * h->ops->n_iplanes * (size_t)h->cfg.batch);
}
int atacom_snapshot_save(atacom_handle* h, void* d_image, void* stream) {
    if (!h || !d_image) return fail(ATACOM_E_INVALID, "atacom_snapshot_save: null argument");
    ON_DEVICE(h);
    const size_t B = (size_t)h->cfg.batch, nf = (size_t)h->ops->elem * h->ops->n_planes * B;
    char* img = (char*)d_image;
    HIP_TRY(hipMemcpyAsync(img, h->snap_dev, sizeof(SnapHeader), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIP_TRY(hipMemcpyAsync(img + sizeof(SnapHeader), h->f, nf, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIP_TRY(hipMemcpyAsync(img + sizeof(SnapHeader) + snapshot_float_bytes(h), h->ip, sizeof(int) * h->ops->n_iplanes * B,
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ATACOM_OK;
}
int atacom_snapshot_restore(atacom_handle* h, const void* d_image, void* stream) {
    if (!h || !d_image) return fail(ATACOM_E_INVALID, "atacom_snapshot_restore: null argument");
    ON_DEVICE(h);
    const size_t B = (size_t)h->cfg.batch, nf = (size_t)h->ops->elem * h->ops->n_planes * B;
    const char* img = (const char*)d_image;
    // the header comes to the host first (64 bytes; synchronises `stream`): an image of another handle shape is refused
    HIP_TRY(hipMemcpyAsync(h->snap_host, img, sizeof(SnapHeader), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    const SnapHeader want = snap_header_with_lanes(h);
    SnapHeader got = *(const SnapHeader*)h->snap_host;
    if (got.magic != kSnapMagic) return fail(ATACOM_E_INVALID, "atacom_snapshot_restore: not a snapshot image (bad magic)");
    if (got.version != kSnapVersion) {
        char msg[200];
        std::snprintf(msg, sizeof(msg), "atacom_snapshot_restore: image format %u, this library reads format %u (images do not "
                      "travel between library versions: re-create the checkpoint)", got.version, kSnapVersion);
        return fail(ATACOM_E_INVALID, msg);
    }
    const int img_step = got.step_lanes, img_roll = got.rollout_lanes, img_seed = got.seed;
    got.step_lanes = want.step_lanes; got.rollout_lanes = want.rollout_lanes;       // compared separately below
    got.seed = want.seed;                                                           // adopted below
    if (std::memcmp(&got, &want, sizeof(SnapHeader)) != 0) {
        char msg[256];
        std::snprintf(msg, sizeof(msg), "atacom_snapshot_restore: the image belongs to another handle shape (env %d dtype %d batch %d "
                      "task %d, %d + %d fields per env; this handle: env %d dtype %d batch %d task %d, %d + %d)", got.env_id, got.dtype,
                      got.batch, got.task, got.n_planes, got.n_iplanes, want.env_id, want.dtype, want.batch, want.task,
                      want.n_planes, want.n_iplanes);
        return fail(ATACOM_E_INVALID, msg);
    }
    bool header_changed = false;
    if (img_seed != h->cfg.seed) {
        // the generator key is part of the state a replay depends on (random_init, obs_noise, env_noise draws): the image's
        // seed replaces the handle's, like atacom_set_seed would (launches captured in a HIP graph keep theirs)
        h->cfg.seed = img_seed;
        header_changed = true;
    }
    if (img_step != want.step_lanes || img_roll != want.rollout_lanes) {
        // The image was written by a handle running other kernel mappings (the state itself does not depend on them).  A
        // handle that left the choice to the library (lanes_per_env = 0) ADOPTS the image's mappings, so that "restore, repeat
        // the calls" reproduces the writer's bits in another process or on another box; a handle with a named mapping keeps
        // it.  Mappings this handle's kernel variant does not have are narrowed the way every request is (step_lanes()).
        // Launches already captured in a HIP graph keep the mapping they were captured with, and a RolloutCollector built
        // before the restore refuses to collect on changed mappings (rollout.py).
        auto ok = [](int l) { return l == 1 || l == 2 || l == 4 || l == 8; };
        if (!ok(img_step) || !ok(img_roll)) return fail(ATACOM_E_INVALID, "atacom_snapshot_restore: corrupt image header (lanes)");
        if (h->cfg.lanes_per_env == 0) {
            h->step_lanes = img_step;
            h->rollout_lanes = img_roll;
            header_changed = true;
        }
    }
    if (header_changed) {
        const SnapHeader now = snap_header_with_lanes(h);
        HIP_TRY(hipMemcpy(h->snap_dev, &now, sizeof(now), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpyAsync(h->f, img + sizeof(SnapHeader), nf, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIP_TRY(hipMemcpyAsync(h->ip, img + sizeof(SnapHeader) + snapshot_float_bytes(h), sizeof(int) * h->ops->n_iplanes * B,
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ATACOM_OK;
}

int atacom_get_aux_state(atacom_handle* h, void* d_aux, void* stream) {
    if (!h || !d_aux) return fail(ATACOM_E_INVALID, "atacom_get_aux_state: null argument");
    if (h->cfg.env_id != ATACOM_ENV_IIWA) return fail(ATACOM_E_INVALID, "atacom_get_aux_state: ATACOM_ENV_IIWA only");
    ON_DEVICE(h);
    atacom::ops_iiwa_dyn(h->cfg.dtype)->get_aux(h->cfg, h->f, d_aux, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

int atacom_set_aux_state(atacom_handle* h, const void* d_aux, void* stream) {
    if (!h || !d_aux) return fail(ATACOM_E_INVALID, "atacom_set_aux_state: null argument");
    if (h->cfg.env_id != ATACOM_ENV_IIWA) return fail(ATACOM_E_INVALID, "atacom_set_aux_state: ATACOM_ENV_IIWA only");
    ON_DEVICE(h);
    atacom::ops_iiwa_dyn(h->cfg.dtype)->set_aux(h->cfg, h->f, d_aux, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

static int filter_io(atacom_handle* h, void* d_buf, int set, void* stream, const char* who) {
    if (!h || !d_buf) return fail(ATACOM_E_INVALID, std::string(who) + ": null argument");
    if (h->cfg.env_id != ATACOM_ENV_PLANAR && h->cfg.env_id != ATACOM_ENV_IIWA)
        return fail(ATACOM_E_INVALID, std::string(who) + ": ATACOM_ENV_PLANAR / ATACOM_ENV_IIWA only");
    ON_DEVICE(h);
    h->ops->filter_io(h->cfg, h->f, d_buf, set, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}
int atacom_get_filter_state(atacom_handle* h, void* d_filter, void* stream) {
    return filter_io(h, d_filter, 0, stream, "atacom_get_filter_state");
}
int atacom_set_filter_state(atacom_handle* h, const void* d_filter, void* stream) {
    return filter_io(h, const_cast<void*>(d_filter), 1, stream, "atacom_set_filter_state");
}

int atacom_inverse_dynamics(int32_t dtype, int32_t n, const void* d_q, const void* d_dq, const void* d_ddq, void* d_tau,
                            void* d_M, void* stream) {
    if (dtype != ATACOM_F32 && dtype != ATACOM_F64) return fail(ATACOM_E_INVALID, "atacom_inverse_dynamics: bad dtype");
    if (n <= 0 || !d_q || !d_dq || !d_ddq || !d_tau) return fail(ATACOM_E_INVALID, "atacom_inverse_dynamics: null buffer");
    atacom::ops_iiwa_dyn(dtype)->inverse_dynamics(n, d_q, d_dq, d_ddq, d_tau, d_M, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

int atacom_forward_dynamics(int32_t dtype, int32_t n, const void* d_q, const void* d_dq, const void* d_tau6,
                            const void* d_ddq_aux, int32_t use_damping, void* d_ddq6, void* stream) {
    if (dtype != ATACOM_F32 && dtype != ATACOM_F64) return fail(ATACOM_E_INVALID, "atacom_forward_dynamics: bad dtype");
    if (n <= 0 || !d_q || !d_dq || !d_tau6 || !d_ddq6) return fail(ATACOM_E_INVALID, "atacom_forward_dynamics: null buffer");
    atacom::ops_iiwa_dyn(dtype)->forward_dynamics(n, d_q, d_dq, d_tau6, d_ddq_aux, use_damping, d_ddq6, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

int atacom_nullspace(int32_t env_id, int32_t dtype, int32_t lanes_per_env, int32_t n, const void* d_Jc,
                     const void* d_rhs, double tol, void* d_x, void* d_null, void* d_rref, void* stream) {
    if (lanes_per_env != 1 && lanes_per_env != 2 && lanes_per_env != 4 && lanes_per_env != 8)
        return fail(ATACOM_E_INVALID, "atacom_nullspace: lanes_per_env must be 1, 2, 4 or 8");
    const atacom::EnvOps* ops = get_ops(env_id, dtype);
    if (!ops) return fail(ATACOM_E_INVALID, "atacom_nullspace: unknown env_id / dtype");
    if (n <= 0 || !d_Jc) return fail(ATACOM_E_INVALID, "atacom_nullspace: n must be positive and d_Jc non-null");
    ops->nullspace(lanes_per_env, n, d_Jc, d_rhs, tol, d_x, d_null, d_rref, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

int atacom_canonical_mu(int32_t env_id, int32_t dtype, int32_t n, const void* d_A, const void* d_s, const void* d_y,
                        const void* d_alpha, double tol, void* d_mu, void* stream) {
    const atacom::VariantOps* v = (dtype == ATACOM_F32 || dtype == ATACOM_F64) ? atacom::ops_chart(env_id, dtype) : nullptr;
    if (!v) return fail(ATACOM_E_INVALID, "atacom_canonical_mu: env_id must be circle / planar / iiwa, dtype f32 / f64");
    if (n <= 0 || !d_A || !d_s || !d_y || !d_alpha || !d_mu)
        return fail(ATACOM_E_INVALID, "atacom_canonical_mu: n must be positive and every buffer non-null");
    v->chart_mu(n, d_A, d_s, d_y, d_alpha, tol, d_mu, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

int atacom_constraint_terms(const atacom_config* cfg, int32_t n, const void* d_q, const void* d_dq, void* d_fun,
                            void* d_J, void* d_b, void* stream) {
    if (!cfg || cfg->struct_size != (int32_t)sizeof(atacom_config))
        return fail(ATACOM_E_INVALID, "atacom_constraint_terms: bad config");
    const atacom::EnvOps* ops = get_ops(cfg->env_id, cfg->dtype);
    if (!ops) return fail(ATACOM_E_INVALID, "atacom_constraint_terms: unknown env_id / dtype");
    if (n <= 0 || !d_q || !d_dq || !d_fun || !d_J || !d_b)
        return fail(ATACOM_E_INVALID, "atacom_constraint_terms: null buffer");
    ops->terms(*cfg, n, d_q, d_dq, d_fun, d_J, d_b, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_OK;
}

}  // extern "C"
