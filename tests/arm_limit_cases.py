"""Limit-binding inputs for the arm tests (CPU and GPU): states of the planar and the iiwa task in which the joint-position
limits, the velocity bounds of `acc_truncation` and the 1.5 vel_max clamp of the integrator BIND, built on the CPU from the
float64 oracle (oracle/atacom_batched.py) alone and deterministic in the seed.

The states every other parity test draws (reset pose +- 0.05 rad, or tests/chart_cases.away_init_q, free-running under random
actions) come no closer than 0.03 rad to a joint limit, stay below vel_max, and never reach the nested saturation of the
velocity bound or the clamp.  Here:

  pushed states   start at chart_cases.init_q(name, ., sigma = 0.05); every environment holds ONE random sign vector in
                  {-1, +1}^n_null as its action for P steps, P in PUSH_STEPS by (candidate index mod 4), no resets: what the
                  closed loop produces at the boundaries -- small slacks on table, link-height and joint-limit rows, violated
                  rows (fun > 0), a positive constraint log, speeds at the bound.
  over-speed      one candidate in four (one of every P class: candidate index mod 16 in OVERSPEED_RESIDUES) gets one random
                  joint's velocity overwritten with +-U(0.9, 1.7) vel_max_j, s left as it is: reachable only through
                  set_state, and the only way to the nested saturation (up = lo = -+acc_max once |dq| > vel_max + acc_max / Kq)
                  and to the 1.5 vel_max clamp in kinematic mode.
  rejection       2 B candidates, the first B eligible ones are kept.  Not eligible: a non-finite state, min |s| < 1e-9
                  (exact zeros: the reference's answer there is set by an rcond, tests/point_reach_cases.py), max |s| > 100
                  (an s that came within 1e-6 of zero is thrown to 1e4 .. 1e8 by the slack rate ~ c / s: the argument of
                  point_reach_cases.fixture_states).
  window          T teacher-forced steps; even environments keep their sign vector, odd ones draw U(-1.3, 1.3) per step.

The iiwa set is built separately per chart (the pushed trajectories differ).  tests/test_arm_limit_cases_oracle.py holds the
sets to their purpose and every ceiling below against the oracle alone; tests/test_gpu_arm_limits.py runs them on the device.
"""
import numpy as np

import parity_tools
from chart_cases import SPECS, init_q
from oracle import atacom_batched as ob

SETS = {'planar': ('planar', 0), 'iiwa_reference': ('iiwa', 0), 'iiwa_canonical': ('iiwa', 1)}
CHART_NAMES = {0: 'reference', 1: 'canonical'}
B_LIMITS = {'planar': 512, 'iiwa_reference': 384, 'iiwa_canonical': 384}
B_RAGGED = 257                               # the T-step kernel cases run the first 257: a partial wave, a partial 8-lane group
T_LIMITS = {'planar': 8, 'iiwa_reference': 4, 'iiwa_canonical': 4}
# seeds picked on the census alone (the iiwa sets: of 80 .. 95 the ones with the most joint-limit rows whose smallest |s| is
# under 1e-3 and the most first-sub-step clamp samples: the two figures that move with the seed at this size)
SEEDS = {'planar': 61, 'iiwa_reference': 94, 'iiwa_canonical': 82}
PUSH_STEPS = (20, 40, 70, 100)
OVERSPEED_RESIDUES = (0, 5, 10, 15)          # candidate index mod 16: one candidate in four, one of every P class
S_MIN, S_MAX = 1e-9, 100.0

# Ceilings held against the oracle alone (tests/test_arm_limit_cases_oracle.py): the share measured on these inputs -- the
# larger of all B environments and the first B_RAGGED -- x 1.25, rounded up to the next 0.5 %.  The iiwa reference chart's
# is capped at 50 %: beyond that the float32 rule says too little to be worth a test.
#   MAX_VACUOUS: share of samples whose float32 bound C sens + floor exceeds parity_tools.VACUOUS
#                measured planar 3.125 %, iiwa reference 47.96 % (x 1.25 = 59.9 %: capped), iiwa canonical 10.70 %
#   MAX_LOOSE64: share of samples whose float64 allowance C sens exceeds F64_BOUND itself
#                measured planar 0.632 %, iiwa reference 9.922 %, iiwa canonical 11.19 %
MAX_VACUOUS = {'planar': 0.04, 'iiwa_reference': 0.50, 'iiwa_canonical': 0.135}
MAX_LOOSE64 = {'planar': 0.01, 'iiwa_reference': 0.125, 'iiwa_canonical': 0.14}
# What census() must find (tests/test_arm_limit_cases_oracle.py): half of what it measures on these inputs (in brackets:
# planar / iiwa reference / iiwa canonical), and never below the floor the purpose of the set asks for.
CENSUS_MIN = {
    'truncation': {'planar': 969, 'iiwa_reference': 627, 'iiwa_canonical': 721},     # the rarest class: [1938 / 1254 / 1443]
    'truncation_floor': 100,                                                         # joint-sub-steps in EVERY class
    'nested_saturation': {'planar': 3, 'iiwa_reference': 18, 'iiwa_canonical': 10},  # [6 / 36 / 20]
    'clamp_samples': {'planar': 20, 'iiwa_reference': 20, 'iiwa_canonical': 20},     # [25 / 30 / 29]: the floor of 20 binds
    'task_rows': {'planar': 1, 'iiwa_reference': 2, 'iiwa_canonical': 2},            # rows with min |s| < 1e-3 [3 / 5 / 5]
    'limit_rows': {'planar': 1, 'iiwa_reference': 2, 'iiwa_canonical': 2},           # [2 / 3 / 4]: iiwa's floor of 2 binds
    'violated_share': {'planar': 0.045, 'iiwa_reference': 0.120, 'iiwa_canonical': 0.107},   # [9.03 % / 24.15 % / 21.55 %]
    'fast_share': {'planar': 0.052, 'iiwa_reference': 0.05, 'iiwa_canonical': 0.05},  # [10.52 % / 8.83 % / 9.16 %]: floor 5 %
    'log_c_max': {'planar': 0.49, 'iiwa_reference': 0.42, 'iiwa_canonical': 0.44},    # [0.9876 / 0.8579 / 0.8859]
}

# the float64 rule of tests/test_gpu_arm_limits.py: err <= F64_BOUND + C_SENS r, r = the oracle's own response to relative
# perturbations of (q, dq, s, puck, action) at F64_QUICK_SCALES (parity_tools.QUICK_SCALES x eps64 / eps32 = 1.9e-9, widened
# 1000 x to stand clear of the oracle's own rounding noise at 1e-16), deep probe at F64_DEEP_SCALES; no J_c noise
F64_BOUND = 1e-8
F64_QUICK_SCALES = (2.5e-13, 1e-12, 4e-12)
F64_DEEP_SCALES = (1e-12, 4e-12, 1.6e-11)


def spec_of(key):
    name, chart = SETS[key]
    spec = SPECS[name]()
    spec.chart_mode = chart
    return name, spec


def _copy_rows(dst, src, rows_dst):
    """Every per-environment array of the oracle env `src` (its batch = len(rows_dst)) into those rows of `dst`."""
    for k, v in src.__dict__.items():
        if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == src.B:
            getattr(dst, k)[rows_dst] = v


def pushed_oracle(key, B=None, seed=None):
    """(o, sign): a BatchedAtacomEnv of B limit-binding environments (module docstring) with a cleared constraint log, and
    the sign vector [B, n_null] every environment was pushed with.  o.push_steps [B] and o.overspeed [B] (the joint whose
    velocity was overwritten, -1: none) say how each environment was made."""
    name, spec = spec_of(key)
    seed = SEEDS[key] if seed is None else seed
    B = B_LIMITS[key] if B is None else B
    rng = np.random.default_rng(seed)
    C = 2 * B
    k, nq = spec.n_null, spec.dim_q
    sign = rng.choice([-1.0, 1.0], (C, k))
    P = np.array(PUSH_STEPS)[np.arange(C) % len(PUSH_STEPS)]
    o = ob.BatchedAtacomEnv(spec, C, init_q=init_q(name, C, rng, sigma=0.05))
    over = np.isin(np.arange(C) % 16, OVERSPEED_RESIDUES)
    joint = rng.integers(0, nq, C)
    mag = rng.uniform(0.9, 1.7, C) * rng.choice([-1.0, 1.0], C)
    final = parity_tools.slice_env(o, np.arange(C))
    ok = np.zeros(C, dtype=bool)
    # every draw above is made for all 2 B candidates; the candidates themselves are independent environments, so the first B
    # are pushed together and the rest in blocks of B / 8 only while fewer than B are eligible: the first B eligible
    # candidates of the 2 B, at little more than half the cost (measured: at most one candidate of a set is rejected)
    step = max(B // 8, 1)
    for block in [np.arange(B)] + [np.arange(a, min(a + step, C)) for a in range(B, C, step)]:
        run, rows, done = parity_tools.slice_env(o, block), block, 0
        with np.errstate(all='ignore'):                  # a candidate may leave the finite numbers: it is rejected below
            for p in PUSH_STEPS:
                for _ in range(p - done):
                    run.step(sign[rows])
                done = p
                here = P[rows] == p
                _copy_rows(final, parity_tools.slice_env(run, np.flatnonzero(here)), rows[here])
                run, rows = parity_tools.slice_env(run, np.flatnonzero(~here)), rows[~here]
        assert len(rows) == 0
        ov = block[over[block]]
        final.dq[ov, joint[ov]] = mag[ov] * spec.vel_max[joint[ov]]
        f = parity_tools.slice_env(final, block)
        s_abs = np.abs(f.s)
        with np.errstate(all='ignore'):
            ok[block] = (np.isfinite(f.q).all(1) & np.isfinite(f.dq).all(1) & np.isfinite(f.s).all(1)
                         & np.isfinite(f.puck).all(1) & np.isfinite(f.r_hit) & np.isfinite(f.vel_hit_x)
                         & (s_abs.min(1) >= S_MIN) & (s_abs.max(1) <= S_MAX))
        if ok.sum() >= B:
            break
    keep = np.flatnonzero(ok)[:B]
    assert len(keep) == B, 'only %d of %d candidates are eligible' % (len(keep), C)
    out = parity_tools.slice_env(final, keep)
    out.env_index = np.arange(B)
    out.push_steps = P[keep]
    out.overspeed = np.where(over, joint, -1)[keep]
    out.rejected = int(keep[-1] + 1 - B)                 # candidates passed over before the B-th eligible one
    out.get_constraints_logs()
    return out, sign[keep]


def forced_inputs(key, sign, seed=None, T=None):
    """The actions [T, B, n_null] of the teacher-forced window: even environments keep their sign vector, odd ones draw
    U(-1.3, 1.3) per step."""
    seed = SEEDS[key] if seed is None else seed
    T = T_LIMITS[key] if T is None else T
    B, k = sign.shape
    acts = np.stack([np.random.default_rng([seed + 100, t]).uniform(-1.3, 1.3, (B, k)) for t in range(T)])   # step t's draws
    acts[:, 0::2] = sign[0::2]                                                          # do not depend on T
    return acts


def step_outputs(p, inputs):
    """What is compared per sample (tests/test_gpu_parity._step_outputs): observation, s, reward, the absorbing flag."""
    oo, orr, oab, _ = p.step(inputs[0])
    return np.concatenate([oo, p.s, orr[:, None], oab[:, None].astype(np.float64)], 1)


TRUNCATION_CLASSES = ('none', 'acc_hi', 'acc_lo', 'vel_upper', 'vel_lower')


def truncation_class(spec, dq, ddq):
    """Per joint, the branch of acc_truncation (atacom_batched.BatchedAtacomEnv.acc_truncation) the demanded ddq takes:
    0 none, 1 clipped at +acc_max, 2 clipped at -acc_max, 3 clipped at the velocity bound's upper limit
    up = -Kq (dq - vel_max) < acc_max, 4 at its lower limit lo = -Kq (dq + vel_max) > -acc_max -- and whether that bound is
    itself saturated at the opposite acceleration limit (nested: up = -acc_max or lo = +acc_max)."""
    up = np.maximum(np.minimum(spec.acc_max, -spec.Kq * (dq - spec.vel_max)), -spec.acc_max)
    lo = np.minimum(np.maximum(-spec.acc_max, -spec.Kq * (dq + spec.vel_max)), spec.acc_max)
    hi, low = ddq > up, ddq < lo
    cls = np.where(hi, np.where(up >= spec.acc_max, 1, 3), np.where(low, np.where(lo <= -spec.acc_max, 2, 4), 0))
    nested = (hi & (up <= -spec.acc_max)) | (low & (lo >= spec.acc_max))
    return cls, nested


def census(o, actions):
    """What the inputs of a teacher-forced test exercise: `o` (left untouched) is stepped through actions [T, B, k]; the
    counts are over the T x B samples (the state BEFORE each step is the sample's input) and, for the truncation classes,
    over their T x B x substeps x dim_q joint-sub-steps."""
    p = parity_tools.slice_env(o, np.arange(o.B))
    sp = p.spec
    nf, nq = sp.n_f, sp.dim_q
    classes, nested = np.zeros(len(TRUNCATION_CLASSES), dtype=np.int64), [0]
    inner = p.acc_truncation

    def counted(dq, ddq):
        c, n = truncation_class(sp, dq, ddq)
        classes[:] += np.bincount(c.ravel(), minlength=len(classes))
        nested[0] += int(n.sum())
        return inner(dq, ddq)
    p.acc_truncation = counted
    smin, violated, clamp, fast = [], [], [], []
    for a in actions:
        fun, _, _ = ob.constraint_terms(sp, p.q, p.dq)
        smin.append(np.abs(p.s))
        violated.append((fun[:, nf:] > 0).any(1))
        clamp.append((np.abs(p.dq) > 1.5 * sp.vel_max + sp.acc_max * sp.dt).any(1))
        fast.append(np.abs(p.dq) > 0.97 * sp.vel_max)
        p.step(a)
    smin = np.array(smin).reshape(-1, sp.n_g)
    log = p.get_constraints_logs()
    n_task = sp.n_g - nq                                  # table / link-height rows come first, the joint-limit rows last
    row_min, row_share = smin.min(0), (smin < 0.05).mean(0)
    return {'samples': len(smin), 'joint_substeps': int(classes.sum()),
            'row_min_abs_s': row_min.tolist(), 'row_share_abs_s_below_0.05': row_share.tolist(),
            'task_rows_min_abs_s_below_1e-3': int((row_min[:n_task] < 1e-3).sum()),
            'limit_rows_min_abs_s_below_1e-3': int((row_min[n_task:] < 1e-3).sum()),
            'violated_share': float(np.mean(violated)),
            'truncation': dict(zip(TRUNCATION_CLASSES, classes.tolist())), 'nested_saturation': nested[0],
            'clamp_samples': int(np.sum(clamp)), 'fast_share': float(np.mean(fast)),
            'log_c_avg': log[0], 'log_c_max': log[1], 'log_dq_max': log[2]}


_PREPARED = {}


def prepared(key):
    """The oracle side of the teacher-forced window of one set, computed once per process and shared by every test and
    kernel mapping: dict(spec, o = the pushed oracle env (untouched), sign, acts [T, B, k], rec32 / rec64 = the recorders of
    the float32 / the float64 rule with every step of the window prepared (rec.snaps[t] = the state before step t, rec.base[t]
    = the oracle's outputs), log = the oracle's constraint log over the window)."""
    if key not in _PREPARED:
        o, sign = pushed_oracle(key)
        acts = forced_inputs(key, sign)
        rec32 = recorder32(seed=5)
        rec64 = recorder64(seed=6)
        p = parity_tools.slice_env(o, np.arange(o.B))
        for a in acts:
            rec64.prepare(p, (a,), base=rec32.prepare(p, (a,)))
            p.step(a)
        _PREPARED[key] = {'spec': o.spec, 'o': o, 'sign': sign, 'acts': acts, 'rec32': rec32, 'rec64': rec64,
                          'log': p.get_constraints_logs()}
    return _PREPARED[key]


# The reproduction audit of finish() on these states (REPRO_ERR, REPRO_GAIN, MAX_UNREPRODUCED as they are) with wider DRAWS:
# the deep scales start at 1e-6, and every draw adds unstructured noise to J_c.  Here the oracle moves by 1 .. 17 (relative)
# under such perturbations on the samples where errors of 1e-3 occur (sens of the iiwa reference-chart samples involved:
# 1.8e-3 .. 17), so 48 draws at >= 1e-6 land nowhere near ANY given point within 2e-3 of the unperturbed oracle, the device's
# result included (closest perturbed oracle 0.2 .. 0.4 away from a device that is 2e-3 off).  The audit therefore draws at
# the quick AND the deep scales (2e-7 .. 1.6e-5), 64 times per scale, with and without the J_c noise (structured
# perturbations: J_c's zeros stay exact, as they do on a device).  Measured on the CPU against recorded float32 device
# outputs of the iiwa reference-chart window (profiles/arm_limits.md): the closest perturbed oracle is then 7 to 200 times
# nearer to the device than the unperturbed oracle on 3 .. 7 of the 3 .. 7 errors above 1e-3 per mapping but at most one,
# while the deliberately wrong oracles of tests/test_arm_limit_cases_oracle.py stay unreproduced.
REPRO_SCALES = parity_tools.QUICK_SCALES + parity_tools.DEEP_SCALES[2:]
REPRO_DRAWS = 64


ARM_FIELDS = ('q', 'dq', 's', 'puck')           # the state the probes perturb (SensitivityRecorder's own default)


def recorder32(step_fn=step_outputs, seed=5, state_fields=ARM_FIELDS):
    """A recorder of the float32 rule, its constants unchanged, with the wider audit draws above.  state_fields: the state
    the probes perturb (tests/rigid_limit_cases.py adds the servo joints' qx, dqx)."""
    return parity_tools.SensitivityRecorder(step_fn, seed=seed, state_fields=state_fields, stacked_draws=True,
                                            repro_scales=REPRO_SCALES, repro_draws=REPRO_DRAWS, repro_structured=True)


def recorder64(step_fn=step_outputs, seed=6, state_fields=ARM_FIELDS):
    """A recorder of the float64 rule (module constants above)."""
    return parity_tools.SensitivityRecorder(step_fn, seed=seed, state_fields=state_fields, quick_scales=F64_QUICK_SCALES,
                                            deep_scales=F64_DEEP_SCALES, floor=F64_BOUND, jc_noise=False, stacked_draws=True)


def shares(p, n=None):
    """(vacuous share of the float32 bound, loose share of the float64 allowance) of a prepared set from the quick probes
    alone, over its first n environments (None: all)."""
    S32, S64 = np.array(p['rec32'].sens)[:, :n], np.array(p['rec64'].sens)[:, :n]
    return (float(np.mean(parity_tools.C_SENS * S32 + parity_tools.FLOOR > parity_tools.VACUOUS)),
            float(np.mean(parity_tools.C_SENS * S64 > F64_BOUND)))


# ------------------------------------------------------------------------------------------------ the policy-kernel case
POLICY_NETS = {'planar': ('sac_planar', 'tanh'), 'iiwa_reference': ('ppo_iiwa', 'relu')}
POLICY_STEPS = (0, 1)                        # the window's states the policy kernel is started from (0: the clamp samples)


def policy_parts(key):
    """(weights [W1, b1, W2, b2, W3, b3], obs_shift, obs_scale, activation) of the golden actor network of the policy case
    (tests/golden/policy_net.npz), the observation normalisation drawn as tests/test_gpu_parity._policy_pair draws it."""
    import os
    net, activation = POLICY_NETS[key]
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'policy_net.npz'))
    W = [g[net + '._h%d.%s' % (i, w)] for i in (1, 2, 3) for w in ('weight', 'bias')]
    rng = np.random.default_rng(3)
    n_in = W[0].shape[1]
    return W, rng.uniform(-0.5, 0.5, n_in), rng.uniform(0.5, 2.0, n_in), activation


def oracle_policy(key):
    from oracle.policy import MlpPolicy
    W, shift, scale, activation = policy_parts(key)
    return MlpPolicy(*W, obs_shift=shift, obs_scale=scale, activation=activation)
