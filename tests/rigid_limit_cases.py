"""Saturating inputs for the rigid-body step of the iiwa task (dynamics_mode 'rigid_body' = 1, 'rigid_body_ff' = 2): states
in which the servo motor limit (with its floor at 0), the six arm effort limits and the integrator's 1.5 vel_max clamp BIND,
built on the CPU from the float64 oracle (oracle/atacom_batched.py, oracle/dynamics.py) alone and deterministic in the seed.

The closed loop never gets there (measured on the inputs of test_gpu_dynamics.test_rigid_body_env_step_against_oracle, 8192
env-sub-steps per mode: the servo velocity set-point clips, the motor limit, its floor and all six arm clips bind 0 times;
with M_ss = 0.002 .. 0.004 the motor limit is 2500 .. 10000 rad/s^2): these saturations bind only from servo speeds put in
through set_state / set_aux_state.  Here:

  arm state    by environment index mod 8 -- 0, 1, 2, 4, 5, 6: the reset pose + N(0, 0.05 rad), at rest (what test_gpu_dynamics
               draws: the bound of the float32 rule says most there); 3: a pushed state of arm_limit_cases.pushed_oracle for
               the same chart (one in four of those over-speed); 7: the reset pose with one random joint's velocity
               overwritten with +-U(0.9, 1.7) vel_max_j, s left as it is -- so that |dq| feeds h and the clamp is met in
               this mode as well.
  servo state  qx = U(-1, 1) rad; dqx = U(-1, 1) x DQX_CLASSES[environment index mod 3] rad/s: within the servo's own speed
               limit / where the motor limit binds / where Coriolis and centrifugal terms of the striker reach the arm's
               effort limits and |h_s| the servo's (the floor).  3 and 8 are coprime: every wave and every quad of lanes
               holds every combination.
  eligibility  the rules of arm_limit_cases.pushed_oracle (finite, S_MIN <= |s| <= S_MAX), asserted on every environment.
  window       T = 2 teacher-forced steps, actions U(-1.3, 1.3): step 0 carries the binding sub-steps, step 1 is the state
               just after saturation with the servo joints at +-1.5 v_max.

The four sets are {reference, canonical} chart x {mode 1, mode 2}; the two modes of a chart share their states.

What the float32 allowance must see in this mode.  Where no clip binds, rhs = tau - h cancels an h of up to a few hundred Nm
down to M ddq of a few Nm: perturbing the INPUT state moves h in tau and in rhs together, so the recorder's probes do not see
the cancellation -- the device's float32 rounding of h and M does (ulp32(300 Nm) / lambda_min(M_aa) x dt is of order 1e-4
rad/s).  Every probe of the float32 rule therefore also draws DYNAMICS NOISE (the analogue of the recorder's J_c noise):
relative perturbations at the probe's own scale of h and of the mass-matrix entries, independently at each use (the motor
limit, the torque, the right-hand side, the solve) -- rigid_substep(noise=).  Its response enters sens like any other draw;
C_SENS, FLOOR, VACUOUS and the audit constants stand.  The float64 rule is that of tests/test_gpu_arm_limits.py (no noise).

Joints 1 and 2 (320 Nm).  The fastest servo class reaches joint 1 at both signs (12 .. 17 counted env-sub-steps per set)
and joint 2 at -320 Nm (8 .. 12; asserted on the reference-chart sets, where the count stands clear of the floor of 8).  Joint
2's clip at +320 Nm is NOT reached: the largest tau found before the clip is +300.6 Nm (reference chart, mode 1) .. +353.7 Nm
(canonical chart, mode 2: one env-sub-step above the limit) against -538 Nm at the other sign; servo speeds beyond
200 rad/s were not tried for it.  It is the only min / max of rigid_body_substep these sets leave unexercised.

tests/test_rigid_limit_cases_oracle.py holds the sets to their purpose and every ceiling below against the oracle alone;
tests/test_gpu_rigid_limits.py runs them on the device.
"""
import time

import numpy as np

import arm_limit_cases as alc
import parity_tools
from chart_cases import init_q
from oracle import atacom_batched as ob
from oracle import atacom_scalar as osc
from oracle import dynamics as D
from oracle import robots

MODES = {1: 'rigid_body', 2: 'rigid_body_ff'}
CHARTS = {'reference': 0, 'canonical': 1}
SETS = {'%s_m%d' % (c, m): (c, m) for c in CHARTS for m in MODES}            # key -> (chart, dynamics_mode)
B_RIGID = 256
B_RAGGED = 197                               # the T-step kernel cases run the first 197: a partial wave with either mapping
T_RIGID = 2
SEED = 31
FIELDS = ('q', 'dq', 's', 'puck', 'qx', 'dqx')
DQX_CLASSES = np.array([[3.5, 4.7, 4.7], [60.0, 30.0, 30.0], [200.0, 120.0, 120.0]])     # rad/s, by environment index mod 3
PUSHED_RESIDUE, OVERSPEED_RESIDUE = 3, 7     # environment index mod 8
SERVO_VMAX = 1.5 * np.array([robots.IIWA_VEL_LIMIT[6], 3.1415926, 3.1415926])

# Ceilings held against the oracle alone (tests/test_rigid_limit_cases_oracle.py), the rule of arm_limit_cases: the share
# measured on these inputs -- the larger of all B environments and the first B_RAGGED -- x 1.25, rounded up to the next
# 0.5 %; the reference chart's float32 ceiling is capped at 50 %.
#   MAX_VACUOUS: share of samples whose float32 bound C sens + floor exceeds parity_tools.VACUOUS; measured reference
#                41.12 % (x 1.25 = 51.4 %: capped) / 39.59 %, canonical 8.376 % / 7.813 % (mode 1 / mode 2)
#   MAX_LOOSE64: share of samples whose float64 allowance C sens exceeds F64_BOUND itself; measured reference 10.41 % /
#                9.898 %, canonical 9.645 % / 8.376 %
MAX_VACUOUS = {'reference_m1': 0.50, 'reference_m2': 0.495, 'canonical_m1': 0.105, 'canonical_m2': 0.10}
MAX_LOOSE64 = {'reference_m1': 0.135, 'reference_m2': 0.125, 'canonical_m1': 0.125, 'canonical_m2': 0.105}
# What census() must find per branch and joint, in env-sub-steps among the samples that count (counted_mask: the float32 bound
# is not vacuous; reference chart: the float64 allowance is tight): half of what it measures there and never below 8; 0 = not
# asserted (measured below 10).  Measured, reference mode 1 / mode 2 // canonical mode 1 / mode 2:
#   vstar_hi  692 785 714 / 719 778 705 // 691 788 717 / 717 784 712      vstar_lo  896 751 682 / 895 753 691 // 926 763 695 / 924 780 705
#   motor_hi  101 166 144 / 103 168 143 //  95 169 132 /  95 166 131      motor_lo  123 184 155 / 119 186 156 // 121 175 159 / 117 178 158
#   floor       4  61  67 /   4  60  67 //   4  58  61 /   4  58  61
#   arm_hi   13 0 33 45 46 100 / 17 0 37 49 58 148 // 12 1 31 41 45  98 / 16 1 38 45 59 148
#   arm_lo   13 12 35 17 48 118 / 16 11 35 21 63 171 // 13 9 34 16 49 109 / 16 8 34 20 60 165
#   clamp    46 11 183 135 158 144 / 27 19 133 140 124 146 // 44 10 171 126 158 142 / 27 18 125 135 121 139
CENSUS_FLOOR = 8
CENSUS_MIN = {
    'reference_m1': {'vstar_hi': [346, 392, 357], 'vstar_lo': [448, 375, 341], 'motor_hi': [50, 83, 72], 'motor_lo': [61, 92, 77], 'floor': [0, 30, 33], 'arm_hi': [8, 0, 16, 22, 23, 50], 'arm_lo': [8, 8, 17, 8, 24, 59], 'clamp': [23, 8, 91, 67, 79, 72]},
    'reference_m2': {'vstar_hi': [359, 389, 352], 'vstar_lo': [447, 376, 345], 'motor_hi': [51, 84, 71], 'motor_lo': [59, 93, 78], 'floor': [0, 30, 33], 'arm_hi': [8, 0, 18, 24, 29, 74], 'arm_lo': [8, 8, 17, 10, 31, 85], 'clamp': [13, 9, 66, 70, 62, 73]},
    'canonical_m1': {'vstar_hi': [345, 394, 358], 'vstar_lo': [463, 381, 347], 'motor_hi': [47, 84, 66], 'motor_lo': [60, 87, 79], 'floor': [0, 29, 30], 'arm_hi': [8, 0, 15, 20, 22, 49], 'arm_lo': [8, 0, 17, 8, 24, 54], 'clamp': [22, 8, 85, 63, 79, 71]},
    'canonical_m2': {'vstar_hi': [358, 392, 356], 'vstar_lo': [462, 390, 352], 'motor_hi': [47, 83, 65], 'motor_lo': [58, 89, 79], 'floor': [0, 29, 30], 'arm_hi': [8, 0, 19, 22, 29, 74], 'arm_lo': [8, 0, 17, 10, 30, 82], 'clamp': [13, 9, 62, 67, 60, 69]},
}


def spec_of(key):
    chart, mode = SETS[key]
    spec = osc.iiwa_spec(dynamics_mode=mode)
    spec.chart_mode = CHARTS[chart]
    return spec


def rigid_oracle(key, B=None, seed=None):
    """A BatchedAtacomEnv (rigid-body spec of the set) of B saturating environments (module docstring), its constraint log
    cleared.  o.arm_class [B]: 0 reset pose, 1 pushed, 2 reset pose with an over-speed joint; o.dqx_class [B]."""
    chart, _ = SETS[key]
    B = B_RIGID if B is None else B
    seed = SEED if seed is None else seed
    rng = np.random.default_rng(seed)
    spec = spec_of(key)
    # 2 B candidates around the reset pose, the first B eligible ones are kept (about one in twenty has a constraint row at
    # or beyond its boundary, where slack_init returns an exact zero)
    cand = ob.BatchedAtacomEnv(spec, 2 * B, init_q=init_q('iiwa', 2 * B, rng, sigma=0.05))
    keep = np.flatnonzero((np.abs(cand.s).min(1) >= alc.S_MIN) & (np.abs(cand.s).max(1) <= alc.S_MAX))[:B]
    assert len(keep) == B, 'only %d of %d candidates are eligible' % (len(keep), 2 * B)
    o = ob.BatchedAtacomEnv(spec, B, init_q=cand.init_q[keep])
    idx = np.arange(B)
    pushed, over = idx % 8 == PUSHED_RESIDUE, idx % 8 == OVERSPEED_RESIDUE
    joint = rng.integers(0, spec.dim_q, B)
    mag = rng.uniform(0.9, 1.7, B) * rng.choice([-1.0, 1.0], B)
    qx = rng.uniform(-1.0, 1.0, (B, 3))
    dqx = rng.uniform(-1.0, 1.0, (B, 3)) * DQX_CLASSES[idx % 3]
    if pushed.any():
        src, _ = alc.pushed_oracle('iiwa_' + chart, B=int(pushed.sum()), seed=seed)
        for f in ('q', 'dq', 's', 'puck', 'has_hit', 'has_bounce', 'r_hit', 'vel_hit_x', 't', 'fv'):
            getattr(o, f)[pushed] = getattr(src, f)
    ov = np.flatnonzero(over)
    o.dq[ov, joint[ov]] = mag[ov] * spec.vel_max[joint[ov]]
    o.qx[:], o.dqx[:] = qx, dqx
    o.arm_class = np.where(pushed, 1, np.where(over, 2, 0))
    o.dqx_class = idx % 3
    s_abs = np.abs(o.s)
    ok = np.ones(B, dtype=bool)
    for f in FIELDS:
        ok &= np.isfinite(getattr(o, f)).all(1)
    ok &= np.isfinite(o.r_hit) & np.isfinite(o.vel_hit_x) & (s_abs.min(1) >= alc.S_MIN) & (s_abs.max(1) <= alc.S_MAX)
    assert ok.all(), 'environments %s are not eligible' % np.flatnonzero(~ok)
    o.get_constraints_logs()
    return o


def forced_inputs(B=None, seed=None, T=None):
    """The actions [T, B, 5] of the teacher-forced window: U(-1.3, 1.3); step t's draws do not depend on T."""
    B, T, seed = B_RIGID if B is None else B, T_RIGID if T is None else T, SEED if seed is None else seed
    return np.stack([np.random.default_rng([seed + 100, t]).uniform(-1.3, 1.3, (B, 5)) for t in range(T)])


# ------------------------------------------------------------------------- the sub-step, re-derived with its intermediates
def rigid_substep(env, q_sim, dq_sim, ddq_des, noise=None, variant=None, sink=None):
    """BatchedAtacomEnv._rigid_body_substep written out from oracle.dynamics with tau = h + M ddq (the equation of motion is
    linear in the accelerations), so that its intermediates can be counted (sink: a list, one dict of per-environment arrays
    per sub-step), perturbed (noise = (relative scale, rng): the dynamics noise of the module docstring) or made wrong on
    purpose (variant: the stand-ins of tests/test_rigid_limit_cases_oracle.py).  With none of the three it is the oracle's
    own sub-step to rounding (held there).  Advances env.qx, env.dqx; returns ddq of the six controlled joints."""
    sp = env.spec
    B = q_sim.shape[0]

    def n(x):
        return x if noise is None else x * (1.0 + noise[0] * noise[1].choice([-1.0, 1.0], x.shape))
    q9 = np.concatenate([q_sim, env.qx], 1)
    dq9 = np.concatenate([dq_sim, env.dqx], 1)
    tgt = np.concatenate([D.joint7_target(q_sim, env.qx[:, 0])[:, None], D.universal_joint_target(q9[:, :7])], 1)
    v_raw = env.SERVO_GAIN * (tgt - env.qx) / sp.dt
    vstar = np.clip(v_raw, -SERVO_VMAX, SERVO_VMAX)
    want = (vstar - env.dqx) / sp.dt
    h = D.rnea(q9, dq9, np.zeros((B, 9)))
    M = D.mass_matrix(q9)
    Mbb = n(np.einsum('bii->bi', M)[:, 6:])
    head = env.SERVO_EFFORT - (0.0 if variant == 'motor_limit_without_h' else np.abs(n(h[:, 6:])))
    lim = (head if variant == 'motor_limit_without_floor' else np.maximum(head, 0.0)) / Mbb
    ddq_b = np.minimum(np.maximum(want, -lim), lim)
    ff = ddq_b if sp.dynamics_mode == 2 else np.zeros((B, 3))
    t_raw = n(h[:, :6]) + np.einsum('bij,bj->bi', n(M[:, :6, :]), np.concatenate([ddq_des, ff], 1))
    eff = D.EFFORT_LIMIT[[0, 1, 2, 3, 5, 4]] if variant == 'effort_5_6_swapped' else D.EFFORT_LIMIT
    if variant == 'no_arm_clip':
        tau = t_raw
    elif variant == 'no_lower_arm_clip':
        tau = np.minimum(t_raw, eff)
    else:
        tau = np.clip(t_raw, -eff, eff)
    rhs = tau - n(h[:, :6]) - np.einsum('bij,bj->bi', n(M[:, :6, 6:]), ddq_b) - D.II.DAMPING[:6] * dq_sim
    Maa = np.tril(n(M[:, :6, :6]))                        # a solver reads one triangle
    Maa = Maa + np.swapaxes(np.tril(Maa, -1), 1, 2)
    ddq_a = np.linalg.solve(Maa, rhs[:, :, None])[:, :, 0]
    env.dqx = env.dqx + ddq_b * sp.dt
    env.qx = env.qx + env.dqx * sp.dt
    if sink is not None:
        with np.errstate(invalid='ignore'):
            sink.append({'vstar_hi': v_raw > SERVO_VMAX, 'vstar_lo': v_raw < -SERVO_VMAX,
                         'motor_hi': want > lim, 'motor_lo': want < -lim, 'floor': head <= 0.0,
                         'arm_hi': t_raw > eff, 'arm_lo': t_raw < -eff,
                         'clamp': np.abs(dq_sim + ddq_a * sp.dt) > env.VEL_CLAMP * sp.vel_max,
                         'ff_live': np.abs(np.einsum('bij,bj->bi', M[:, :6, 6:], ddq_b)) > 1e-3 * np.abs(t_raw),
                         'tau_abs': np.abs(t_raw), 'tau': t_raw, 'h_s_abs': np.abs(h[:, 6:])})
    return ddq_a


class RigidEnv(ob.BatchedAtacomEnv):
    """The oracle with rigid_substep in the place of its own sub-step: self.dyn_noise, self.sink as rigid_substep takes them."""
    variant = None

    def _rigid_body_substep(self, q_sim, dq_sim, ddq_des):
        return rigid_substep(self, q_sim, dq_sim, ddq_des, noise=getattr(self, 'dyn_noise', None), variant=self.variant,
                             sink=getattr(self, 'sink', None))


def outputs_of(p, action):
    """What is compared per sample: the output vector of test_gpu_dynamics (observation, s, qx, dqx, reward) and the
    absorbing flag."""
    oo, orr, oab, _ = p.step(action)
    return np.concatenate([oo, p.s, p.qx, p.dqx, orr[:, None], oab[:, None].astype(np.float64)], 1)


def step_outputs(p, inputs):
    """The step function of the recorders.  A probe of the float32 rule (parity_tools.perturbed left its J_c noise on p) also
    draws the dynamics noise, at the probe's own scale and from the probe's generator."""
    jc = getattr(p, 'jc_noise', None)
    if jc is not None:
        if not isinstance(p, RigidEnv):
            p.__class__ = RigidEnv
        p.dyn_noise = (jc[0] / parity_tools.JC_NOISE_FRACTION, jc[1])
    return outputs_of(p, inputs[0])


BRANCHES = ('vstar_hi', 'vstar_lo', 'motor_hi', 'motor_lo', 'floor', 'arm_hi', 'arm_lo', 'clamp', 'ff_live')


def census(o, actions):
    """What the inputs of a teacher-forced window exercise: `o` (left untouched) is stepped through actions [T, B, 5] with
    rigid_substep counting.  Returns per branch of BRANCHES an int array [T, B, joints]: in how many of the sample's
    sub-steps the branch was taken (vstar / motor / floor: the 3 servo joints; arm clips, clamp, ff_live: the 6 arm joints),
    'tau_abs_max' [6] / 'h_s_abs_max' [3]: the largest |tau| before the clip / |h_s|, and 'finite'."""
    p = parity_tools.slice_env(o, np.arange(o.B))
    p.__class__ = RigidEnv
    out = {b: [] for b in BRANCHES}
    tau_max, hs_max, finite = np.zeros(6), np.zeros(3), True
    tau_hi, tau_lo = np.zeros(6), np.zeros(6)
    for a in actions:
        p.sink = []
        p.step(a)
        for b in BRANCHES:
            out[b].append(sum(d[b].astype(np.int64) for d in p.sink))
        tau_max = np.maximum(tau_max, np.max([d['tau_abs'].max(0) for d in p.sink], 0))
        tau_hi = np.maximum(tau_hi, np.max([d['tau'].max(0) for d in p.sink], 0))
        tau_lo = np.minimum(tau_lo, np.min([d['tau'].min(0) for d in p.sink], 0))
        hs_max = np.maximum(hs_max, np.max([d['h_s_abs'].max(0) for d in p.sink], 0))
        finite = finite and all(np.isfinite(getattr(p, f)).all() for f in FIELDS)
    res = {b: np.array(v) for b, v in out.items()}
    res.update(tau_hi=tau_hi, tau_lo=tau_lo, tau_abs_max=tau_max, h_s_abs_max=hs_max, finite=finite, substeps=len(actions) * o.B * o.spec.substeps)
    return res


def counts(c, mask=None):
    """{branch: per-joint env-sub-step counts} of a census over the samples mask [T, B] (None: all)."""
    m = np.ones(c['floor'].shape[:2], dtype=bool) if mask is None else mask
    return {b: (c[b] * m[:, :, None]).sum((0, 1)).tolist() for b in BRANCHES}


_PREPARED = {}


def prepared(key):
    """The oracle side of the teacher-forced window of one set, computed once per process (arm_limit_cases.prepared): dict(spec,
    o, acts [T, B, 5], rec32 / rec64 with every step prepared, log, seconds = the host time it took)."""
    if key not in _PREPARED:
        t0 = time.perf_counter()
        o = rigid_oracle(key)
        acts = forced_inputs()
        rec32 = alc.recorder32(step_outputs, seed=5, state_fields=FIELDS)
        rec64 = alc.recorder64(step_outputs, seed=6, state_fields=FIELDS)
        p = parity_tools.slice_env(o, np.arange(o.B))
        for a in acts:
            rec64.prepare(p, (a,), base=rec32.prepare(p, (a,)))
            p.step(a)
        _PREPARED[key] = {'spec': o.spec, 'o': o, 'acts': acts, 'rec32': rec32, 'rec64': rec64,
                          'log': p.get_constraints_logs(), 'seconds': time.perf_counter() - t0}
        print('RIGID-LIMITS %s: host preparation %.1f s' % (key, _PREPARED[key]['seconds']))
    return _PREPARED[key]


def counted_mask(key, p):
    """[T, B]: the samples a binding branch counts on -- the float32 bound is not vacuous; on the reference chart (where that
    bound is vacuous on up to half the samples for the chart's own reasons) the float64 allowance is tight instead."""
    if SETS[key][0] == 'reference':
        return parity_tools.C_SENS * np.array(p['rec64'].sens) <= alc.F64_BOUND
    return parity_tools.C_SENS * np.array(p['rec32'].sens) + parity_tools.FLOOR <= parity_tools.VACUOUS


# ------------------------------------------------------------------------------------------------ the policy-kernel case
POLICY_KEY = 'iiwa_reference'                # arm_limit_cases.POLICY_NETS: the golden ppo_iiwa actor


def policy_actions(p):
    """The golden actor's float64 mean action on the window's step-0 states."""
    return alc.oracle_policy(POLICY_KEY).mean(p['rec32'].snaps[0].observation())
