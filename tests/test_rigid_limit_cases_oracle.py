"""Conditions on the ORACLE SIDE ALONE (no device) that hold the saturating inputs of tests/test_gpu_rigid_limits.py to their
purpose: the sets of tests/rigid_limit_cases.py really sit where the servo motor limit, its floor, the arm effort limits and
the integrator's clamp bind -- counted among the samples on which the rules say something; the float32 bound and the float64
allowance stay under the ceilings the GPU tests pass on; and both rules have teeth there -- a float64 oracle with one of the
saturations wrong, run as the `device`, fails them, while the oracle under float32-sized dynamics noise passes.

Every census floor is half of what the census measures on the committed inputs and never below 8 env-sub-steps, every
ceiling the measured share x 1.25 (both written in rigid_limit_cases.py): none comes from a device run.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arm_limit_cases as alc                                                        # noqa: E402
import parity_tools                                                                  # noqa: E402
import rigid_limit_cases as rlc                                                      # noqa: E402
from oracle import atacom_batched as ob                                              # noqa: E402
from parity_tools import C_SENS, FLOOR, VACUOUS, slice_env                           # noqa: E402

KEYS = list(rlc.SETS)


def test_recorders_keep_their_defaults():
    """state_fields is optional on recorder32 / recorder64: without it they perturb what they always did."""
    assert alc.recorder32().fields == alc.recorder64().fields == ('q', 'dq', 's', 'puck') == alc.ARM_FIELDS
    assert parity_tools.SensitivityRecorder(alc.step_outputs).fields == alc.ARM_FIELDS
    r = alc.recorder32(rlc.step_outputs, state_fields=rlc.FIELDS)
    assert r.fields == rlc.FIELDS and r.jc_noise and r.floor == FLOOR and r.quick_scales == parity_tools.QUICK_SCALES
    r = alc.recorder64(rlc.step_outputs, state_fields=rlc.FIELDS)
    assert r.fields == rlc.FIELDS and not r.jc_noise and r.floor == alc.F64_BOUND and r.quick_scales == alc.F64_QUICK_SCALES


def test_generation_is_deterministic_in_the_seed():
    a, b = rlc.rigid_oracle('canonical_m1', B=48, seed=5), rlc.rigid_oracle('canonical_m1', B=48, seed=5)
    for f in rlc.FIELDS + ('arm_class', 'dqx_class', 't'):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    c = rlc.rigid_oracle('canonical_m1', B=48, seed=6)
    assert not np.array_equal(a.q, c.q) and not np.array_equal(a.dqx, c.dqx)
    m2 = rlc.rigid_oracle('canonical_m2', B=48, seed=5)                              # the two modes share their states
    for f in rlc.FIELDS:
        assert np.array_equal(getattr(a, f), getattr(m2, f)), f
    assert (a.spec.dynamics_mode, m2.spec.dynamics_mode) == (1, 2)
    acts = rlc.forced_inputs(B=48, seed=5, T=2)
    assert np.array_equal(acts, rlc.forced_inputs(B=48, seed=5, T=3)[:2]) and np.abs(acts).max() <= 1.3
    assert (np.abs(acts) > 1.0).mean() > 0.1                                         # the action clip is met


@pytest.mark.parametrize('key', KEYS)
def test_the_sets_are_what_the_module_says(key):
    p = rlc.prepared(key)
    o, sp = p['o'], p['spec']
    B, T = rlc.B_RIGID, rlc.T_RIGID
    chart, mode = rlc.SETS[key]
    assert o.B == B and B % 64 == 0 and p['acts'].shape == (T, B, 5)
    assert (sp.dynamics_mode, sp.chart_mode) == (mode, rlc.CHARTS[chart])
    assert 0 < rlc.B_RAGGED < B and rlc.B_RAGGED % 64 != 0 and (4 * rlc.B_RAGGED) % 64 != 0      # a partial wave, lane and quad
    for f in rlc.FIELDS:
        assert np.isfinite(getattr(o, f)).all(), f
    assert alc.S_MIN <= np.abs(o.s).min() and np.abs(o.s).max() <= alc.S_MAX
    assert o.stat_cnt.sum() == 0 and np.isneginf(o.stat_cmax).all()                   # the log is cleared
    # the classes are interleaved: every wave of 64 environments (16 with a quad each) holds every combination
    combo = o.arm_class * 3 + o.dqx_class
    for a in range(B - 23):
        assert len(np.unique(combo[a:a + 24])) == 9
    for a in range(B - 3):
        assert len(np.unique(o.dqx_class[a:a + 3])) == 3
    assert np.mean(o.arm_class == 0) == 0.75 and np.mean(o.arm_class == 1) == np.mean(o.arm_class == 2) == 0.125
    assert np.abs(o.qx).max() <= 1.0 and (np.abs(o.dqx) <= rlc.DQX_CLASSES[o.dqx_class]).all()
    over = o.arm_class == 2
    ratio = (np.abs(o.dq[over]) / sp.vel_max).max(1)
    assert ratio.min() >= 0.9 and ratio.max() <= 1.7 and (ratio > 1.5).any()
    assert (o.dq[o.arm_class == 0] == 0).all() and (np.abs(o.dq[o.arm_class == 1]) > 0).any()
    # what the oracle returns over the window is finite (a NaN would pass every comparison of the GPU tests), and step 1
    # starts just after saturation: servo joints at +-1.5 v_max
    for r in (p['rec32'], p['rec64']):
        assert len(r.base) == T and all(np.isfinite(b).all() for b in r.base) and np.isfinite(np.array(r.sens)).all()
        assert r.fields == rlc.FIELDS
    at_vmax = np.abs(np.abs(p['rec32'].snaps[1].dqx) - rlc.SERVO_VMAX) < 1e-9
    assert at_vmax.mean(0).min() > 0.25, at_vmax.mean(0)
    assert all(np.isfinite(x) for x in p['log'])


@pytest.mark.parametrize('key', ['reference_m1', 'canonical_m2'])
def test_the_counting_sub_step_is_the_oracles_own(key):
    """rigid_substep with no noise, no variant and no sink computes what BatchedAtacomEnv._rigid_body_substep computes (tau =
    h + M ddq in the place of a second inverse-dynamics pass: rounding apart), over the window."""
    p = rlc.prepared(key)
    a, b = slice_env(p['o'], np.arange(p['o'].B)), slice_env(p['o'], np.arange(p['o'].B))
    b.__class__ = rlc.RigidEnv
    for act in p['acts']:
        ya, yb = rlc.outputs_of(a, act), rlc.outputs_of(b, act)
        assert (np.abs(ya - yb) / np.maximum(1.0, np.abs(ya))).max() < 1e-9
    assert type(p['rec32'].snaps[0]) is ob.BatchedAtacomEnv                           # the expected outputs: the oracle itself


@pytest.mark.parametrize('key', KEYS)
def test_census_of_the_sets_the_gpu_tests_run(key):
    """Every min / max of rigid_body_substep is taken on both sides, on samples whose bound says something (the arm clips of
    joint 2 at +320 Nm apart: module docstring of rigid_limit_cases)."""
    p = rlc.prepared(key)
    c = rlc.census(p['o'], p['acts'])
    mask = rlc.counted_mask(key, p)
    got, everywhere = rlc.counts(c, mask), rlc.counts(c)
    print('census %s over %d env-sub-steps, all samples: %s' % (key, c['substeps'], everywhere))
    print('census %s, the %.1f %% of the samples that count: %s' % (key, 100 * mask.mean(), got))
    print('census %s: largest tau before the clip %s, smallest %s; largest |h_s| %s' % (
        key, np.round(c['tau_hi'], 1), np.round(c['tau_lo'], 1), np.round(c['h_s_abs_max'], 1)))
    assert c['finite'] and c['substeps'] == rlc.B_RIGID * rlc.T_RIGID * p['spec'].substeps
    need = rlc.CENSUS_MIN[key]
    for branch, floors in need.items():
        for j, f in enumerate(floors):
            assert f == 0 or f >= rlc.CENSUS_FLOOR, (branch, j, f)
            assert got[branch][j] >= f, (branch, j, got[branch][j], f)
            assert f == 0 or f >= got[branch][j] // 2, (branch, j, got[branch][j], f)   # half of what is measured, no less
    # the mandatory branches: none of them may be left at 0
    for branch in ('vstar_hi', 'vstar_lo', 'motor_hi', 'motor_lo'):
        assert min(need[branch]) >= rlc.CENSUS_FLOOR, branch
    assert max(need['floor']) >= rlc.CENSUS_FLOOR
    for branch in ('arm_hi', 'arm_lo'):
        assert min(need[branch][2:]) >= rlc.CENSUS_FLOOR, branch
    assert max(need['clamp']) >= rlc.CENSUS_FLOOR
    # step 0 carries the binding sub-steps, and the servo speed classes do what they are there for
    assert c['arm_hi'][0].sum() + c['arm_lo'][0].sum() > c['arm_hi'][1].sum() + c['arm_lo'][1].sum()
    slow = p['o'].dqx_class == 0
    assert c['motor_hi'][:, slow].sum() + c['motor_lo'][:, slow].sum() + c['floor'][:, slow].sum() == 0
    assert np.allclose(p['log'], slice_and_log(p), rtol=0, atol=1e-12)


def slice_and_log(p):
    q = slice_env(p['o'], np.arange(p['o'].B))
    for a in p['acts']:
        q.step(a)
    return q.get_constraints_logs()


def _as_device(p, make):
    """(r32, r64) with make(copy of the state before step t) -> the environment that plays the device, compared on every step."""
    r32, r64 = p['rec32'].fresh(), p['rec64'].fresh()
    for t, snap in enumerate(r32.snaps):
        dev = rlc.outputs_of(make(slice_env(snap, np.arange(snap.B)), t), r32.inputs[t][0])
        r32.compare(t, dev)
        r64.compare(t, dev)
    return r32, r64


@pytest.mark.parametrize('key', KEYS)
def test_ceilings_against_the_oracle_alone(key):
    """The vacuous share of the float32 bound and the loose share of the float64 allowance, over all B environments and over
    the first B_RAGGED, stay under the ceilings the GPU tests pass on; the oracle as its own device passes both rules as they
    are applied there; and so does, under the float32 rule, the oracle with float32-sized DYNAMICS NOISE alone (h and the
    mass-matrix entries perturbed by 2e-7 relative at every use, inputs exact): the term the allowance has for it covers it."""
    p = rlc.prepared(key)
    chart = rlc.SETS[key][0]
    worst = [0.0, 0.0]
    for n in (None, rlc.B_RAGGED):
        vac, loose = alc.shares(p, n)
        worst = [max(worst[0], vac), max(worst[1], loose)]
        print('%s, first %s environments: float32 bound vacuous on %.3f %% (ceiling %.1f %%), float64 allowance loose on '
              '%.3f %% (ceiling %.1f %%)' % (key, n or 'all', 100 * vac, 100 * rlc.MAX_VACUOUS[key], 100 * loose,
                                             100 * rlc.MAX_LOOSE64[key]))
        assert vac <= rlc.MAX_VACUOUS[key] <= 0.5 and loose <= rlc.MAX_LOOSE64[key]
    rule = [np.ceil(w * 1.25 * 200 - 1e-9) / 200 for w in worst]
    assert rlc.MAX_VACUOUS[key] <= (min(rule[0], 0.5) if chart == 'reference' else rule[0])      # no looser than the rule
    assert rlc.MAX_LOOSE64[key] <= rule[1]
    rng = np.random.default_rng(1)

    def rounded(lo, t):                                   # the least a float32 device does: inputs rounded to float32
        for f in rlc.FIELDS:
            setattr(lo, f, getattr(lo, f).astype(np.float32).astype(np.float64))
        return lo
    r32 = p['rec32'].fresh()
    r64 = p['rec64'].fresh()
    for t, snap in enumerate(r32.snaps):
        a32 = r32.inputs[t][0].astype(np.float32).astype(np.float64)
        r32.compare(t, rlc.outputs_of(rounded(slice_env(snap, np.arange(snap.B)), t), a32).astype(np.float32))
        hi = parity_tools.perturbed(snap, 4 * np.finfo(np.float64).eps, rng, rlc.FIELDS, jc_noise=False)
        r64.compare(t, rlc.outputs_of(hi, r64.inputs[t][0]))
    print(r32.finish('%s: the oracle on float32-rounded inputs as the device' % key, max_vacuous=rlc.MAX_VACUOUS[key]))
    print(r64.finish_float64('%s: the oracle on inputs moved by 4 eps64 as the device' % key, max_loose=rlc.MAX_LOOSE64[key]))

    def noisy(q, t):
        q.__class__ = rlc.RigidEnv
        q.dyn_noise = (parity_tools.QUICK_SCALES[0], rng)
        return q
    n32, _ = _as_device(p, noisy)
    E = np.array(n32.err)
    print(n32.finish('%s: the oracle under dynamics noise of 2e-7 as the device' % key, max_vacuous=rlc.MAX_VACUOUS[key]))
    print('%s: dynamics noise of 2e-7 alone moves the outputs by median %.2e / p99 %.2e / max %.2e; above the floor of 5e-6 on '
          '%.1f %% of the samples' % (key, np.median(E), np.quantile(E, 0.99), E.max(), 100 * np.mean(E > FLOOR)))
    assert np.mean(E > FLOOR) > 0.05                       # the term is no formality: rounding of h and M alone exceeds the floor


@pytest.mark.parametrize('mode', [1, 2])
def test_policy_case_ceiling_against_the_oracle_alone(mode):
    """The policy-kernel case steps the window's step-0 states with the golden actor's mean action instead of the window's:
    the float32 bound stays under the set's ceiling there as well, and the network really drives the arm."""
    key = 'reference_m%d' % mode
    p = rlc.prepared(key)
    a = rlc.policy_actions(p)
    assert np.isfinite(a).all() and 0.05 < np.mean(np.abs(a) >= 1.0) < 0.95, np.mean(np.abs(a) >= 1.0)
    rec = alc.recorder32(rlc.step_outputs, seed=7, state_fields=rlc.FIELDS)
    snap = p['rec32'].snaps[0]
    rec.record(snap, (a,), rlc.outputs_of(slice_env(snap, np.arange(snap.B)), a))
    vac = float(np.mean(C_SENS * np.array(rec.sens) + FLOOR > VACUOUS))
    print('%s policy case: float32 bound vacuous on %.3f %% (ceiling %.1f %%)' % (key, 100 * vac, 100 * rlc.MAX_VACUOUS[key]))
    assert vac <= rlc.MAX_VACUOUS[key]


# ------------------------------------------------------------------------------------------- deliberately wrong stand-ins
VARIANTS = {'a': 'no_arm_clip', 'b': 'effort_5_6_swapped', 'c': 'motor_limit_without_floor', 'd': 'motor_limit_without_h',
            'e': 'no_lower_arm_clip'}


def _subset(rec, t, idx):
    """A recorder holding step t of `rec` restricted to the environments idx."""
    import copy
    r = copy.copy(rec)
    r.snaps, r.inputs = [slice_env(rec.snaps[t], idx)], [tuple(x[idx] for x in rec.inputs[t])]
    r.base, r.sens = [rec.base[t][idx]], [rec.sens[t][idx].copy()]
    r.err, r.where, r.dev = [], [], []
    return r


def _fails_both_rules(p, r32, r64, what, audit=True):
    n = np.array(r64.err).size
    E, S, bad64, _ = r64._explain(limit=n // 100 + 4)
    print('%s: float64 rule unexplained on %d of the %d probed (%d samples, 1 %% = %d); quick bound exceeded on %.2f %%'
          % (what, len(bad64), n // 100 + 4, n, n // 100, 100 * np.mean(E > C_SENS * np.array(r64.sens) + r64.floor)))
    assert len(bad64) > n // 100
    E, S, bad32, _ = r32._explain(limit=8)
    told = [b for b in bad32 if C_SENS * b[3] + FLOOR <= VACUOUS]
    print('%s: float32 rule unexplained on %d of the 8 probed, %d of them with a bound that is not vacuous: %s'
          % (what, len(bad32), len(told), told[:3]))
    assert told
    if not audit:
        return
    # and the reproduction audit of finish(): no perturbed oracle lands near the wrong device (the 16 largest errors of step 0)
    idx = np.sort(np.argsort(-np.array(r32.err[0]), kind='stable')[:16])
    few = _subset(p['rec32'], 0, idx)
    few.compare(0, r32.dev[0][idx])
    E0 = np.array(few.err[:1])
    unrep, n_big = few._unreproduced(E0)
    print('%s: %d of the %d errors above 1e-3 among the 16 largest of step 0 are not reproduced' % (what, len(unrep), n_big))
    assert len(unrep) > parity_tools.MAX_UNREPRODUCED * E0.size


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('key', ['reference_m1', 'canonical_m2'])
def test_a_wrong_oracle_fails_both_rules(key, variant):
    """The float64 oracle with one saturation wrong -- (a) no arm effort clip, (b) the effort limits of joints 5 and 6
    swapped, (c) the motor limit without its floor at 0, (d) the motor limit as effort_s / M_ss, (e) only min(t, +effort) --
    as the `device` of the window, against the unmodified oracle: it must fail the float64 rule on more than 1 % of the
    samples and the float32 rule on at least one sample whose bound is not vacuous (tests/test_arm_limit_cases_oracle.py)."""
    p = rlc.prepared(key)

    def wrong(q, t):
        q.__class__ = type('Wrong_' + variant, (rlc.RigidEnv,), {'variant': VARIANTS[variant]})
        return q
    r32, r64 = _as_device(p, wrong)
    _fails_both_rules(p, r32, r64, '%s, (%s) %s' % (key, variant, VARIANTS[variant]))


@pytest.mark.parametrize('chart', list(rlc.CHARTS))
def test_mode_2_is_not_mode_1(chart):
    """The oracle of dynamics_mode 2 as the device against mode 1's expected outputs fails both rules: the feed-forward term
    is live on these samples (what the GPU test of the same name relies on)."""
    p = rlc.prepared(chart + '_m1')
    spec2 = rlc.spec_of(chart + '_m2')

    def mode2(q, t):
        q.spec = spec2
        return q
    r32, r64 = _as_device(p, mode2)
    _fails_both_rules(p, r32, r64, '%s chart, mode 2 against mode 1' % chart, audit=False)
