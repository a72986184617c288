"""Conditions on the ORACLE SIDE ALONE (no device) that hold the limit-binding inputs of tests/test_gpu_arm_limits.py to their
purpose: the sets of tests/arm_limit_cases.py really sit where the joint limits, the velocity bounds of acc_truncation and
the 1.5 vel_max clamp bind; the float32 sensitivity bound and the float64 allowance say something on them (the ceilings the
GPU tests pass on); and both rules have teeth there -- a deliberately wrong float64 oracle, run as the `device`, fails them.

Every threshold here is half of what the census measures on the committed inputs (written next to it in arm_limit_cases.py),
every ceiling the measured share x 1.25: none comes from a device run.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arm_limit_cases as alc                                                        # noqa: E402
import parity_tools                                                                  # noqa: E402
from oracle import atacom_batched as ob                                              # noqa: E402
from parity_tools import C_SENS, FLOOR, VACUOUS, SensitivityRecorder, slice_env      # noqa: E402

KEYS = list(alc.SETS)


def test_recorder_defaults_are_the_float32_rule():
    """The optional arguments of SensitivityRecorder default to the module's constants, whose values stand."""
    r = SensitivityRecorder(alc.step_outputs)
    assert (r.quick_scales, r.deep_scales, r.floor, r.jc_noise, r.stacked) == (
        parity_tools.QUICK_SCALES, parity_tools.DEEP_SCALES, parity_tools.FLOOR, True, False)
    assert parity_tools.QUICK_SCALES == (2e-7, 1e-6, 4e-6) and parity_tools.DEEP_SCALES == (1e-6, 4e-6, 1.6e-5)
    assert (C_SENS, FLOOR, VACUOUS) == (4.0, 5e-6, 1e-2)
    assert (parity_tools.REPRO_ERR, parity_tools.REPRO_GAIN, parity_tools.MAX_UNREPRODUCED) == (1e-3, 5.0, 2e-3)
    # the float64 scales: the float32 ones x about eps64 / eps32 (1.9e-9, taken as 1e-9 .. 1.25e-9), widened 1000 x
    ratio = np.finfo(np.float64).eps / np.finfo(np.float32).eps * 1000
    for f64, f32 in ((alc.F64_QUICK_SCALES, parity_tools.QUICK_SCALES), (alc.F64_DEEP_SCALES, parity_tools.DEEP_SCALES)):
        r = np.array(f64) / np.array(f32)
        assert (0.5 * ratio <= r).all() and (r <= ratio).all(), r
    assert alc.F64_BOUND == 1e-8


def test_generation_is_deterministic_in_the_seed():
    a, sa = alc.pushed_oracle('planar', B=32, seed=5)
    b, sb = alc.pushed_oracle('planar', B=32, seed=5)
    for f in ('q', 'dq', 's', 'puck', 'push_steps', 'overspeed'):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(sa, sb)
    full = alc.prepared('planar')                        # and another seed gives other states
    assert not np.array_equal(a.q, full['o'].q[:32]) and not np.array_equal(sa, full['sign'][:32])
    acts = alc.forced_inputs('planar', sa, seed=5, T=3)
    assert np.array_equal(acts, alc.forced_inputs('planar', sb, seed=5, T=5)[:3])     # step t's draws do not depend on T
    assert (acts[:, 0::2] == sa[0::2]).all() and (np.abs(acts[:, 1::2]) != 1).all() and np.abs(acts).max() <= 1.3


@pytest.mark.parametrize('key', KEYS)
def test_the_sets_are_what_the_module_says(key):
    p = alc.prepared(key)
    o, sp = p['o'], p['spec']
    B, T = alc.B_LIMITS[key], alc.T_LIMITS[key]
    assert o.B == B and p['acts'].shape == (T, B, sp.n_null) and sp.chart_mode == alc.SETS[key][1]
    assert np.isfinite(o.q).all() and np.isfinite(o.dq).all() and np.isfinite(o.puck).all()
    assert alc.S_MIN <= np.abs(o.s).min() and np.abs(o.s).max() <= alc.S_MAX
    assert o.stat_cnt.sum() == 0 and np.isneginf(o.stat_cmax).all()                   # the log is cleared
    assert set(np.unique(o.push_steps)) == set(alc.PUSH_STEPS) and (o.t == o.push_steps).all()      # no resets on the way
    over = o.overspeed >= 0
    assert 0.2 <= over.mean() <= 0.3
    for P in alc.PUSH_STEPS:
        assert (over & (o.push_steps == P)).any()
    ratio = np.abs(o.dq[over, o.overspeed[over]]) / sp.vel_max[o.overspeed[over]]
    assert ratio.min() >= 0.9 and ratio.max() <= 1.7 and (ratio > 1.5).any() and (ratio < 1.0).any()
    # what the oracle returns over the window is finite: a NaN would pass every comparison of the GPU tests
    for r in (p['rec32'], p['rec64']):
        assert len(r.base) == T and all(np.isfinite(b).all() for b in r.base) and np.isfinite(np.array(r.sens)).all()
    assert all(np.isfinite(x) for x in p['log'])


@pytest.mark.parametrize('key', KEYS)
def test_census_of_the_sets_the_gpu_tests_run(key):
    p = alc.prepared(key)
    c = alc.census(p['o'], p['acts'])
    print('census %s: %s' % (key, c))
    m = alc.CENSUS_MIN
    assert c['samples'] == alc.B_LIMITS[key] * alc.T_LIMITS[key]
    assert c['joint_substeps'] == c['samples'] * p['spec'].substeps * p['spec'].dim_q
    assert min(c['truncation'].values()) >= max(m['truncation'][key], m['truncation_floor']), c['truncation']
    assert c['nested_saturation'] >= m['nested_saturation'][key], c
    assert c['clamp_samples'] >= m['clamp_samples'][key] >= 20, c
    assert c['task_rows_min_abs_s_below_1e-3'] >= m['task_rows'][key] >= 1, c
    assert c['limit_rows_min_abs_s_below_1e-3'] >= m['limit_rows'][key] >= (2 if key.startswith('iiwa') else 1), c
    assert c['violated_share'] >= m['violated_share'][key] > 0, c
    assert c['fast_share'] >= m['fast_share'][key] >= 0.05, c
    assert c['log_c_max'] >= m['log_c_max'][key] > 0, c
    assert np.allclose((c['log_c_avg'], c['log_c_max'], c['log_dq_max']), p['log'], rtol=0, atol=1e-12)


@pytest.mark.parametrize('key', KEYS)
def test_ceilings_against_the_oracle_alone(key):
    """The vacuous share of the float32 bound and the loose share of the float64 allowance, over all B environments and
    over the first B_RAGGED (the batch of the T-step kernel cases), stay under the ceilings the GPU tests pass on; and the
    oracle, run as its own device, passes both rules as they are applied there."""
    p = alc.prepared(key)
    for n in (None, alc.B_RAGGED):
        vac, loose = alc.shares(p, n)
        print('%s, first %s environments: float32 bound vacuous on %.3f %% (ceiling %.1f %%), float64 allowance loose on '
              '%.3f %% (ceiling %.1f %%)' % (key, n or 'all', 100 * vac, 100 * alc.MAX_VACUOUS[key], 100 * loose,
                                             100 * alc.MAX_LOOSE64[key]))
        assert vac <= alc.MAX_VACUOUS[key] <= 0.5 and loose <= alc.MAX_LOOSE64[key]
        assert alc.MAX_VACUOUS[key] <= max(np.ceil(vac * 1.25 * 200) / 200, 0.005) + 0.01      # and no looser than the rule
    r32, r64 = p['rec32'].fresh(), p['rec64'].fresh()
    rng = np.random.default_rng(1)
    for t, snap in enumerate(r32.snaps):
        # float32 stand-in: the oracle from the state and action ROUNDED TO FLOAT32 (what set_state hands a float32 device),
        # its outputs rounded again -- the least a float32 device does, and enough to put errors above 1e-3 through the deep
        # probe and the reproduction audit.  float64 stand-in: the oracle from inputs moved by 4 eps64
        lo = slice_env(snap, np.arange(snap.B))
        for f in ('q', 'dq', 's', 'puck'):
            setattr(lo, f, getattr(lo, f).astype(np.float32).astype(np.float64))
        r32.compare(t, alc.step_outputs(lo, (r32.inputs[t][0].astype(np.float32).astype(np.float64),)).astype(np.float32))
        hi = parity_tools.perturbed(snap, 4 * np.finfo(np.float64).eps, rng, jc_noise=False)
        r64.compare(t, alc.step_outputs(hi, r64.inputs[t]))
    print(r32.finish('%s: the oracle on float32-rounded inputs as the device' % key, max_vacuous=alc.MAX_VACUOUS[key]))
    print(r64.finish_float64('%s: the oracle on inputs moved by 4 eps64 as the device' % key, max_loose=alc.MAX_LOOSE64[key]))


@pytest.mark.parametrize('key', list(alc.POLICY_NETS))
def test_policy_case_ceiling_against_the_oracle_alone(key):
    """The policy-kernel case steps the window's states POLICY_STEPS with the action of the golden actor network instead of
    the window's: with the float64 network's action the float32 bound stays under the set's ceiling there as well, and the
    network really drives the arm (its mean action is neither zero nor saturated everywhere)."""
    p, pol = alc.prepared(key), alc.oracle_policy(key)
    rec = alc.recorder32(seed=7)
    for t in alc.POLICY_STEPS:
        snap = p['rec32'].snaps[t]
        a = pol.mean(snap.observation())
        assert np.isfinite(a).all() and 0.05 < np.mean(np.abs(a) >= 1.0) < 0.95, np.mean(np.abs(a) >= 1.0)
        rec.record(snap, (a,), alc.step_outputs(slice_env(snap, np.arange(snap.B)), (a,)))
    vac = float(np.mean(C_SENS * np.array(rec.sens) + FLOOR > VACUOUS))
    print('%s policy case: float32 bound vacuous on %.3f %% (ceiling %.1f %%)' % (key, 100 * vac, 100 * alc.MAX_VACUOUS[key]))
    assert vac <= alc.MAX_VACUOUS[key]


# ------------------------------------------------------------------------------------------- deliberately wrong stand-ins
class _VelocityBoundSignFlipped(ob.BatchedAtacomEnv):
    """(a) acc_truncation with the sign of the velocity bound flipped wherever that bound, and not +-acc_max, is the limit."""

    def acc_truncation(self, dq, ddq):
        sp = self.spec
        up_v, lo_v = -sp.Kq * (dq - sp.vel_max), -sp.Kq * (dq + sp.vel_max)
        up = np.where(np.abs(up_v) < sp.acc_max, -up_v, np.clip(up_v, -sp.acc_max, sp.acc_max))
        lo = np.where(np.abs(lo_v) < sp.acc_max, -lo_v, np.clip(lo_v, -sp.acc_max, sp.acc_max))
        return np.maximum(np.minimum(ddq, up), lo)


class _ClampAtVelMax(ob.BatchedAtacomEnv):
    """(b) the integrator's clamp at 1.0 vel_max instead of 1.5."""
    VEL_CLAMP = 1.0


class _NeighbourSlack(ob.BatchedAtacomEnv):
    """(c) the slack of the last but one joint-limit row taken from its neighbour (a stale lane in J_c's slack column)."""

    def tangent_space_accel(self, q, dq, s, alpha, terms=None):
        s = s.copy()
        s[:, -2] = s[:, -1]
        return super().tangent_space_accel(q, dq, s, alpha, terms)


VARIANTS = {'velocity_bound_sign': _VelocityBoundSignFlipped, 'clamp_at_vel_max': _ClampAtVelMax,
            'neighbour_slack': _NeighbourSlack}


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('key', ['planar', 'iiwa_reference'])
def test_a_wrong_oracle_fails_both_rules(key, variant):
    """The float64 oracle with one defect, as the `device` of the teacher-forced window, against the unmodified oracle: it
    must fail the float64 rule on more than 1 % of the samples and the float32 rule on at least one sample whose bound is
    not vacuous.  Only the samples furthest above their quick bound get the deep probe (enough of them to decide either
    question); a sample counts only if it stays unexplained after it, as in the GPU tests."""
    p = alc.prepared(key)
    r32, r64 = p['rec32'].fresh(), p['rec64'].fresh()
    for t, snap in enumerate(r32.snaps):
        wrong = slice_env(snap, np.arange(snap.B))
        wrong.__class__ = VARIANTS[variant]
        dev = alc.step_outputs(wrong, r32.inputs[t])
        r32.compare(t, dev)
        r64.compare(t, dev)
    n = np.array(r64.err).size
    E, S, bad64, _ = r64._explain(limit=n // 100 + 4)
    print('%s, %s: float64 rule unexplained on %d of the %d probed (%d samples, 1 %% = %d); quick bound exceeded on %.2f %%'
          % (key, variant, len(bad64), n // 100 + 4, n, n // 100, 100 * np.mean(E > C_SENS * np.array(r64.sens) + r64.floor)))
    assert len(bad64) > n // 100
    E, S, bad32, _ = r32._explain(limit=8)
    told = [b for b in bad32 if C_SENS * b[3] + FLOOR <= VACUOUS]
    print('%s, %s: float32 rule unexplained on %d of the 8 probed, %d of them with a bound that is not vacuous: %s'
          % (key, variant, len(bad32), len(told), told[:3]))
    assert told
    # and the reproduction audit of finish(), with the wider draws these sets use: no perturbed oracle lands near the wrong
    # device (step 0 of the window, the first 16 environments)
    few = p['rec32'].head(16)
    few.compare(0, r32.dev[0][:16])
    E0 = np.array(few.err[:1])
    unrep, n_big = few._unreproduced(E0)
    print('%s, %s: %d of the %d errors above 1e-3 at step 0 of the first 16 environments are not reproduced' % (key, variant, len(unrep), n_big))
    assert len(unrep) > parity_tools.MAX_UNREPRODUCED * E0.size
