"""Conditions on the REFERENCE SIDE ALONE (no device) that hold the constraint-active inputs of
tests/test_gpu_point_reach_active.py to their purpose: the (n, seed) cases of tests/point_reach_cases.py really sit where the
constraints bind, the float32 sensitivity bound says something on them, the float64 answer is determined far inside the
device's 1e-8 bound, and the restatement is the reference's own class there (tests/golden/point_reach_active.npz, recorded by
profiles/tools/gen_point_reach_active_golden.py).

A sample that fails the line-by-line check is an input to drop by raising gap_lo or the prefix ON THIS EVIDENCE -- never on
what a device returns.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_reach_cases as prc                  # noqa: E402
import point_reach_oracle as pro                 # noqa: E402
from parity_tools import C_SENS, FLOOR, VACUOUS, SensitivityRecorder, slice_env     # noqa: E402
from point_reach_cases import MAX_VACUOUS, step_outputs                              # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'point_reach_active.npz'))
B, T = prc.B_ACTIVE, prc.T_ACTIVE


@pytest.mark.parametrize('draw_mode', ['supplied', 'generator'])
@pytest.mark.parametrize('n', [2, 4])
def test_census_of_the_cases_the_gpu_tests_run(n, draw_mode):
    o = prc.active_oracle(B, n, prc.SEEDS[n])
    acts, draws = prc.forced_inputs(n, prc.SEEDS[n])
    c = prc.census(o, acts, draws if draw_mode == 'supplied' else None)
    print('census n=%d %s draws: %s' % (n, draw_mode, c))
    assert c['samples'] == B * T
    assert c['inside'] >= 0.10 and c['within_0.8'] >= 0.50, c          # the agent inside / next to an obstacle
    assert c['min_abs_s'] < 1e-3, c                                       # the ~ 1 / s slack dynamics, a nearly singular J_c
    fl = np.array(c['wall_flips_axis_low_high'])
    assert c['wall_flips'] >= 20 and ((fl[:, 0] > 0) & (fl[:, 1] > 0)).any(), c    # the walls at 0 AND at 10 of an axis
    assert min(c['clip_low'], c['clip_inactive'], c['clip_high']) >= 0.10, c       # every state of the acceleration clip
    assert c['log_max'] > 0, c                                            # a violated constraint is logged


def test_generation_is_deterministic_and_leaves_no_exact_zero_slack():
    for n in (2, 4):
        a, b = prc.active_oracle(64, n, 5), prc.active_oracle(64, n, 5)
        assert np.array_equal(a.get_state(), b.get_state())
        assert not np.array_equal(a.get_state(), prc.active_oracle(64, n, 6).get_state())
        o = prc.active_oracle(B, n, prc.SEEDS[n])
        assert np.isfinite(o.get_state()).all() and (o.s != 0).all()
        assert o.log_cnt.sum() == 0 and np.isneginf(o.log_max).all()     # the log is cleared
        assert (o.episode == 1).all() and o.have_centres.all()


@pytest.mark.parametrize('n', [2, 4])
def test_sensitivity_bound_is_not_vacuous_on_the_cases(n):
    """The recorder of the float32 test, driven with the restatement's own output as the `device`: the share of samples on
    which 4 sens + 5e-6 exceeds 1e-2 (where the bound would say nothing) stays under the ceiling the existing random-walk
    test uses."""
    o = prc.active_oracle(B, n, prc.SEEDS[n])
    acts, draws = prc.forced_inputs(n, prc.SEEDS[n])
    rec = SensitivityRecorder(step_outputs, seed=3, state_fields=('state', 's'))
    for t in range(T):
        dev = step_outputs(slice_env(o, np.arange(B)), (acts[t], draws[t]))
        rec.record(o, (acts[t], draws[t]), dev)
        o.step(acts[t], draws=draws[t])
    vac = float(np.mean(C_SENS * np.array(rec.sens) + FLOOR > VACUOUS))
    print('n=%d: bound vacuous on %.3f %% of %d samples' % (n, 100 * vac, B * T))
    assert vac <= MAX_VACUOUS, vac
    rec.finish('restatement against itself, n=%d' % n, max_vacuous=MAX_VACUOUS)


@pytest.mark.parametrize('n', [2, 4])
def test_line_by_line_and_vectorised_restatements_agree_on_the_cases(n):
    """Every 4th environment (256 of them, lower-wall ones included) at every step of the window: PointReachScalar (scipy
    SVD, the reference's rref) from the state PointReachBatched is in, within 1e-10 -- the float64 answer on exactly these
    inputs is determined a hundred times inside the device's 1e-8."""
    o = prc.active_oracle(B, n, prc.SEEDS[n])
    acts, draws = prc.forced_inputs(n, prc.SEEDS[n])
    idx = np.arange(0, B, 4)
    assert len(idx) >= 256 and idx[-1] >= B - B // prc.WALL_SHARE
    worst = 0.0
    for t in range(T):
        st0, s0 = o.state.copy(), o.s.copy()
        obs, r, _, _ = o.step(acts[t], draws=draws[t])
        for b in idx:
            sc = pro.PointReachScalar(n_objects=n, random_walk=True)
            sc._state, sc.s = st0[b].copy(), s0[b].copy()
            o1, r1, _, _ = sc.step(acts[t, b], draws=draws[t, b])
            e = max(np.abs(o1 - obs[b]).max(), np.abs(sc.s - o.s[b]).max(), abs(r1 - r[b]))
            worst = max(worst, e)
            assert e <= 1e-10, (t, b, e)
    print('n=%d: worst |line by line - vectorised| = %.3e over %d samples' % (n, worst, T * len(idx)))


@pytest.mark.parametrize('n', [2, 4])
def test_restatement_reproduces_the_active_fixture(n):
    """The reference's own class, its state and slack SET to generated states and stepped once, against both restatements."""
    S = int(G['states'])
    k = lambda name: G['n%d_%s' % (n, name)]                           # noqa: E731
    state0, s0 = prc.fixture_states(n)                                   # the fixture's inputs ARE the generator's
    assert S == prc.FIXTURE_STATES and np.array_equal(state0, k('state0')) and np.array_equal(s0, k('s0'))
    d = np.sqrt(((state0[:, None, 0:2] - state0[:, 4:].reshape(S, n, 4)[:, :, 0:2]) ** 2).sum(2)).min(1)
    q1 = k('state1')[:, 0:2]
    print('n=%d fixture: min d %.3f, inside %.2f, min |s| %.2e, log max %+.3f, steps onto a wall: %d low %d high'
          % (n, d.min(), (d < 0.6).mean(), np.abs(s0).min(), k('log')[:, 0].max(), (q1 <= 0).any(1).sum(), (q1 >= 10).any(1).sum()))
    assert (d < 0.6).mean() >= 0.25 and np.abs(s0).min() < 1e-3 and k('log')[:, 0].max() > 0
    assert (q1 <= 0).any(1).sum() >= 8 and (q1 >= 10).any(1).sum() >= 8
    o = pro.PointReachBatched(S, n_objects=n, random_walk=True)
    o.state, o.s = k('state0').copy(), k('s0').copy()
    obs, r, ab, _ = o.step(k('action'), draws=k('draws'))
    e = max(np.abs(obs - k('state1')).max(), np.abs(o.s - k('s1')).max(), np.abs(r - k('reward')).max())
    print('n=%d: vectorised restatement against the reference, worst %.3e' % (n, e))
    assert e <= 1e-12 and not ab.any()
    assert np.abs(o.log_max - k('log')[:, 0]).max() <= 1e-12 and (k('log')[:, 1] == 0).all()
    for b in range(S):
        sc = pro.PointReachScalar(n_objects=n, random_walk=True)
        sc._state, sc.s = k('state0')[b].copy(), k('s0')[b].copy()
        o1, r1, _, _ = sc.step(k('action')[b], draws=k('draws')[b])
        assert max(np.abs(o1 - k('state1')[b]).max(), np.abs(sc.s - k('s1')[b]).max(), abs(r1 - k('reward')[b])) <= 1e-12, b
        assert abs(sc.constr_logs[-1][0] - k('log')[b, 0]) <= 1e-12
