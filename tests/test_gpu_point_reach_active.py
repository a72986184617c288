"""GPU tests of the collision-avoidance kernels (k_point_step, k_point_rollout, k_point_rollout_mlp) WHERE THE CONSTRAINTS
BIND: the constraint-active states of tests/point_reach_cases.py (agent at or inside an obstacle's boundary d = 0.6, slack s
down to 1e-4, steps onto the walls at 0 and at 10, both clip states of the acceleration, a positive constraint log), which
tests/test_point_reach_active_oracle.py holds to that purpose on the CPU.  tests/test_gpu_point_reach.py covers the states
the task visits from its reset corner, where every obstacle is more than 1.4 away.

Teacher-forced like the existing tests: set_state from the restatement before every step, B = 1024, n in {2, 4}.

Stated bounds
  float64 build : 1e-8 on EVERY sample against the restatement (observation, s, reward), supplied and generator draws; the
                  fixture of the reference's own class (tests/golden/point_reach_active.npz) as one batch; the logs.
  float32 build : every sample within 4 sens + 5e-6 (tests/parity_tools.SensitivityRecorder, its constants unchanged), the
                  vacuous share capped at the 0.02 of tests/test_gpu_point_reach.py; the wall-flip and clip decisions of the
                  float64 build; the constraint log within a bound derived from float32's epsilon.
  structure     : equalities, bit for bit, float32, from active states.
"""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_reach_cases as prc                                      # noqa: E402
import point_reach_oracle as pro                                     # noqa: E402
from parity_tools import C_SENS, FLOOR, VACUOUS, SensitivityRecorder # noqa: E402
from point_reach_cases import step_outputs                           # noqa: E402
from test_gpu_point_reach import DEV, F64_BOUND, MAX_VACUOUS, _env, _np, device_outputs      # noqa: E402

assert MAX_VACUOUS == prc.MAX_VACUOUS                                # the ceiling the CPU tests checked is the existing one
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'point_reach_active.npz'))
B, T = prc.B_ACTIVE, prc.T_ACTIVE
EPS32 = float(np.finfo(np.float32).eps)


# ---------------------------------------------------------------------------------------------------- float64
@pytest.mark.parametrize('draw_mode', ['supplied', 'generator'])
@pytest.mark.parametrize('n', [2, 4])
def test_float64_teacher_forced_on_active_states(n, draw_mode):
    seed = prc.SEEDS[n]
    o = prc.active_oracle(B, n, seed)
    acts, draws = prc.forced_inputs(n, seed)
    env = _env(B, n, True, 'f64', seed=seed, auto_reset=False)
    worst = 0.0
    for t in range(T):
        env.set_state(o.get_state())
        d = draws[t] if draw_mode == 'supplied' else None
        obs, r, ab, info = env.step(acts[t], draws=d)
        dev = device_outputs(env, obs, r)
        ref = step_outputs(o, (acts[t], d))
        err = np.abs(dev - ref)
        worst = max(worst, err.max())
        assert err.max() <= F64_BOUND, (t, err.max(), np.unravel_index(err.argmax(), err.shape))
        assert not ab.any().item() and not info['last'].any().item()
    print('float64 active n=%d %s draws: worst |dev - restatement| = %.3e over %d samples' % (n, draw_mode, worst, B * T))
    dl, ol = env.get_constraints_logs(), o.get_constraints_logs()
    print('float64 active n=%d %s draws: log device %s restatement %s' % (n, draw_mode, dl, ol))
    assert abs(dl[0] - ol[0]) <= F64_BOUND and abs(dl[1] - ol[1]) <= F64_BOUND and dl[2] == 0.0
    assert dl[1] > 0 and ol[1] > 0                                   # a violated constraint went through the log


@pytest.mark.parametrize('n', [2, 4])
def test_float64_replays_the_active_fixture(n):
    """Every recorded step of the reference's own class from a constraint-active state, as one batch."""
    S = int(G['states'])
    k = lambda name: G['n%d_%s' % (n, name)]                         # noqa: E731
    env = _env(S, n, True, 'f64', auto_reset=False)
    o = pro.PointReachBatched(S, n_objects=n, random_walk=True)
    o.state, o.s = k('state0').copy(), k('s0').copy()
    o.have_centres[:] = True
    o.episode[:] = 1
    env.set_state(o.get_state())
    obs, r, ab, _ = env.step(k('action'), draws=k('draws'))
    dev = device_outputs(env, obs, r)
    ref = np.concatenate([k('state1'), k('s1'), k('reward')[:, None]], 1)
    err = np.abs(dev - ref)
    print('active fixture n=%d: worst |dev - reference| = %.3e' % (n, err.max()))
    assert err.max() <= F64_BOUND, (err.max(), np.unravel_index(err.argmax(), err.shape))
    assert not ab.any().item()
    logs = env.get_constraints_logs()
    assert abs(logs[0] - k('log')[:, 0].mean()) <= F64_BOUND and abs(logs[1] - k('log')[:, 0].max()) <= F64_BOUND
    assert logs[1] > 0 and logs[2] == 0.0


# ---------------------------------------------------------------------------------------------------- float32
@functools.lru_cache(maxsize=None)
def _forced_run(n):
    """The float32 AND the float64 build through the same teacher-forced window (supplied draws), once per n: per step the
    restatement's state before it, its outputs, both devices' outputs; the recorder of the float32 errors; the logs."""
    seed = prc.SEEDS[n]
    o = prc.active_oracle(B, n, seed)
    acts, draws = prc.forced_inputs(n, seed)
    e32 = _env(B, n, True, 'f32', auto_reset=False)
    e64 = _env(B, n, True, 'f64', auto_reset=False)
    rec = SensitivityRecorder(step_outputs, seed=3, state_fields=('state', 's'))
    run = {'state0': [], 'ref': [], 'f32': [], 'f64': [], 'rec': rec}
    for t in range(T):
        dev = {}
        for name, env in (('f32', e32), ('f64', e64)):
            env.set_state(o.get_state())
            obs, r, _, _ = env.step(acts[t], draws=draws[t])
            dev[name] = device_outputs(env, obs, r)
            run[name].append(dev[name])
        assert np.isfinite(dev['f32']).all()
        run['state0'].append(o.state.copy())
        run['ref'].append(rec.record(o, (acts[t], draws[t]), dev['f32']))
        o.step(acts[t], draws=draws[t])
    for k in ('state0', 'ref', 'f32', 'f64'):
        run[k] = np.array(run[k])
    run['logs'] = {'f32': e32.get_constraints_logs(), 'f64': e64.get_constraints_logs(), 'ref': o.get_constraints_logs()}
    return run


@pytest.mark.parametrize('n', [2, 4])
def test_float32_active_every_sample_explained(n):
    rec = _forced_run(n)['rec']
    print(rec.finish('point reach ACTIVE n=%d random walk: %d envs x %d steps, HIP f32 vs restatement f64' % (n, B, T),
                     max_vacuous=MAX_VACUOUS))


@pytest.mark.parametrize('n', [2, 4])
def test_float32_takes_the_float64_decisions_on_active_states(n):
    """The two decisions of base:45-54 -- the acceleration clip per axis and the agent's wall flip -- of the float32 build
    equal the float64 build's (and the restatement's) wherever float64 is clear of the decision's boundary.

    Flip.  The decision is on q' = q + dq dt against 0 and 10.  float32 rounds q (|q| < 16: half an ulp, 4.8e-7 at most) and
    the sum (as much again), 1e-6 together, and the margin is fifty times that, 5e-5 -- the factor of the existing
    tests/test_gpu_point_reach._decisions (5e-4 for a resolution of 1e-5).  A build flipped when its new velocity is nearer
    to -v than to v, v = the restatement's velocity before the flip.  That reading needs the build's velocity within |v| of
    the restatement's: it is taken where |v| > 0.05 on samples whose sensitivity bound is not vacuous, where an explained
    float32 velocity is within 1e-2 max(1, |v|) < 0.03 (|v| <= 3 here, asserted).

    Clip.  Read as in _decisions off the velocity update a = (dq' - dq) / (10 dt), the flip undone; a saturated axis shows
    |a| = 1 to rounding and the class boundary sits at 1 - 1e-3.  float32 resolves dq' and dq to eps32 |dq| / 2 each, |dq| <= 3:
    a to 3 eps32 / 0.1 = 4e-6, below the 1e-5 of the existing test, whose margin of 5e-4 is kept.

    More than 0.9 of the axes must be clear for either decision."""
    run = _forced_run(n)
    dq0, q1, dq1r = run['state0'][:, :, 2:4], run['ref'][:, :, 0:2], run['ref'][:, :, 2:4]
    assert np.abs(dq0).max() <= 3 and np.abs(dq1r).max() <= 3 and np.abs(q1).max() < 16
    flip_ref = (q1 <= 0) | (q1 >= 10)
    v = np.where(flip_ref, -dq1r, dq1r)
    wall_clear = np.minimum(np.abs(q1), np.abs(q1 - 10)) > 5e-5
    told = (C_SENS * np.array(run['rec'].sens) + FLOOR <= VACUOUS)[:, :, None]
    clear = wall_clear & (np.abs(v) > 0.05) & told
    flipped = {k: np.abs(run[k][:, :, 2:4] + v) < np.abs(run[k][:, :, 2:4] - v) for k in ('f32', 'f64')}
    at0, at10 = int((flip_ref & clear & (q1 <= 0)).sum()), int((flip_ref & clear & (q1 >= 10)).sum())
    print('decisions n=%d: flip clear on %.4f of %d axes, %d flips at 0 and %d at 10 among them' % (n, clear.mean(), clear.size, at0, at10))
    assert clear.mean() > 0.9, clear.mean()
    assert at0 >= 10 and at10 >= 10
    assert (flipped['f64'][clear] == flip_ref[clear]).all(), np.argwhere(clear & (flipped['f64'] != flip_ref))[:10]
    assert (flipped['f32'][clear] == flipped['f64'][clear]).all(), np.argwhere(clear & (flipped['f32'] != flipped['f64']))[:10]
    # the acceleration clip (the flip undone with the restatement's decision, on axes clear of the walls)
    res = {k: prc.clip_state(dq0, flip_ref, run[k][:, :, 2:4], boundary=1 - 1e-3) for k in ('ref', 'f32', 'f64')}
    cls = {k: res[k][0] for k in res}
    clear = (np.abs(np.abs(res['f64'][1]) - (1 - 1e-3)) > 5e-4) & wall_clear
    print('decisions n=%d: clip clear on %.4f of %d axes, float64 classes low / inactive / high among them %s' % (
        n, clear.mean(), clear.size, [int((cls['f64'][clear] == c).sum()) for c in (-1, 0, 1)]))
    assert clear.mean() > 0.9, clear.mean()
    assert min((cls['ref'][clear] == c).mean() for c in (-1, 0, 1)) >= 0.10            # every class is compared
    assert (cls['f64'][clear] == cls['ref'][clear]).all(), np.argwhere(clear & (cls['f64'] != cls['ref']))[:10]
    assert (cls['f32'][clear] == cls['f64'][clear]).all(), np.argwhere(clear & (cls['f32'] != cls['f64']))[:10]


@pytest.mark.parametrize('n', [2, 4])
def test_float32_constraint_log_on_active_states(n):
    """Mean and maximum of the float32 build's constraint log (max_i 0.36 - d_i^2 before every step) against the
    restatement's.  With X the largest |coordinate| and D the largest agent-obstacle distance of the batch (both from the
    restatement), eps = 2^-23: set_state rounds every coordinate by eps X / 2 at most, so a component of d = q - p carries
    eps X from its inputs and eps D / 2 from the subtraction; d^2 = dx^2 + dy^2 then errs by at most
    2 (|dx| + |dy|) eps (X + D / 2) + 2 eps D^2 <= eps (2 sqrt(2) D (X + D / 2) + 2 D^2), and 0.36 - d^2 adds eps D^2 / 2:
        tol_max  = eps (2 sqrt(2) D (X + D / 2) + 2.5 D^2)          about 5 eps D^2, 6e-5 at D = 10
    (the maximum over samples and the maximum over obstacles move by no more than their arguments do).  The mean goes
    through a float32 sum of T terms per environment (then double): each addition rounds a partial sum of at most T D^2 by
    eps / 2, T eps T D^2 / 2 per environment and T times less per term:
        tol_mean = tol_max + eps T D^2 / 2
    The float64 build's log is within 1e-8 (test_float64_teacher_forced_on_active_states)."""
    run = _forced_run(n)
    st = run['state0']
    q, p = st[:, :, None, 0:2], st[:, :, 4:].reshape(T, B, n, 4)[:, :, :, 0:2]
    X, Dm = np.abs(st.reshape(T, B, 1 + n, 4)[:, :, :, 0:2]).max(), np.sqrt(((q - p) ** 2).sum(3).max())
    tol_max = EPS32 * (2 * np.sqrt(2) * Dm * (X + Dm / 2) + 2.5 * Dm ** 2)
    tol_mean = tol_max + EPS32 * T * Dm ** 2 / 2
    dl, ol = run['logs']['f32'], run['logs']['ref']
    print('float32 log n=%d: device (%.7f, %.7f) restatement (%.7f, %.7f): |mean| off %.2e (tol %.2e), |max| off %.2e (tol %.2e)'
          % (n, dl[0], dl[1], ol[0], ol[1], abs(dl[0] - ol[0]), tol_mean, abs(dl[1] - ol[1]), tol_max))
    assert ol[1] > 0 and dl[1] > 0
    assert abs(dl[1] - ol[1]) <= tol_max and abs(dl[0] - ol[0]) <= tol_mean and dl[2] == 0.0
    assert abs(run['logs']['f64'][0] - ol[0]) <= F64_BOUND and abs(run['logs']['f64'][1] - ol[1]) <= F64_BOUND


# ---------------------------------------------------------------------------------------------------- structure
HORIZON_AT = 5                     # active_oracle leaves every environment at t = 20: the horizon falls inside the window


def _active_state(n, B_, seed):
    o = prc.active_oracle(B_, n, seed)
    assert (o.t == 20).all()
    return torch.tensor(o.get_state(), device=DEV, dtype=torch.float32)


@pytest.mark.parametrize('supplied', [False, True])
@pytest.mark.parametrize('n', [2, 4])
def test_rollout_equals_steps_from_active_states(n, supplied):
    """k_point_rollout over T steps against T launches of k_point_step, bit for bit, from constraint-active states: agents
    that flip at the walls at 0 and at 10, and the horizon reset of every environment after HORIZON_AT steps."""
    B_ = 1000                                                        # not a multiple of the block
    st = _active_state(n, B_, prc.SEEDS[n] + 1)
    acts = torch.rand((T, B_, 2), device=DEV) * 2.4 - 1.2
    draws = (torch.rand((T, B_, n, 2), device=DEV) * 2 - 1) if supplied else None
    a = _env(B_, n, True, 'f32', horizon=20 + HORIZON_AT, auto_reset=True, seed=4)
    b = _env(B_, n, True, 'f32', horizon=20 + HORIZON_AT, auto_reset=True, seed=4)
    a.set_state(st), b.set_state(st)
    out = a.rollout(acts, draws=draws)
    prev = st[:, :4 * (1 + n)]
    for t in range(T):
        obs, r, ab, info = b.step(acts[t], draws=None if draws is None else draws[t])
        assert torch.equal(out['obs'][t], prev), t
        assert torch.equal(out['next_obs'][t], obs) and torch.equal(out['reward'][t], r), t
        assert torch.equal(out['absorbing'][t].bool(), ab) and torch.equal(out['last'][t].bool(), info['last']), t
        prev = b.get_state()[:, :4 * (1 + n)]
    assert torch.equal(a.get_state(), b.get_state())
    assert a.get_constraints_logs() == b.get_constraints_logs()
    q1 = out['next_obs'][:HORIZON_AT, :, 0:2]
    assert (q1 <= 0).sum().item() >= 10 and (q1 >= 10).sum().item() >= 10          # flips at both walls before the reset
    assert torch.equal(out['last'].sum(1).cpu(), torch.tensor([B_ if t == HORIZON_AT - 1 else 0 for t in range(T)]))
    assert torch.isfinite(out['next_obs']).all().item()


@pytest.mark.parametrize('n', [2, 4])
def test_set_state_of_get_state_is_the_identity_on_active_states(n):
    st = _active_state(n, 777, prc.SEEDS[n] + 2)
    a, b = _env(777, n, True, 'f32', auto_reset=False), _env(777, n, True, 'f32', auto_reset=False)
    a.set_state(st)
    got = a.get_state()
    assert torch.equal(got, st)
    b.set_state(got)
    assert torch.equal(b.get_state(), st)
    acts = torch.rand((4, 777, 2), device=DEV) * 2 - 1
    oa, ob = a.rollout(acts), b.rollout(acts)
    for k in ('obs', 'next_obs', 'reward', 'last'):
        assert torch.equal(oa[k], ob[k]), k
    a.set_state(a.get_state())
    assert torch.equal(a.get_state(), b.get_state())


@pytest.mark.parametrize('n,kind', [(2, 'sac'), (4, 'td3')])
def test_policy_rollout_env_part_from_active_states(n, kind):
    """The environment part of k_point_rollout_mlp against k_point_rollout on the actions it recorded, bit for bit, both
    started from constraint-active states by set_state (one policy kind per n: the full matrix of
    tests/test_gpu_point_policy.py starts from reset states)."""
    from test_gpu_point_policy import _assert_env_part_equal, _inputs, _pair
    B_ = 1000
    st = _active_state(n, B_, prc.SEEDS[n] + 3)
    env = _env(B_, n, True, 'f32', horizon=20 + HORIZON_AT, auto_reset=True, seed=6)
    twin = _env(B_, n, True, 'f32', horizon=20 + HORIZON_AT, auto_reset=True, seed=6)
    env.set_state(st), twin.set_state(st)
    dev, _ = _pair(kind, n)
    noise, draws = _inputs(B_, n, 'f32', True, seed=11, steps=T)
    out = env.rollout_policy(dev, T, noise=noise, draws=draws)
    assert torch.equal(out['obs'][0], st[:, :4 * (1 + n)])
    assert torch.isfinite(out['action']).all().item() and out['last'].sum().item() == B_
    q1 = out['next_obs'][:HORIZON_AT, :, 0:2]
    assert (q1 <= 0).any().item() and (q1 >= 10).any().item()
    _assert_env_part_equal(out, env, twin, draws)
