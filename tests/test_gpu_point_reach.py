"""GPU tests of the collision-avoidance task (libatacom_point.so) through its C ABI and Python classes, against the
float64 restatement (tests/point_reach_oracle.py) and the fixture recorded from the reference (tests/golden/point_reach.npz).

Stated bounds
  float64 build : 1e-8 on EVERY sample (the project's bound for float64 builds), teacher-forced; the fixture replay too.
  float32 build : random_walk=True -- every sample within 4 sens + 5e-6 (tests/parity_tools.SensitivityRecorder), with the
                  share of samples whose bound is vacuous capped at max_vacuous = 0.02 (the planar task's ceiling).
                  random_walk=False -- finiteness, and the decisions of the float64 build on the fixture's first episode.
"""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_reach_oracle as pro                 # noqa: E402
from parity_tools import SensitivityRecorder     # noqa: E402

DEV = 'cuda:0'
DT = {'f64': torch.float64, 'f32': torch.float32}
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'point_reach.npz'))
EP, TS = int(G['episodes']), int(G['episode_steps'])
F64_BOUND = 1e-8
MAX_VACUOUS = 0.02


def key(n, rw, name):
    return G['n%d_rw%d_%s' % (n, int(rw), name)]


def _env(B, n, rw, dt, **kw):
    from rl_on_manifold_amd import BatchedPointReachEnv
    return BatchedPointReachEnv(B, n_objects=n, random_walk=rw, device=DEV, dtype=DT[dt], **kw)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def spread_oracle(B, n, rw, seed, prefix):
    """A batched restatement whose environments were reset (generator draws) and then ran free for `prefix` steps under
    uniform actions: the states the task visits, at different phases of their episodes."""
    o = pro.PointReachBatched(B, n_objects=n, random_walk=rw, seed=seed)
    o.reset()
    rng = np.random.default_rng(seed + 1)
    for _ in range(prefix):
        o.step(rng.uniform(-1, 1, (B, 2)))
    o.get_constraints_logs()
    return o


def step_outputs(p, inputs):
    """What is compared per sample: the observation after the step, s after the step, the reward."""
    obs, r, _, _ = p.step(inputs[0], draws=inputs[1])
    return np.concatenate([obs, p.s, r[:, None]], 1)


def device_outputs(env, obs, r):
    n = env.n_objects
    s = _np(env.get_state())[:, 4 * (1 + n):4 * (1 + n) + n]
    return np.concatenate([_np(obs), s, _np(r)[:, None]], 1)


# ---------------------------------------------------------------------------------------------------- 4. float64
@pytest.mark.parametrize('draw_mode', ['supplied', 'generator'])
@pytest.mark.parametrize('rw', [True, False])
@pytest.mark.parametrize('n', [2, 4])
def test_float64_teacher_forced_against_the_restatement(n, rw, draw_mode):
    B, T = 1024, 40
    o = spread_oracle(B, n, rw, seed=11 + n, prefix=60)
    env = _env(B, n, rw, 'f64', seed=11 + n, auto_reset=False)
    rng = np.random.default_rng(5)
    worst = 0.0
    for t in range(T):
        env.set_state(o.get_state())
        a = rng.uniform(-1.2, 1.2, (B, 2))
        d = rng.uniform(-1, 1, (B, n, 2)) if draw_mode == 'supplied' else None
        obs, r, ab, info = env.step(a, draws=d)
        dev = device_outputs(env, obs, r)
        ref = step_outputs(o, (a, d))
        err = np.abs(dev - ref).max()
        worst = max(worst, err)
        assert err <= F64_BOUND, (t, err, np.unravel_index(np.abs(dev - ref).argmax(), dev.shape))
        assert not ab.any().item() and not info['last'].any().item()
    print('float64 n=%d random_walk=%s %s draws: worst |dev - restatement| = %.3e over %d samples' % (n, rw, draw_mode, worst, B * T))
    dl, ol = env.get_constraints_logs(), o.get_constraints_logs()
    assert abs(dl[0] - ol[0]) <= F64_BOUND and abs(dl[1] - ol[1]) <= F64_BOUND and dl[2] == 0.0


@pytest.mark.parametrize('rw', [True, False])
@pytest.mark.parametrize('n', [2, 4])
def test_float64_replays_the_reference_fixture(n, rw):
    """Every recorded step of the reference as one batch through atacom_point_set_state / atacom_point_step."""
    B = EP * TS
    env = _env(B, n, rw, 'f64', auto_reset=False)
    o = pro.PointReachBatched(B, n_objects=n, random_walk=rw)
    o.state = key(n, rw, 'state0').reshape(B, -1).copy()
    o.s = key(n, rw, 's0').reshape(B, -1).copy()
    o.centres[:] = key(n, rw, 'reset_draws')[0] - np.array([2.0, 0.0])      # the FIRST reset's, for all three episodes
    o.have_centres[:] = True
    o.time = np.tile(np.cumsum(np.r_[0.0, np.full(TS - 1, 0.01)]), EP)
    o.t = np.tile(np.arange(TS), EP)
    o.episode[:] = 1
    env.set_state(o.get_state())
    obs, r, ab, _ = env.step(key(n, rw, 'action').reshape(B, 2), draws=key(n, rw, 'draws').reshape(B, n, 2))
    dev = device_outputs(env, obs, r)
    ref = np.concatenate([key(n, rw, 'state1').reshape(B, -1), key(n, rw, 's1').reshape(B, -1), key(n, rw, 'reward').reshape(B, 1)], 1)
    err = np.abs(dev - ref)
    print('fixture n=%d random_walk=%s: worst |dev - reference| = %.3e' % (n, rw, err.max()))
    assert err.max() <= F64_BOUND, (err.max(), np.unravel_index(err.argmax(), err.shape))
    logs = env.get_constraints_logs()
    fl = key(n, rw, 'final_logs')
    assert abs(logs[0] - fl[0]) <= F64_BOUND and abs(logs[1] - fl[1]) <= F64_BOUND and logs[2] == fl[2] == 0.0


# ---------------------------------------------------------------------------------------------------- 5. float32
@pytest.mark.parametrize('n', [2, 4])
def test_float32_random_walk_every_sample_explained(n):
    B, T = 1024, 40
    o = spread_oracle(B, n, True, seed=23 + n, prefix=60)
    env = _env(B, n, True, 'f32', auto_reset=False)
    rec = SensitivityRecorder(step_outputs, seed=3, state_fields=('state', 's'))
    rng = np.random.default_rng(9)
    for t in range(T):
        env.set_state(o.get_state())
        a = rng.uniform(-1.2, 1.2, (B, 2))
        d = rng.uniform(-1, 1, (B, n, 2))
        obs, r, _, _ = env.step(a, draws=d)
        dev = device_outputs(env, obs, r)
        assert np.isfinite(dev).all()
        rec.record(o, (a, d), dev)
        o.step(a, draws=d)
    print(rec.finish('point reach n=%d random walk: %d envs x %d steps, HIP f32 vs restatement f64' % (n, B, T),
                     max_vacuous=MAX_VACUOUS))


def _decisions(dq0, dq1, dt=0.01):
    """Per axis: -1 / 0 / +1 = the acceleration clip low / inactive / high, read off the velocity update a = dq' - dq over
    10 dt (a saturated axis shows |a| = 1 to rounding: the class boundary sits at 1 - 1e-3), and the distance of |a| to that
    boundary."""
    a = (dq1 - dq0) / (10 * dt)
    return np.where(a >= 1 - 1e-3, 1, np.where(a <= -(1 - 1e-3), -1, 0)), np.abs(np.abs(a) - (1 - 1e-3))


@pytest.mark.parametrize('n', [2, 4])
def test_float32_circling_obstacles_finite_and_same_decisions(n):
    """random_walk=False in float32: its ill-conditioning after the jump of Q2 is the reference's own, so (a) a free run over
    two auto-resets stays finite, (b) on the fixture's first episode (before any jump) the float32 build takes the float64
    build's decisions -- the acceleration clip per axis -- wherever float64 is not within 5e-4 of the class boundary
    (float32 resolves the velocity update to about 1e-5)."""
    env = _env(512, n, False, 'f32', horizon=150, auto_reset=True, seed=2)
    env.reset()
    out = env.rollout(torch.rand((400, 512, 2), device=DEV) * 2.4 - 1.2)
    assert torch.isfinite(out['next_obs']).all().item() and torch.isfinite(out['reward']).all().item()
    assert np.isfinite(_np(env.get_state())).all()
    res = {}
    for dt in ('f32', 'f64'):
        e = _env(TS, n, False, dt, auto_reset=False)
        o = pro.PointReachBatched(TS, n_objects=n, random_walk=False)
        o.state, o.s = key(n, False, 'state0')[0].copy(), key(n, False, 's0')[0].copy()
        o.centres[:] = key(n, False, 'reset_draws')[0] - np.array([2.0, 0.0])
        o.have_centres[:] = True
        o.time, o.t = np.cumsum(np.r_[0.0, np.full(TS - 1, 0.01)]), np.arange(TS)
        o.episode[:] = 1
        e.set_state(o.get_state())
        obs, _, _, _ = e.step(key(n, False, 'action')[0])
        res[dt] = _decisions(key(n, False, 'state0')[0][:, 2:4], _np(obs)[:, 2:4])
    clear = res['f64'][1] > 5e-4
    assert clear.mean() > 0.9, clear.mean()
    assert (res['f32'][0][clear] == res['f64'][0][clear]).all()
    ref = _decisions(key(n, False, 'state0')[0][:, 2:4], key(n, False, 'state1')[0][:, 2:4])
    assert (res['f64'][0][clear] == ref[0][clear]).all()


# ---------------------------------------------------------------------------------------------------- 6. structure
@pytest.mark.parametrize('supplied', [False, True])
@pytest.mark.parametrize('rw', [True, False])
@pytest.mark.parametrize('n', [2, 4])
def test_rollout_equals_steps_bit_for_bit(n, rw, supplied):
    B, T = 300, 20                                                   # not a multiple of the block: the tail is exercised
    acts = torch.rand((T, B, 2), device=DEV) * 2.4 - 1.2
    draws = (torch.rand((T, B, n, 2), device=DEV) * 2 - 1) if supplied else None
    a = _env(B, n, rw, 'f32', horizon=7, auto_reset=True, seed=4)
    b = _env(B, n, rw, 'f32', horizon=7, auto_reset=True, seed=4)
    o0 = a.reset()
    assert torch.equal(o0, b.reset())
    out = a.rollout(acts, draws=draws)
    prev = o0
    for t in range(T):
        obs, r, ab, info = b.step(acts[t], draws=None if draws is None else draws[t])
        assert torch.equal(out['obs'][t], prev), t
        assert torch.equal(out['next_obs'][t], obs) and torch.equal(out['reward'][t], r), t
        assert torch.equal(out['absorbing'][t].bool(), ab) and torch.equal(out['last'][t].bool(), info['last']), t
        prev = b.get_state()[:, :4 * (1 + n)]                       # after an in-kernel reset: the reset state
    assert torch.equal(a.get_state(), b.get_state())
    assert a.get_constraints_logs() == b.get_constraints_logs()
    assert out['last'].sum().item() == B * (T // 7) and out['absorbing'].sum().item() == 0


@pytest.mark.parametrize('n', [2, 4])
def test_auto_reset_and_generator_match_the_restatement(n):
    """Free-running float64 with generator draws over two horizons: `last` at the horizon, never absorbing, the episode
    counter re-keys the draws (the reset positions are the restatement's BIT FOR BIT: 2 + 6 u is exact in float64), and the
    step draws are the restatement's draw for draw (recovered as 24-bit integers from the unclipped velocity updates)."""
    B, T, H = 256, 13, 5
    env = _env(B, n, True, 'f64', horizon=H, auto_reset=True, seed=77)
    o = pro.PointReachBatched(B, n_objects=n, random_walk=True, horizon=H, auto_reset=True, seed=77)
    obs0 = _np(env.reset())
    assert np.array_equal(obs0, o.reset())
    assert np.array_equal(obs0.reshape(B, 1 + n, 4)[:, 1:, 0:2], pro.generator_reset_draws(77, np.arange(B), np.zeros(B, dtype=int), n))
    rng = np.random.default_rng(1)
    acts = rng.uniform(-1.2, 1.2, (T, B, 2))
    out = env.rollout(acts)
    checked = 0
    for t in range(T):
        before = o.state.copy()
        ep, tt = o.episode - 1, o.t.copy()
        assert np.abs(_np(out['obs'][t]) - before).max() <= F64_BOUND
        if t % H == 0 and t > 0:                                      # the state after an in-kernel reset: exact draws
            ob = before.reshape(B, 1 + n, 4)[:, 1:, 0:2]
            assert np.array_equal(_np(out['obs'][t]).reshape(B, 1 + n, 4)[:, 1:, 0:2], ob)
            assert np.array_equal(ob, pro.generator_reset_draws(77, np.arange(B), np.full(B, t // H), n))
        obs, r, ab, last = o.step(acts[t])
        assert np.abs(_np(out['next_obs'][t]) - obs).max() <= F64_BOUND and np.abs(_np(out['reward'][t]) - r).max() <= F64_BOUND
        assert np.array_equal(_np(out['last'][t]) != 0, last) and last.all() == ((t + 1) % H == 0)
        assert out['absorbing'][t].sum().item() == 0
        # draw for draw: dp' = clip(+-dp + 10 u dt) -> u where nothing clipped and nothing flipped
        dp0 = before.reshape(B, 1 + n, 4)[:, 1:, 2:4]
        p1 = _np(out['next_obs'][t]).reshape(B, 1 + n, 4)[:, 1:, 0:2]
        dp1 = _np(out['next_obs'][t]).reshape(B, 1 + n, 4)[:, 1:, 2:4]
        ok = (np.abs(dp1) < 1) & (p1 > 2) & (p1 < 10)
        k_dev = np.rint(((dp1 - dp0) / 0.1 + 1) / 2 * 16777216.0)
        k_ref = np.rint((pro.generator_step_draws(77, np.arange(B), ep, tt, n) + 1) / 2 * 16777216.0)
        assert np.array_equal(k_dev[ok], k_ref[ok])
        checked += ok.sum()
    assert checked > 0.8 * T * B * n * 2
    assert np.abs(_np(env.get_state()) - o.get_state()).max() <= F64_BOUND
    dl, ol = env.get_constraints_logs(), o.get_constraints_logs()
    assert abs(dl[0] - ol[0]) <= F64_BOUND and abs(dl[1] - ol[1]) <= F64_BOUND and dl[2] == 0.0
    cleared = env.get_constraints_logs()
    assert np.isnan(cleared[0]) and cleared[1] == -np.inf and cleared[2] == 0.0


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_set_state_of_get_state_is_the_identity(dt):
    B, n = 200, 4
    a = _env(B, n, True, dt, seed=3)
    a.reset()
    acts = torch.rand((6, B, 2), device=DEV, dtype=DT[dt]) * 2 - 1
    a.rollout(acts[:3])
    st = a.get_state()
    b = _env(B, n, True, dt, seed=3)
    b.set_state(st)
    assert torch.equal(b.get_state(), st)
    a.set_state(st)
    assert torch.equal(a.get_state(), st)
    oa, ob = a.rollout(acts[3:]), b.rollout(acts[3:])
    for k in ('obs', 'next_obs', 'reward', 'last'):
        assert torch.equal(oa[k], ob[k]), k


FREE_RUN = 20


@pytest.mark.parametrize('rw', [True, False])
def test_facade_replays_a_fixture_episode(rw):
    """The batch-1 numpy facade, float64, over the fixture's first episode with the recorded draws: free-running for the
    first FREE_RUN steps, then every step from the recorded state.  The whole episode is not run free at 1e-8 because the
    task's closed loop amplifies rounding-order differences by about 10 x per 20 steps: the vectorised restatement against
    the line-by-line one (both float64, both within 1e-14 of the reference per step) is 1e-13 apart at step 20, 1.9e-9 at
    step 80 and 2e-5 at step 120 of this episode (n = 4, random walk)."""
    from rl_on_manifold_amd import PointReachAtacom
    n = 4
    mdp = PointReachAtacom(n_objects=n, random_walk=rw, device=DEV, dtype=torch.float64)
    assert mdp.info.observation_space.shape == (4 * (1 + n),) and mdp.info.action_space.shape == (2,)
    assert (mdp.info.observation_space.high == 10).all() and (mdp.info.action_space.low == -1).all()
    assert mdp.info.horizon == 1000 and mdp.info.gamma == 0.99
    st = mdp.reset(draws=key(n, rw, 'reset_draws')[0])
    assert np.abs(st - key(n, rw, 'reset_state')[0]).max() <= F64_BOUND
    assert np.abs(mdp.s - key(n, rw, 'reset_s')[0]).max() <= F64_BOUND
    st[0] = 123.0
    assert mdp.state[0] == 1.0                                       # copies out
    worst = 0.0
    for t in range(TS):
        if t >= FREE_RUN:
            full = _np(mdp._engine.get_state())
            full[0, :4 * (1 + n)], full[0, 4 * (1 + n):4 * (1 + n) + n] = key(n, rw, 'state0')[0, t], key(n, rw, 's0')[0, t]
            mdp._engine.set_state(full)
        obs, r, ab, info = mdp.step(key(n, rw, 'action')[0, t], draws=key(n, rw, 'draws')[0, t])
        worst = max(worst, np.abs(obs - key(n, rw, 'state1')[0, t]).max(), abs(r - key(n, rw, 'reward')[0, t]),
                    np.abs(mdp.s - key(n, rw, 's1')[0, t]).max())
        assert ab is False and info == {}
    print('facade random_walk=%s, %d steps: worst error %.3e' % (rw, TS, worst))
    assert worst <= F64_BOUND
    logs = mdp.get_constraints_logs()
    assert abs(logs[0] - key(n, rw, 'log')[0, :, 0].mean()) <= F64_BOUND
    assert abs(logs[1] - key(n, rw, 'log')[0, :, 0].max()) <= F64_BOUND and logs[2] == 0.0
    mdp.seed(3)
    mdp.stop()


def test_unsupported_obstacle_count_is_an_error():
    from rl_on_manifold_amd import AtacomError
    with pytest.raises(AtacomError, match='n_objects = 3'):
        _env(8, 3, True, 'f32')


def test_handles_of_both_libraries_alternate_on_one_stream():
    from rl_on_manifold_amd import BatchedAtacomEnv
    B, T, n = 512, 12, 4
    ac = torch.rand((T, B, 1), device=DEV) * 2 - 1
    ap = torch.rand((T, B, 2), device=DEV) * 2 - 1

    def circle():
        return BatchedAtacomEnv('circle', B, device=DEV, dtype=torch.float32)

    def point():
        e = _env(B, n, True, 'f32', seed=8)
        e.reset()
        return e

    c0, p0 = circle(), point()
    alone_c = [c0.step(ac[t])[0] for t in range(T)]
    alone_p = [p0.step(ap[t])[0] for t in range(T)]
    c1, p1 = circle(), point()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for t in range(T):
            oc = c1.step(ac[t])[0]
            op = p1.step(ap[t])[0]
            assert torch.equal(oc, alone_c[t]) and torch.equal(op, alone_p[t]), t
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(c1.get_state(), c0.get_state()) and torch.equal(p1.get_state(), p0.get_state())


def test_rollout_policy_is_the_host_loop():
    B, n = 128, 2
    env = _env(B, n, True, 'f32', seed=6, horizon=9)
    twin = _env(B, n, True, 'f32', seed=6, horizon=9)
    env.reset(), twin.reset()
    W = torch.randn((4 * (1 + n), 2), device=DEV) * 0.05

    def policy(obs):
        return torch.tanh(obs @ W)

    out = env.rollout_policy(policy, 12)
    ref = twin.rollout(out['action'])
    for k in ('obs', 'next_obs', 'reward', 'last'):
        assert torch.equal(out[k], ref[k]), k
    assert torch.equal(out['action'][3], policy(out['obs'][3]))
