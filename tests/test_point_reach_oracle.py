"""The float64 restatement of PointReachAtacom (tests/point_reach_oracle.py) against the fixture recorded from the
reference's own class (tests/golden/point_reach.npz, profiles/tools/gen_point_reach_golden.py).

Teacher-forced: every step starts from the fixture's recorded state, s and draws.  Tolerances are the circle's golden
replay's (tests/test_oracle_trajectories.py): 1e-12 on observations and s, 1e-13 on the reward, 1e-9 on the logs.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_reach_oracle as pro      # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'point_reach.npz'))
CASES = [(n, rw) for n in (2, 4) for rw in (True, False)]
EP, TS = int(G['episodes']), int(G['episode_steps'])


def key(n, rw, name):
    return G['n%d_rw%d_%s' % (n, int(rw), name)]


def centres_of_first_reset(n, rw):
    return key(n, rw, 'reset_draws')[0] - np.array([2.0, 0.0])


@pytest.mark.parametrize('n,rw', CASES)
def test_scalar_replays_fixture(n, rw):
    """One object, reset three times with the recorded reset draws, each step teacher-forced."""
    env = pro.PointReachScalar(n_objects=n, random_walk=rw)
    worst = {'obs': 0.0, 's': 0.0, 'reward': 0.0}
    for ep in range(EP):
        st = env.reset(draws=key(n, rw, 'reset_draws')[ep])
        np.testing.assert_allclose(st, key(n, rw, 'reset_state')[ep], rtol=0, atol=1e-12)
        np.testing.assert_allclose(env.s, key(n, rw, 'reset_s')[ep], rtol=0, atol=1e-12)
        for t in range(TS):
            env._state = key(n, rw, 'state0')[ep, t].copy()
            env.s = key(n, rw, 's0')[ep, t].copy()
            obs, r, ab, _ = env.step(key(n, rw, 'action')[ep, t], draws=key(n, rw, 'draws')[ep, t])
            worst['obs'] = max(worst['obs'], np.abs(obs - key(n, rw, 'state1')[ep, t]).max())
            worst['s'] = max(worst['s'], np.abs(env.s - key(n, rw, 's1')[ep, t]).max())
            worst['reward'] = max(worst['reward'], abs(r - key(n, rw, 'reward')[ep, t]))
            np.testing.assert_allclose(env.constr_logs[-1], key(n, rw, 'log')[ep, t], rtol=0, atol=1e-12)
            assert ab is False
    print('n=%d random_walk=%s worst errors %s' % (n, rw, worst))
    assert worst['obs'] <= 1e-12 and worst['s'] <= 1e-12 and worst['reward'] <= 1e-13, worst
    assert len(env._obj_circle_center) == EP * n                          # Q1: never cleared
    np.testing.assert_allclose(env.get_constraints_logs(), key(n, rw, 'final_logs'), rtol=0, atol=1e-9)
    assert env.constr_logs == []


@pytest.mark.parametrize('n,rw', CASES)
def test_batched_replays_fixture(n, rw):
    """All recorded steps of a case as ONE batch (environment = recorded step): the vectorised arithmetic."""
    B = EP * TS
    env = pro.PointReachBatched(B, n_objects=n, random_walk=rw)
    env.state = key(n, rw, 'state0').reshape(B, -1).copy()
    env.s = key(n, rw, 's0').reshape(B, -1).copy()
    env.centres[:] = centres_of_first_reset(n, rw)                       # Q1
    env.have_centres[:] = True
    env.time = np.tile(np.cumsum(np.r_[0.0, np.full(TS - 1, 0.01)]), EP)   # _time as the reference accumulates it
    env.t = np.tile(np.arange(TS), EP)
    obs, r, ab, last = env.step(key(n, rw, 'action').reshape(B, 2), draws=key(n, rw, 'draws').reshape(B, n, 2))
    e_obs = np.abs(obs - key(n, rw, 'state1').reshape(B, -1)).max()
    e_s = np.abs(env.s - key(n, rw, 's1').reshape(B, -1)).max()
    e_r = np.abs(r - key(n, rw, 'reward').reshape(B)).max()
    print('n=%d random_walk=%s batched: obs %.2e s %.2e reward %.2e' % (n, rw, e_obs, e_s, e_r))
    assert e_obs <= 1e-12 and e_s <= 1e-12 and e_r <= 1e-13
    assert not ab.any() and not last.any()
    np.testing.assert_allclose(env.get_constraints_logs(), key(n, rw, 'final_logs'), rtol=0, atol=1e-9)
    assert env.log_cnt.sum() == 0 and np.isneginf(env.log_max).all()     # cleared


@pytest.mark.parametrize('n,rw', CASES)
def test_scalar_and_batched_agree_free_running(n, rw):
    """Both classes, free-running from the same reset with the same draws (no teacher forcing), three resets."""
    sc = pro.PointReachScalar(n_objects=n, random_walk=rw)
    ba = pro.PointReachBatched(1, n_objects=n, random_walk=rw)
    for ep in range(EP):
        d = key(n, rw, 'reset_draws')[ep]
        np.testing.assert_array_equal(sc.reset(draws=d), ba.reset(draws=d[None])[0])
        for t in range(40):
            a, dr = key(n, rw, 'action')[ep, t], key(n, rw, 'draws')[ep, t]
            o1, r1, _, _ = sc.step(a, draws=dr)
            o2, r2, _, _ = ba.step(a[None], draws=dr[None])
            np.testing.assert_allclose(o2[0], o1, rtol=0, atol=1e-9)
            np.testing.assert_allclose(ba.s[0], sc.s, rtol=0, atol=1e-9)
            assert abs(r1 - r2[0]) <= 1e-9
    np.testing.assert_allclose(ba.get_constraints_logs(), sc.get_constraints_logs(), rtol=0, atol=1e-9)


@pytest.mark.parametrize('n', (2, 4))
def test_first_reset_centres_survive_later_resets(n):
    """Q1 + Q2: with random_walk=False the first step of EVERY episode puts the obstacles on the circles of the FIRST
    reset (its draws minus (2, 0)), whatever the later resets drew, and the drawn positions are overwritten (a jump)."""
    c0 = centres_of_first_reset(n, False)
    for ep in range(EP):
        after = key(n, False, 'state1')[ep, 0].reshape(1 + n, 4)[1:]
        np.testing.assert_allclose(after[:, 0:2], c0 + np.array([2.0, 0.0]), rtol=0, atol=1e-12)   # time 0: centre + 2 (1, 0)
        np.testing.assert_allclose(after[:, 2:4], np.tile([0.0, 4 * np.pi], (n, 1)), rtol=0, atol=1e-12)
        if ep > 0:
            drawn = key(n, False, 'reset_draws')[ep]
            assert np.abs(drawn - after[:, 0:2]).max() > 0.1              # the jump
    # the restatement does the same when it free-runs over the resets
    env = pro.PointReachBatched(1, n_objects=n, random_walk=False)
    for ep in range(EP):
        env.reset(draws=key(n, False, 'reset_draws')[ep][None])
        np.testing.assert_allclose(env.centres[0], c0, rtol=0, atol=0)
        obs, _, _, _ = env.step(np.zeros((1, 2)))
        np.testing.assert_allclose(obs[0].reshape(1 + n, 4)[1:, 0:2], c0 + np.array([2.0, 0.0]), rtol=0, atol=1e-12)


def test_generator_draws_are_keyed_by_env_episode_and_draw():
    """The draws of the generator mode: distinct per (env, episode, step, obstacle, coordinate), inside their ranges,
    and the scalar class (env_index b) draws what row b of the batched class draws."""
    n = 4
    ba = pro.PointReachBatched(8, n_objects=n, random_walk=True, seed=5)
    ba.reset()
    sc = pro.PointReachScalar(n_objects=n, random_walk=True, seed=5, env_index=3)
    np.testing.assert_array_equal(sc.reset(), ba.state[3])
    assert ((ba._p() >= 2) & (ba._p() < 8)).all()
    a = np.zeros((8, 2))
    for t in range(5):
        o, _, _, _ = ba.step(a)
        o1, _, _, _ = sc.step(a[0])
        np.testing.assert_allclose(o[3], o1, rtol=0, atol=1e-10)
    d0 = pro.generator_step_draws(5, np.arange(8), np.zeros(8, dtype=int), np.zeros(8, dtype=int), n)
    d1 = pro.generator_step_draws(5, np.arange(8), np.ones(8, dtype=int), np.zeros(8, dtype=int), n)
    assert len(np.unique(np.concatenate([d0.ravel(), d1.ravel()]))) == 2 * 8 * n * 2
    assert (np.abs(d0) <= 1).all()
