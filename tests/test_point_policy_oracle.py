"""The restated policy loop of the collision-avoidance task (tests/point_policy_oracle.py) against the fixture recorded from
the reference's OWN networks driving its OWN PointReachAtacom (tests/golden/point_policy.npz, written by
profiles/tools/gen_point_policy_golden.py).  CPU only.

Bounds: 1e-12 on the actions (float64 modules against float64 numpy); on the env quantities the bounds of
tests/test_point_reach_oracle.py -- 1e-12 on observations and s, 1e-13 on the reward.  Every step is teacher-forced from the
recorded state.  The networks and the task are pinned; the exploration formulas are MushroomRL's and stay restated, unpinned.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_policy_oracle as ppo                 # noqa: E402
import point_reach_oracle as pro                  # noqa: E402

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'point_policy.npz'))


def _weights(p, tag):
    return [G['%s%s_%s%d' % (p, tag, w, i)] for i in (1, 2, 3) for w in ('W', 'b')]


@pytest.mark.parametrize('kind', ['ppo', 'sac', 'td3', 'ddpg'])
@pytest.mark.parametrize('n', [2, 4])
def test_restatement_reproduces_the_reference_fixture(n, kind):
    p = 'n%d_%s_' % (n, kind)
    S = int(G['steps'])
    assert G[p + 'state0'].shape == (S, 4 * (1 + n))
    scaling = G[p + 'action_scaling'] if kind in ('td3', 'ddpg') else 1.0
    pol = ppo.make_policy(kind, _weights(p, 'mu'), sigma_W=_weights(p, 'sigma') if kind == 'sac' else None, act_scale=scaling)
    env = pro.PointReachBatched(S, n_objects=n, random_walk=True)
    env.state, env.s = G[p + 'state0'].copy(), G[p + 's0'].copy()
    env.have_centres[:] = True
    env.t = np.arange(S)                          # step 0 is an episode start: DDPG's process restarts there
    env.episode[:] = 1
    if kind == 'ddpg':
        pol.x = G[p + 'x0'].copy()
        assert not G[p + 'x0'][0].any()
    a = ppo.draw(pol, env.state.copy(), G[p + 'noise'], env.t.copy())
    e_a = np.abs(a - G[p + 'action']).max()
    obs, r, ab, last = env.step(G[p + 'action'], draws=G[p + 'draws'])
    e_obs, e_s, e_r = np.abs(obs - G[p + 'state1']).max(), np.abs(env.s - G[p + 's1']).max(), np.abs(r - G[p + 'reward']).max()
    print('n=%d %s: action %.2e obs %.2e s %.2e reward %.2e' % (n, kind, e_a, e_obs, e_s, e_r))
    assert e_a <= 1e-12
    assert e_obs <= 1e-12 and e_s <= 1e-12 and e_r <= 1e-13
    assert not ab.any() and not last.any()
    if kind == 'td3':
        assert np.abs(G[p + 'action']).max() <= 1.0
    if kind == 'ddpg':                            # the recorded process: x before step t + 1 is x after step t
        np.testing.assert_allclose(pol.x[:-1], G[p + 'x0'][1:], rtol=0, atol=1e-15)


def test_closed_loop_restatement_follows_the_fixture_for_a_few_steps():
    """The free-running loop of point_policy_oracle.rollout from the fixture's first state, recorded noise and draws: the
    first steps stay at rounding level (the task's closed loop amplifies by about 10 x per 20 steps,
    tests/test_gpu_point_reach.py::test_facade_replays_a_fixture_episode)."""
    n, kind, K = 4, 'ppo', 10
    p = 'n%d_%s_' % (n, kind)
    pol = ppo.make_policy(kind, _weights(p, 'mu'))
    env = pro.PointReachBatched(1, n_objects=n, random_walk=True)
    env.state, env.s = G[p + 'state0'][:1].copy(), G[p + 's0'][:1].copy()
    env.have_centres[:] = True
    env.episode[:] = 1
    out = ppo.rollout(env, pol, K, G[p + 'noise'][:K, None], draws=G[p + 'draws'][:K, None])
    assert np.abs(out['action'][:, 0] - G[p + 'action'][:K]).max() <= 1e-12
    assert np.abs(out['next_obs'][:, 0] - G[p + 'state1'][:K]).max() <= 1e-12
