#!/usr/bin/env python3
"""Capture tests/golden/point_reach.npz from the reference's OWN PointReachAtacom (runs only where the reference exists).

    python profiles/tools/gen_point_reach_golden.py --reference /path/to/rl_on_manifold

The reference is imported unchanged by its module path (examples/collision_avoidance_exp.py is un-importable as shipped,
the class is not); its MushroomRL dependency is satisfied by oracle/_mushroom_stub.  np.random.uniform is wrapped so that
every draw the reference makes is recorded; the fixture holds data only: per step the state before, the action, the draws,
s before and after, the state after, the reward and the constraint-log row, plus get_constraints_logs() at the end.
For each of n_objects in {2, 4} x random_walk in {True, False} ONE object is reset three times and stepped EPISODE_STEPS
times after each reset, so that the second and third episodes show what survives a reset (the circle centres of the
first one).  Re-running reproduces the committed file bit for bit (fixed seeds, plain np.savez).
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True

EPISODES, EPISODE_STEPS = 3, 120


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('ATACOM_REFERENCE'), help='checkout of the reference project')
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden', 'point_reach.npz'))
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        sys.exit('the reference checkout is needed: --reference PATH (or ATACOM_REFERENCE)')
    sys.path.insert(0, os.path.join(REPO, 'oracle', '_mushroom_stub'))
    sys.path.insert(0, args.reference)
    import matplotlib
    matplotlib.use('Agg')
    import numpy as np
    from atacom.environments.collision_avoidance.collision_avoidance_atacom import PointReachAtacom   # (reference)

    real_uniform = np.random.uniform
    drawn = []

    def recording_uniform(*a, **k):
        v = real_uniform(*a, **k)
        drawn.append(np.array(v, dtype=np.float64, copy=True))
        return v

    np.random.uniform = recording_uniform
    out = {'episodes': np.array(EPISODES), 'episode_steps': np.array(EPISODE_STEPS)}
    try:
        for n in (2, 4):
            for rw in (True, False):
                key = 'n%d_rw%d' % (n, int(rw))
                np.random.seed(1000 + 10 * n + int(rw))
                arng = np.random.default_rng(2000 + 10 * n + int(rw))
                env = PointReachAtacom(n_objects=n, random_walk=rw)
                rec = {k: [] for k in ('state0', 'action', 'draws', 's0', 's1', 'state1', 'reward', 'log')}
                reset_draws, reset_state, reset_s = [], [], []
                for ep in range(EPISODES):
                    del drawn[:]
                    env.reset()
                    reset_draws.append(np.array(drawn).reshape(n, 2))
                    reset_state.append(env._state.copy())
                    reset_s.append(env.s.copy())
                    for t in range(EPISODE_STEPS):
                        a = arng.uniform(-1.2, 1.2, 2)
                        rec['state0'].append(env._state.copy())
                        rec['s0'].append(env.s.copy())
                        rec['action'].append(a.copy())
                        del drawn[:]
                        obs, r, absorbing, _ = env.step(a.copy())
                        assert absorbing is False
                        rec['draws'].append(np.array(drawn).reshape(n, 2) if rw else np.zeros((n, 2)))
                        rec['s1'].append(env.s.copy())
                        rec['state1'].append(np.array(obs, copy=True))
                        rec['reward'].append(r)
                        rec['log'].append(np.array(env.constr_logs[-1], dtype=np.float64))
                assert len(env._obj_circle_center) == EPISODES * n
                for k, v in rec.items():
                    out[key + '_' + k] = np.array(v, dtype=np.float64).reshape((EPISODES, EPISODE_STEPS) + np.shape(v[0]))
                out[key + '_reset_draws'] = np.array(reset_draws)
                out[key + '_reset_state'] = np.array(reset_state)
                out[key + '_reset_s'] = np.array(reset_s)
                out[key + '_final_logs'] = np.array(env.get_constraints_logs(), dtype=np.float64)
    finally:
        np.random.uniform = real_uniform
    np.savez(args.out, **out)
    print('wrote %s (%d bytes)' % (args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
