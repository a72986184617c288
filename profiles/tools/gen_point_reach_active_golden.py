#!/usr/bin/env python3
"""Capture tests/golden/point_reach_active.npz: ONE step of the reference's OWN PointReachAtacom from each of 256
constraint-active states per n_objects in {2, 4}, random walk (runs only where the reference exists).

    python profiles/tools/gen_point_reach_active_golden.py --reference /path/to/rl_on_manifold

The states come from tests/point_reach_cases.fixture_states (the float64 restatement, no device): the agent at or inside
the boundary of an obstacle, the smallest slacks of the pool, steps onto the walls at 0 and at 10.  The reference is imported unchanged by its module path, as
profiles/tools/gen_point_reach_golden.py does; for every state one object's _state and s are SET, the object is stepped
once under a recorded action, and np.random.uniform is wrapped so that the draws it makes are recorded.  The fixture holds
data only: state0, s0, action, draws, state1, s1, reward and the constraint-log row.  Re-running reproduces the
committed file bit for bit (fixed seeds, plain np.savez).
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('ATACOM_REFERENCE'), help='checkout of the reference project')
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden', 'point_reach_active.npz'))
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        sys.exit('the reference checkout is needed: --reference PATH (or ATACOM_REFERENCE)')
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    sys.path.insert(0, os.path.join(REPO, 'oracle', '_mushroom_stub'))
    sys.path.insert(0, args.reference)
    import matplotlib
    matplotlib.use('Agg')
    import numpy as np
    from atacom.environments.collision_avoidance.collision_avoidance_atacom import PointReachAtacom   # (reference)
    import point_reach_cases as prc

    real_uniform = np.random.uniform
    drawn = []

    def recording_uniform(*a, **k):
        v = real_uniform(*a, **k)
        drawn.append(np.array(v, dtype=np.float64, copy=True))
        return v

    STATES, SEED = prc.FIXTURE_STATES, prc.FIXTURE_SEEDS
    out = {'states': np.array(STATES)}
    for n in (2, 4):
        state0, s0 = prc.fixture_states(n)                      # before np.random.uniform is wrapped: draws of its own rng
        arng = np.random.default_rng(SEED[n] + 1000)
        np.random.seed(SEED[n] + 2000)
        rec = {k: [] for k in ('state0', 's0', 'action', 'draws', 'state1', 's1', 'reward', 'log')}
        np.random.uniform = recording_uniform
        try:
            env = PointReachAtacom(n_objects=n, random_walk=True)
            env.reset()
            for b in range(STATES):
                a = arng.uniform(-1.2, 1.2, 2)
                env._state = state0[b].copy()
                env.s = s0[b].copy()
                rec['state0'].append(env._state.copy())
                rec['s0'].append(env.s.copy())
                rec['action'].append(a.copy())
                del drawn[:]
                obs, r, absorbing, _ = env.step(a.copy())
                assert absorbing is False
                rec['draws'].append(np.array(drawn).reshape(n, 2))
                rec['state1'].append(np.array(obs, copy=True))
                rec['s1'].append(env.s.copy())
                rec['reward'].append(r)
                rec['log'].append(np.array(env.constr_logs[-1], dtype=np.float64))
        finally:
            np.random.uniform = real_uniform
        for k, v in rec.items():
            out['n%d_%s' % (n, k)] = np.array(v, dtype=np.float64)
    np.savez(args.out, **out)
    print('wrote %s (%d bytes)' % (args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
