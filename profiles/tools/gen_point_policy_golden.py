#!/usr/bin/env python3
"""Capture tests/golden/point_policy.npz: the reference's OWN actor networks driving its OWN PointReachAtacom (runs only
where the reference exists; no test imports this file).

    python profiles/tools/gen_point_policy_golden.py --reference /path/to/rl_on_manifold

The reference's examples/network.py (PPONetwork, SACActorNetwork, TD3ActorNetwork, DDPGActorNetwork at the task's shapes,
n_features [64, 64]) and atacom/environments/collision_avoidance are imported unchanged; MushroomRL is satisfied by
oracle/_mushroom_stub.  The modules are cast to float64 (.double()); their forward() calls `state.float()`, so the state is
handed over as a tensor subclass whose float() keeps float64 -- the arithmetic is the modules' own.  For n_objects in {2, 4}
and each of the four agents one environment (random_walk=True) is reset and driven for STEPS steps with recorded noise and
obstacle draws (np.random.uniform is wrapped).  Per step the file holds the state and slack before, the noise, the draws,
the OU state before (DDPG), the action, the state and slack after and the reward; plus the weights and action_scaling.
Data only.  The observation normalisation (MinMaxPreprocessor of the task's bounds +-10) and the exploration formulas are
MushroomRL's: they are restated here as in tests/policy_explore_oracle.py and stay UNPINNED; the fixture pins the networks
and the task.  Re-running reproduces the committed file (fixed seeds).
"""
import argparse
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True

STEPS = 40
PPO_STD, TD3_SIGMA, DDPG_SIGMA, THETA, OU_DT = 0.5, 0.25, 0.2, 0.15, 1e-2     # examples/collision_avoidance_exp.py:23,147,223-225


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('ATACOM_REFERENCE'), help='checkout of the reference project')
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden', 'point_policy.npz'))
    args = ap.parse_args()
    if not args.reference or not os.path.isdir(args.reference):
        sys.exit('the reference checkout is needed: --reference PATH (or ATACOM_REFERENCE)')
    sys.path.insert(0, os.path.join(REPO, 'oracle', '_mushroom_stub'))
    sys.path.insert(0, args.reference)
    import matplotlib
    matplotlib.use('Agg')
    import numpy as np
    import torch
    from atacom.environments.collision_avoidance.collision_avoidance_atacom import PointReachAtacom   # (reference)
    spec = importlib.util.spec_from_file_location('ref_network', os.path.join(args.reference, 'examples', 'network.py'))
    net_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(net_mod)

    class F64State(torch.Tensor):
        def float(self):
            return torch.Tensor.double(self).as_subclass(torch.Tensor)

    def forward(net, x):
        with torch.no_grad():
            return net(torch.from_numpy(np.asarray(x, dtype=np.float64)[None]).as_subclass(F64State)).numpy()[0].astype(np.float64)

    real_uniform = np.random.uniform
    drawn = []

    def recording_uniform(*a, **k):
        v = real_uniform(*a, **k)
        drawn.append(np.array(v, dtype=np.float64, copy=True))
        return v

    np.random.uniform = recording_uniform
    out = {'steps': np.array(STEPS)}
    try:
        for n in (2, 4):
            D = 4 * (1 + n)
            for kind in ('ppo', 'sac', 'td3', 'ddpg'):
                p = 'n%d_%s_' % (n, kind)
                torch.manual_seed(31 * n + len(kind))
                np.random.seed(500 + 10 * n + len(kind))
                rng = np.random.default_rng(700 + 10 * n + len(kind))
                scaling = np.ones(2)                                   # (action_space.high - action_space.low) / 2
                cls = {'ppo': net_mod.PPONetwork, 'sac': net_mod.SACActorNetwork, 'td3': net_mod.TD3ActorNetwork,
                       'ddpg': net_mod.DDPGActorNetwork}[kind]
                nets = {}
                for tag in (('mu', 'sigma') if kind == 'sac' else ('mu',)):
                    m = cls((D,), (2,), [64, 64], action_scaling=scaling, use_cuda=False).double()
                    with torch.no_grad():
                        if kind in ('td3', 'ddpg'):                     # the reference's +-3e-3 never leaves tanh's linear range
                            m._h3.weight.uniform_(-0.4, 0.4)
                        else:
                            m._h3.weight.mul_(4.0)
                    nets[tag] = m
                    for i, lin in enumerate((m._h1, m._h2, m._h3)):
                        out['%s%s_W%d' % (p, tag, i + 1)] = lin.weight.detach().numpy().copy()
                        out['%s%s_b%d' % (p, tag, i + 1)] = lin.bias.detach().numpy().copy()
                if kind in ('td3', 'ddpg'):
                    out[p + 'action_scaling'] = scaling.copy()
                env = PointReachAtacom(n_objects=n, random_walk=True)
                env.reset()
                rec = {k: [] for k in ('state0', 's0', 'noise', 'draws', 'x0', 'action', 'state1', 's1', 'reward')}
                x = np.zeros(2)                                         # OrnsteinUhlenbeckPolicy.reset(): x0 = None -> zeros
                for t in range(STEPS):
                    obs = env._state.copy()
                    xin = (obs - 0.0) / 10.0                            # MinMaxPreprocessor of +-10 (restated)
                    eps = rng.standard_normal(2)
                    rec['state0'].append(obs)
                    rec['s0'].append(env.s.copy())
                    rec['noise'].append(eps.copy())
                    rec['x0'].append(x.copy())
                    mu = forward(nets['mu'], xin)
                    if kind == 'ppo':
                        a = mu + PPO_STD * eps
                    elif kind == 'sac':
                        a = np.tanh(mu + np.exp(np.clip(forward(nets['sigma'], xin), -20.0, 2.0)) * eps)
                    elif kind == 'td3':
                        a = np.clip(mu + np.sqrt(TD3_SIGMA) * eps, -1.0, 1.0)
                    else:
                        x = x - THETA * x * OU_DT + DDPG_SIGMA * np.sqrt(OU_DT) * eps
                        a = mu + x
                    del drawn[:]
                    o1, r, absorbing, _ = env.step(a.copy())
                    assert absorbing is False
                    rec['draws'].append(np.array(drawn).reshape(n, 2))
                    rec['action'].append(a.copy())
                    rec['state1'].append(np.array(o1, copy=True))
                    rec['s1'].append(env.s.copy())
                    rec['reward'].append(r)
                for k, v in rec.items():
                    out[p + k] = np.array(v, dtype=np.float64)
    finally:
        np.random.uniform = real_uniform
    np.savez_compressed(args.out, **out)
    print('wrote %s (%d bytes, %d arrays)' % (args.out, os.path.getsize(args.out), len(out)))


if __name__ == '__main__':
    main()
