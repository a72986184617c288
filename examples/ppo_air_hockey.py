#!/usr/bin/env python3
"""Minimal on-GPU PPO on the batched ATACOM air-hockey hitting task -- an end-to-end use of the engine.

Not part of the hot path: the reference trains with MushroomRL's PPO (examples/planar_air_hockey_exp.py,
examples/iiwa_air_hockey_exp.py:137-170), which is not installed here.  This script shows the same loop shape on the
engine: collection = ONE kernel launch per iteration (policy MLP + exploration noise + ATACOM env step fused, written as packed
records: `rollout_packed`), the critic on obs and next_obs and the log-probability of the drawn actions = three more, read from
the records in place (`values_from_records`, `log_prob_from_records`), advantages = one more (`gae_from_records`), and the
gradients of a minibatch = one launch per network, gathered from the records through the minibatch's row numbers
(`policy_gradient_from_records`, `value_gradient_from_records`), and the optimiser step = one more for both networks and log
std (`Adam`), its state on the device -- so an epoch of minibatches is ONE graph replay (`GraphedUpdate`) with a permutation
drawn on the device.  `--update torch` runs the loop this replaces -- the same gradient calls, torch's Adam taking them as
.grad, one Python iteration per minibatch -- for comparison.
Network = the reference's PPONetwork (examples/network.py:8-36: Linear-ReLU-Linear-ReLU-Linear, 64 units), Gaussian policy with
state-independent std.

    python examples/ppo_air_hockey.py --env planar --iters 60
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from anywhere in the checkout
from rl_on_manifold_amd import (Adam, BatchedAtacomEnv, GraphedUpdate, MlpPolicy, RecordLayout, gae_from_records,
                                log_prob_from_records, policy_gradient_from_records, value_gradient_from_records,
                                values_from_records)


class Net(nn.Module):                      # same layer names as the reference's PPONetwork
    def __init__(self, n_in, n_out, h=64):
        super().__init__()
        self._h1, self._h2, self._h3 = nn.Linear(n_in, h), nn.Linear(h, h), nn.Linear(h, n_out)
        for lin, g in ((self._h1, 'relu'), (self._h2, 'relu'), (self._h3, 'linear')):
            nn.init.xavier_uniform_(lin.weight, gain=nn.init.calculate_gain(g))

    def forward(self, x):
        return self._h3(torch.relu(self._h2(torch.relu(self._h1(x)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--env', default='planar')
    ap.add_argument('--task', default='H', choices=['H', 'D'], help="planar only: 'D' = defending (horizon 180 in the reference)")
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--horizon', type=int, default=120)
    ap.add_argument('--lr', type=float, default=3e-4)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--update', default='graph', choices=['graph', 'torch'],
                    help="'graph': the device Adam, an epoch replayed as one graph; 'torch': torch.optim.Adam in a Python loop")
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    dev = torch.device('cuda:0')
    B, T = args.batch, args.horizon
    env = BatchedAtacomEnv(args.env, B, device=dev, auto_reset=True, horizon=T, random_init=True, seed=args.seed, task=args.task)
    D, k = env.obs_dim, env.dims['null']
    # observation normalisation (what MinMaxPreprocessor does with finite bounds): fixed shift / scale
    shift = torch.zeros(D, device=dev)
    scale = torch.ones(D, device=dev)
    shift[0] = 1.1
    scale[3:6] = 0.2
    actor, critic = Net(D, k).to(dev), Net(D, 1).to(dev)
    log_std = torch.full((k,), -0.7, device=dev, requires_grad=True)          # std_0 = 0.5
    gamma, lam, clip, epochs, mb = 0.99, 0.95, 0.2, 4, 16384
    lay = RecordLayout([B], D, k)
    # The networks as the kernels see them, made once: the weights are the modules' own storage, so Adam's in-place steps are
    # seen by the next launch; std is a tensor of the policy that follows log_std (refreshed in place after every step).
    std = log_std.detach().exp()
    pol, cri = MlpPolicy.from_module(actor, std=std), MlpPolicy.from_module(critic)
    for net in (pol, cri):
        net.tensors['obs_shift'], net.tensors['obs_scale'] = shift, scale
    gp = gc = None                                                            # the gradients' buffers, reused by every call
    if args.update == 'torch':
        opt = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()) + [log_std], lr=args.lr)
    else:                                                                     # the loss is  policy + 0.5 value
        opt = Adam([dict(net=pol, log_std=log_std, std=std), dict(net=cri, scale=0.5)], lr=args.lr)
    # what the graph reads is static: the records, returns, advantages and old log-probabilities are refilled in place
    rec = torch.zeros((T, B, lay.F), device=dev)
    ret, adv, logp_old = (torch.zeros((T, B), device=dev) for _ in range(3))
    # one epoch = one replay: a permutation drawn into the graph's static buffer, then for every minibatch the two gradient
    # launches and the Adam launch (clip and lr are baked into the graph; the capture's warm-up is undone by the constructor)
    update = GraphedUpdate(lay, rec, adv, ret, logp_old, pol, cri, opt, mb, clip=clip) if args.update == 'graph' else None
    t_collect = t_fit = 0.0
    for it in range(args.iters):
        t0 = time.perf_counter()
        noise = torch.randn((T, B, k), device=dev)
        env.reset()
        env.rollout_packed(policy=pol, n_steps=T, noise=noise, out=rec)       # ONE launch: T steps of B envs, [T, B, 2 D + k + 3]
        c_avg, c_max, c_dq = env.get_constraints_logs()
        torch.cuda.synchronize()
        t_collect += time.perf_counter() - t0
        t0 = time.perf_counter()
        # what the update needs from the old networks, each one launch over the records where they lie (evaluate.py): V(obs) and
        # V(next_obs), the log-probability of the drawn actions -- and then advantages, returns and PPO's normalisation, the
        # recurrence over time in one launch (returns.py), where a loop `for t in reversed(range(T))` costs five per step
        v, nv = values_from_records(lay, rec, cri)
        gae_from_records(lay, rec, v, nv, gamma, lam, normalize=True, out=(ret, adv))
        logp_old.copy_(log_prob_from_records(lay, rec, pol))
        d = lay.unpack(rec)
        rew, last = d['reward'], d['last']
        for _ in range(epochs):
            if update is not None:
                update.replay()
                continue
            perm = torch.randperm(T * B, device=dev)
            for i in range(0, T * B, mb):
                idx = perm[i:i + mb]                                          # row numbers into the flat [T * B] records
                # the gradients of  -min(ratio adv, clamp(ratio) adv).mean()  and  (critic(obs) - ret).pow(2).mean()  over the rows
                # idx names: forward and backward pass of each network in one launch, obs and action read from the records
                gp = policy_gradient_from_records(lay, rec, adv, logp_old, pol, clip=clip, idx=idx, out=gp)
                gc = value_gradient_from_records(lay, rec, ret, cri, idx=idx, out=gc)
                gc.flat.mul_(0.5)                                             # the loss is  policy + 0.5 value
                gp.to_module(actor, log_std)
                gc.to_module(critic)
                opt.step()
                std.copy_(log_std.detach().exp())
        torch.cuda.synchronize()
        t_fit += time.perf_counter() - t0
        ep_ret = rew.sum(0).mean().item() if not last[:-1].any() else (rew.sum() / last.sum().clamp_min(1)).item()
        goals = ((rew > 70) if args.task == 'H' else (rew < -40)).sum().item()      # task 'D': goals CONCEDED
        hits = (rew > 0.99).any(0).float().mean().item()
        print('iter %3d  return/episode %8.3f  goals %5d  frac envs with a hit %.3f  c_max %.4f  c_dq_max %.4f  std %.3f'
              % (it, ep_ret, goals, hits, c_max, c_dq, log_std.exp().mean().item()), flush=True)
    print('collection %.2f s (%.3g env-steps/s incl. policy), fitting %.2f s' % (
        t_collect, args.iters * T * B / t_collect, t_fit))


if __name__ == '__main__':
    main()
