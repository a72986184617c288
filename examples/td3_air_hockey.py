#!/usr/bin/env python3
"""Minimal on-GPU TD3 on the batched ATACOM tasks -- an end-to-end use of the off-policy half of the engine.

Not part of the hot path: the reference trains with MushroomRL's TD3 (examples/iiwa_air_hockey_exp.py: build_agent_td3), which
is not installed here.  This script shows the same loop shape on the engine: collection = ONE kernel launch per iteration (the
actor's squashed mean + clipped Gaussian exploration + ATACOM env step, `MlpPolicy.from_td3` inside `rollout_packed`), the
records go into a `ReplayMemory` on the device, and for each fit a minibatch of row numbers is drawn (`sample`), the TD target
r + gamma (1 - absorbing) min_j Q'_j(s', clip(pi'(s') + clip(sigma eps))) is ONE launch that reads the memory in place
(`ReplayMemory.td_target`), the gradients of the two critic losses are ONE launch and that of the actor loss another
(`ReplayMemory.critic_gradient`, `actor_gradient`: the memory read in place again), torch's Adam steps the critics from
`QGradients.to_module` and the device `Adam` steps the actor, and the three target networks move in ONE launch (`soft_update`).
`--step device` replaces both optimisers and `soft_update` with `TrackedAdam` -- the critics' and the actor's Adam steps on the
device, each target following its network in the step's own launch -- and `--step graph` replays `policy_delay` whole fits as one
graph (`GraphedFit`; row numbers and noise are drawn into its static buffers).  `--step torch`, the default, is the path above.
`--losses torch` takes the losses through torch autograd on `columns(idx)` instead -- the gather, three forward and three
backward passes that the two gradient calls replace -- for comparison.  `--target torch` computes the same targets with torch modules -- the gather, three module
passes and a dozen elementwise kernels that `td_target` replaces -- for comparison.  The time per stage is printed (host clock
around a device synchronise, the first iteration left out as warm-up); the whole fit is timed around all its stages, and
`--no-stage-sync` leaves the synchronisations between the stages out, so that the whole-fit time is that of an undisturbed loop.

    python examples/td3_air_hockey.py --env planar --iters 10
"""
import argparse
import copy
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from anywhere in the checkout
from rl_on_manifold_amd import (Adam, BatchedAtacomEnv, BatchedPointReachEnv, GraphedFit, MlpPolicy, QCritic, RecordLayout,
                                ReplayMemory, TrackedAdam, soft_update)


class Actor(nn.Module):                    # the layer names of the reference's TD3ActorNetwork
    def __init__(self, n_in, n_out, scaling, h=64):
        super().__init__()
        self._h1, self._h2, self._h3 = nn.Linear(n_in, h), nn.Linear(h, h), nn.Linear(h, n_out)
        self.register_buffer('_action_scaling', scaling.clone())

    def forward(self, x):
        return self._action_scaling * torch.tanh(self._h3(torch.relu(self._h2(torch.relu(self._h1(x))))))


class Critic(nn.Module):                   # the layer names of the reference's TD3CriticNetwork: the action enters twice
    def __init__(self, n_obs, n_act, scaling, h=64):
        super().__init__()
        self._h1, self._h2_s, self._h2_a, self._h3 = (nn.Linear(n_obs + n_act, h), nn.Linear(h, h), nn.Linear(n_act, h, bias=False),
                                                      nn.Linear(h, 1))
        self.register_buffer('_action_scaling', scaling.clone())

    def forward(self, s, a):
        a = a / self._action_scaling
        h1 = torch.relu(self._h1(torch.cat((s, a), -1)))
        return self._h3(torch.relu(self._h2_s(h1) + self._h2_a(a))).squeeze(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--env', default='planar', choices=['planar', 'iiwa', 'point'])
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--steps', type=int, default=16, help='environment steps per iteration and environment')
    ap.add_argument('--fits', type=int, default=16, help='minibatches per iteration')
    ap.add_argument('--minibatch', type=int, default=16384)
    ap.add_argument('--capacity', type=int, default=1 << 20)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--target', default='fused', choices=['fused', 'torch'], help="'torch': the targets through torch modules")
    ap.add_argument('--losses', default='fused', choices=['fused', 'torch'], help="'torch': the losses through torch autograd")
    ap.add_argument('--step', default='torch', choices=['torch', 'device', 'graph'],
                    help="'torch': torch's Adam over the critics, the device Adam over the actor, soft_update; 'device': TrackedAdam, "
                         "no soft_update call; 'graph': GraphedFit, policy_delay fits per replay")
    ap.add_argument('--no-stage-sync', action='store_true', help='time the whole fit only, without synchronising between its stages')
    args = ap.parse_args()
    if args.step != 'torch' and (args.target, args.losses) != ('fused', 'fused'):
        ap.error('--step %s takes the fused target and losses' % args.step)
    torch.manual_seed(args.seed)
    dev = torch.device('cuda:0')
    B, T = args.batch, args.steps
    if args.env == 'point':
        env = BatchedPointReachEnv(B, device=dev, horizon=200, seed=args.seed)
    else:
        env = BatchedAtacomEnv(args.env, B, device=dev, auto_reset=True, horizon=120, random_init=True, seed=args.seed)
    D, k = env.obs_dim, env.dims['null']
    gamma, tau, sigma, noise_std, noise_clip, delay = 0.99, 5e-3, 0.1, 0.2, 0.5, 2
    scaling = torch.ones(k, device=dev)
    low, high = -scaling, scaling.clone()
    actor = Actor(D, k, scaling).to(dev)
    critics = [Critic(D, k, scaling).to(dev) for _ in range(2)]
    actor_t, critics_t = copy.deepcopy(actor), [copy.deepcopy(c) for c in critics]

    def as_policy(net):                    # the weights are the module's own storage: Adam's in-place steps are seen by the kernels
        pol = MlpPolicy.from_td3(net, sigma ** 2, low=-1.0, high=1.0)
        pol.tensors.update(act_scale=scaling, act_low=low, act_high=high, std=torch.full((k,), sigma, device=dev))
        return pol

    def as_critic(net):
        c = QCritic.from_module(net, D)
        c.tensors['act_scale'] = scaling
        return c

    pol, pol_t = as_policy(actor), as_policy(actor_t)
    cri, cri_t = [as_critic(c) for c in critics], [as_critic(c) for c in critics_t]
    opt_a = torch.optim.Adam(actor.parameters(), lr=1e-4)
    opt_c = torch.optim.Adam([p for c in critics for p in c.parameters()], lr=3e-4)
    opt_a_dev = Adam([{'net': pol}], lr=1e-4) if args.losses == 'fused' else None      # steps the actor's own storage, in one launch
    opt_dev = TrackedAdam([dict(net=pol, target=pol_t, lr=1e-4)] + [dict(net=c, target=ct, lr=3e-4) for c, ct in zip(cri, cri_t)],
                          tau=tau) if args.step != 'torch' else None      # the three networks and their targets: one launch
    graphed = None                         # made after the first collection: the memory must hold a row
    grads = dict(q=None, a=None)
    lay = RecordLayout([B], D, k)
    mem = ReplayMemory(args.capacity, D, k, device=dev)
    rec = torch.zeros((T, B, lay.F), device=dev)
    y = torch.empty(args.minibatch, device=dev)
    times = dict(collect=0.0, add=0.0, sample=0.0, target=0.0, losses=0.0, soft_update=0.0, fit=0.0)
    if args.step == 'graph' and args.fits % delay:
        ap.error('--step graph replays %d fits at a time: --fits must be a multiple of it' % delay)

    warm = [args.iters > 1]                # the first iteration loads code objects and lets the libraries pick algorithms: not timed

    def timed(name, fn):
        if args.no_stage_sync and name not in ('collect', 'add', 'fit'):
            return fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if not warm[0]:
            times[name] += time.perf_counter() - t0
        return out

    def torch_target(idx, eps):
        with torch.no_grad():
            c = mem.columns(idx)
            a = actor_t(c['next_obs'])
            a = torch.minimum(torch.maximum(a + torch.clamp(noise_std * eps, -noise_clip, noise_clip), low), high)
            q = torch.minimum(critics_t[0](c['next_obs'], a), critics_t[1](c['next_obs'], a))
            return c['reward'] + gamma * (q * (1.0 - c['absorbing']))

    def one_fit(n_fit):
        idx = timed('sample', lambda: mem.sample(args.minibatch))
        eps = torch.randn((args.minibatch, k), device=dev)
        if args.target == 'fused':
            timed('target', lambda: mem.td_target(pol_t, cri_t, idx, gamma, eps=eps, noise_std=noise_std, noise_clip=noise_clip,
                                                  low=low, high=high, out=y))
            tgt = y
        else:
            tgt = timed('target', lambda: torch_target(idx, eps))

        def losses():
            c = mem.columns(idx)
            lq = sum(((cr(c['obs'], c['action']) - tgt) ** 2).mean() for cr in critics)
            opt_c.zero_grad(set_to_none=True)
            lq.backward()
            opt_c.step()
            la = None
            if n_fit % delay == 0:
                la = -critics[0](c['obs'], actor(c['obs'])).mean()
                opt_a.zero_grad(set_to_none=True)
                la.backward()
                opt_a.step()
            return lq, la

        def fused_losses():
            first = grads['q'] is None
            grads['q'] = mem.critic_gradient(cri, idx, tgt, out=grads['q'])
            if first:                      # the parameters share the buffers from here on: every later call rewrites their .grad
                for g, net in zip(grads['q'], critics):
                    g.to_module(net)
            opt_c.step()
            la = None
            if n_fit % delay == 0:
                grads['a'] = mem.actor_gradient(pol, cri[0], idx, out=grads['a'])
                opt_a_dev.step(grads['a'])
                la = grads['a'].loss
            return grads['q'][0].loss + grads['q'][1].loss, la

        def device_losses():               # MushroomRL's order: critic fit, the actor through the updated critic, the targets
            grads['q'] = mem.critic_gradient(cri, idx, tgt, out=grads['q'])
            la = None
            if n_fit % delay == 0:
                opt_dev.step(None, *grads['q'], only=(1, 2))
                grads['a'] = mem.actor_gradient(pol, cri[0], idx, out=grads['a'])
                opt_dev.step(grads['a'], None, None, only=(0,))
                la = grads['a'].loss
            else:
                opt_dev.step(None, *grads['q'])
            return grads['q'][0].loss + grads['q'][1].loss, la
        out = timed('losses', device_losses if args.step == 'device' else fused_losses if args.losses == 'fused' else losses)
        if args.step == 'torch':           # ('device': every target has followed its network in the step's launch)
            timed('soft_update', lambda: soft_update([pol_t] + cri_t, [pol] + cri, tau))
        return out

    n_fit = timed_iters = timed_fits = 0
    env.reset()
    for it in range(args.iters):
        noise = torch.randn((T, B, k), device=dev)
        timed('collect', lambda: env.rollout_packed(policy=pol, n_steps=T, noise=noise, out=rec))
        timed('add', lambda: mem.add(lay, rec))
        q_loss = a_loss = float('nan')
        if args.step == 'graph' and graphed is None:
            graphed = GraphedFit(mem, pol, pol_t, cri, cri_t, opt_dev, args.minibatch, gamma, policy_delay=delay, noise_std=noise_std,
                                 noise_clip=noise_clip, low=low, high=high)
        for _ in range(args.fits // delay if args.step == 'graph' else args.fits):
            if args.step == 'graph':       # `delay` fits: row numbers, noise, targets, gradients, steps and target updates
                timed('fit', graphed.replay)
                n_fit += delay
                q_loss, a_loss = sum(x.item() for x in graphed.critic_losses), graphed.actor_loss.item()
                continue
            lq, la = timed('fit', lambda: one_fit(n_fit))
            n_fit += 1
            q_loss, a_loss = lq.item(), (a_loss if la is None else la.item())
        timed_iters = timed_iters + (0 if warm[0] else 1)
        timed_fits = timed_fits + (0 if warm[0] else args.fits)
        warm[0] = False
        r = rec[..., lay.fields['reward']]
        print('iter %3d  memory %8d  reward/step %8.4f  critic loss %10.4f  actor loss %10.4f' % (it, mem.size, r.mean().item(), q_loss, a_loss),
              flush=True)
    n, ni = max(timed_fits, 1), max(timed_iters, 1)
    print('per iteration (%d timed): collect %.3f ms, add %.3f ms;  per fit (%d rows, targets: %s, losses: %s): sample %.3f ms, target %.3f ms, '
          'losses + Adam %.3f ms, soft update %.3f ms;  whole fit (step: %s%s) %.3f ms' % (
              ni, 1e3 * times['collect'] / ni, 1e3 * times['add'] / ni, args.minibatch, args.target, args.losses, 1e3 * times['sample'] / n,
              1e3 * times['target'] / n, 1e3 * times['losses'] / n, 1e3 * times['soft_update'] / n, args.step,
              ', no stage synchronisation' if args.no_stage_sync or args.step == 'graph' else '', 1e3 * times['fit'] / n))


if __name__ == '__main__':
    main()
