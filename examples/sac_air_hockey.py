#!/usr/bin/env python3
"""Minimal on-GPU SAC on the batched ATACOM tasks -- an end-to-end use of libatacom_soft.so.

Not part of the hot path: the reference trains with MushroomRL's SAC (examples/*_exp.py: build_agent_SAC, its default agent),
which is not installed here.  This script shows the same loop shape on the engine: collection = ONE kernel launch per iteration
(the squashed Gaussian of `MlpPolicy.from_sac` inside `rollout_packed`), the records go into a `ReplayMemory` on the device, and
for each fit a minibatch of row numbers is drawn (`sample`); the soft target, the two critics' gradients and -- after a warm-up
count of fits -- the actor's gradients are ONE launch each that reads the memory in place (`ReplayMemory.soft_td_target`,
`soft_critic_gradient`, `soft_actor_gradient`), ONE device `Adam` of four groups (per-group lr) steps mu, sigma and both
critics, `AlphaAdam` steps log_alpha from the gradient the actor call left on the device, and `soft_update` moves the two target
critics.  `--update torch` runs the same fit through torch modules, torch.distributions and autograd -- what the calls replace --
for comparison.  The time per stage is printed (host clock around a device synchronise, the first iteration left out as warm-up).

    python examples/sac_air_hockey.py --env planar --iters 10
"""
import argparse
import copy
import math
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from anywhere in the checkout
from rl_on_manifold_amd import (Adam, AlphaAdam, BatchedAtacomEnv, BatchedPointReachEnv, MlpPolicy, RecordLayout, ReplayMemory,
                                SoftCritic, soft_update)


class Net(nn.Module):                      # the layer names of the reference's SACActorNetwork and SACCriticNetwork
    def __init__(self, n_in, n_out, h=64):
        super().__init__()
        self._h1, self._h2, self._h3 = nn.Linear(n_in, h), nn.Linear(h, h), nn.Linear(h, n_out)

    def forward(self, x):
        return self._h3(torch.relu(self._h2(torch.relu(self._h1(x)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--env', default='planar', choices=['planar', 'iiwa', 'point'])
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--steps', type=int, default=16, help='environment steps per iteration and environment')
    ap.add_argument('--fits', type=int, default=16, help='minibatches per iteration')
    ap.add_argument('--minibatch', type=int, default=16384)
    ap.add_argument('--capacity', type=int, default=1 << 20)
    ap.add_argument('--warmup-fits', type=int, default=4, help='fits before the actor is updated (MushroomRL: warmup_transitions)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--update', default='fused', choices=['fused', 'torch'], help="'torch': the fit through torch autograd")
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    dev = torch.device('cuda:0')
    B, T, M = args.batch, args.steps, args.minibatch
    if args.env == 'point':
        env = BatchedPointReachEnv(B, device=dev, horizon=200, seed=args.seed)
    else:
        env = BatchedAtacomEnv(args.env, B, device=dev, auto_reset=True, horizon=120, random_init=True, seed=args.seed)
    D, k = env.obs_dim, env.dims['null']
    gamma, tau, lr_actor, lr_critic, lr_alpha, target_entropy = 0.99, 5e-3, 3e-4, 3e-4, 3e-4, -float(k)
    lmin, lmax = -20.0, 2.0
    mu, sg = Net(D, k).to(dev), Net(D, k).to(dev)
    critics = [Net(D + k, 1).to(dev) for _ in range(2)]
    critics_t = [copy.deepcopy(c) for c in critics]
    log_alpha = torch.zeros(1, device=dev, requires_grad=(args.update == 'torch'))

    # the weights are the modules' own storage: the optimisers' in-place steps are seen by the kernels
    pol = MlpPolicy.from_sac(mu, sg, log_std_min=lmin, log_std_max=lmax)
    pol_sigma = MlpPolicy.from_module(sg)
    cri, cri_t = [SoftCritic.from_module(c, D) for c in critics], [SoftCritic.from_module(c, D) for c in critics_t]
    nets, nets_t = [c.as_policy() for c in cri], [c.as_policy() for c in cri_t]
    if args.update == 'fused':
        opt = Adam([dict(net=pol, lr=lr_actor), dict(net=pol_sigma, lr=lr_actor), dict(net=nets[0], lr=lr_critic), dict(net=nets[1], lr=lr_critic)])
        opt_alpha = AlphaAdam(log_alpha, lr=lr_alpha)
    else:
        opt_a = torch.optim.Adam(list(mu.parameters()) + list(sg.parameters()), lr=lr_actor)
        opt_c = torch.optim.Adam([p for c in critics for p in c.parameters()], lr=lr_critic)
        opt_l = torch.optim.Adam([log_alpha], lr=lr_alpha)
    lay = RecordLayout([B], D, k)
    mem = ReplayMemory(args.capacity, D, k, device=dev)
    rec = torch.zeros((T, B, lay.F), device=dev)
    y = torch.empty(M, device=dev)
    held = dict(c=None, a=None)
    times = dict(collect=0.0, add=0.0, sample=0.0, target=0.0, critics=0.0, actor=0.0, optimise=0.0, soft_update=0.0)
    warm = [args.iters > 1]                # the first iteration loads code objects and lets the libraries pick algorithms: not timed

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if not warm[0]:
            times[name] += time.perf_counter() - t0
        return out

    def sample_t(x, eps):                  # SACPolicy.compute_action_and_log_prob_t with the caller's eps
        m, l = mu(x), torch.clamp(sg(x), lmin, lmax)
        dist = torch.distributions.Normal(m, l.exp())
        u = m + l.exp() * eps
        a = torch.tanh(u)
        return a, dist.log_prob(u).sum(1) - torch.log(1.0 - a.pow(2) + 1e-6).sum(1)

    def q_t(net, s, a):
        return net(torch.cat((s, a), 1))[:, 0]

    def torch_target(idx, eps):
        with torch.no_grad():
            c = mem.columns(idx)
            a, lp = sample_t(c['next_obs'], eps)
            q = torch.minimum(q_t(critics_t[0], c['next_obs'], a), q_t(critics_t[1], c['next_obs'], a))
            return c['reward'] + gamma * (1.0 - c['absorbing']) * (q - log_alpha.exp() * lp)

    def torch_critics(idx, tgt):
        c = mem.columns(idx)
        loss = sum(((q_t(cr, c['obs'], c['action']) - tgt) ** 2).mean() for cr in critics)
        opt_c.zero_grad(set_to_none=True)
        loss.backward()
        return loss

    def torch_actor(idx, eps):
        c = mem.columns(idx)
        a, lp = sample_t(c['obs'], eps)
        loss = (log_alpha.exp().detach() * lp - torch.minimum(q_t(critics[0], c['obs'], a), q_t(critics[1], c['obs'], a))).mean()
        opt_a.zero_grad(set_to_none=True)
        loss.backward(inputs=opt_a.param_groups[0]['params'])
        opt_l.zero_grad(set_to_none=True)
        (-(log_alpha * (lp.detach() + target_entropy)).mean()).backward()
        return loss

    n_fit = timed_iters = timed_fits = 0
    env.reset()
    for it in range(args.iters):
        noise = torch.randn((T, B, k), device=dev)
        timed('collect', lambda: env.rollout_packed(policy=pol, n_steps=T, noise=noise, out=rec))
        timed('add', lambda: mem.add(lay, rec))
        q_loss = a_loss = float('nan')
        for _ in range(args.fits):
            idx = timed('sample', lambda: mem.sample(M))
            eps_t, eps_a = torch.randn((M, k), device=dev), torch.randn((M, k), device=dev)
            act = n_fit >= args.warmup_fits
            la = None
            if args.update == 'fused':
                timed('target', lambda: mem.soft_td_target(pol, cri_t, idx, gamma, log_alpha, eps_t, out=y))
                held['c'] = timed('critics', lambda: mem.soft_critic_gradient(cri, idx, y, out=held['c']))
                lq = held['c'][0].loss + held['c'][1].loss
                if act:
                    held['a'] = timed('actor', lambda: mem.soft_actor_gradient(pol, cri, idx, eps_a, log_alpha, target_entropy, out=held['a']))
                    la = held['a'].loss

                    def optimise():
                        opt.step(held['a'].mu, held['a'].sigma, held['c'][0], held['c'][1])
                        opt_alpha.step(held['a'].alpha_grad)
                    timed('optimise', optimise)
                else:                      # the critics alone: the actor's groups step on zero gradients of a first call
                    if held['a'] is None:
                        held['a'] = mem.soft_actor_gradient(pol, cri, idx, eps_a, log_alpha, target_entropy)
                    held['a'].mu.flat.zero_()
                    held['a'].sigma.flat.zero_()
                    timed('optimise', lambda: opt.step(held['a'].mu, held['a'].sigma, held['c'][0], held['c'][1]))
            else:
                tgt = timed('target', lambda: torch_target(idx, eps_t))
                lq = timed('critics', lambda: torch_critics(idx, tgt))
                if act:
                    la = timed('actor', lambda: torch_actor(idx, eps_a))

                def optimise():
                    opt_c.step()
                    if act:
                        opt_a.step()
                        opt_l.step()
                timed('optimise', optimise)
            timed('soft_update', lambda: soft_update(nets_t, nets, tau))
            n_fit += 1
            q_loss, a_loss = lq.item(), (a_loss if la is None else la.item())
            if not (math.isfinite(q_loss) and (la is None or math.isfinite(a_loss))):
                raise SystemExit('a loss is not finite: critics %r, actor %r' % (q_loss, a_loss))
        timed_iters = timed_iters + (0 if warm[0] else 1)
        timed_fits = timed_fits + (0 if warm[0] else args.fits)
        warm[0] = False
        r = rec[..., lay.fields['reward']]
        print('iter %3d  memory %8d  reward/step %8.4f  critic loss %10.4f  actor loss %10.4f  alpha %.4f' % (
            it, mem.size, r.mean().item(), q_loss, a_loss, log_alpha.exp().item()), flush=True)
    n, ni = max(timed_fits, 1), max(timed_iters, 1)
    print('per iteration (%d timed): collect %.3f ms, add %.3f ms;  per fit (%d rows, update: %s): sample %.3f ms, target %.3f ms, '
          'critic gradients %.3f ms, actor gradients %.3f ms, optimisers %.3f ms, soft update %.3f ms' % (
              ni, 1e3 * times['collect'] / ni, 1e3 * times['add'] / ni, M, args.update, 1e3 * times['sample'] / n, 1e3 * times['target'] / n,
              1e3 * times['critics'] / n, 1e3 * times['actor'] / n, 1e3 * times['optimise'] / n, 1e3 * times['soft_update'] / n))


if __name__ == '__main__':
    main()
