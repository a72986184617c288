#!/usr/bin/env python3
"""Minimal on-GPU TRPO on the batched ATACOM air-hockey hitting task -- the loop of examples/ppo_air_hockey.py with the
trust-region policy step in place of the PPO epochs.

Not part of the hot path: the reference trains with MushroomRL's TRPO (examples/iiwa_air_hockey_exp.py:122-131), which is not
installed here.  Collection, the critic's values, the log-probabilities and GAE are the PPO example's launches.  The policy step
is `trpo_step`: the gradient of the surrogate in one launch, ten conjugate-gradient iterations and the step length at one
Fisher-vector product each (`fisher_vector_product`: one launch over the WHOLE collection, the obs column read in place), and
a line search whose candidates cost one evaluation launch each.  The critic is fitted as before: `value_gradient_from_records`
and the device `Adam`.  `--update torch` runs what this replaces -- the Fisher-vector product as autograd's double backward
through the KL divergence on contiguous copies of the rows, MushroomRL's way -- for comparison.

    python examples/trpo_air_hockey.py --env planar --iters 60
"""
import argparse
import math
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from anywhere in the checkout
from rl_on_manifold_amd import (Adam, BatchedAtacomEnv, MlpPolicy, RecordLayout, gae_from_records, log_prob_from_records,
                                trpo_step, value_gradient_from_records, values_from_records)

MAX_KL, ENT_COEFF, CG_ITERS, CG_DAMPING, CG_TOL, LINE_SEARCH = 1e-2, 5e-5, 10, 1e-2, 1e-10, 10      # the reference's


class Net(nn.Module):                      # same layer names as the reference's TRPONetwork
    def __init__(self, n_in, n_out, h=64):
        super().__init__()
        self._h1, self._h2, self._h3 = nn.Linear(n_in, h), nn.Linear(h, h), nn.Linear(h, n_out)
        for lin, g in ((self._h1, 'relu'), (self._h2, 'relu'), (self._h3, 'linear')):
            nn.init.xavier_uniform_(lin.weight, gain=nn.init.calculate_gain(g))

    def forward(self, x):
        return self._h3(torch.relu(self._h2(torch.relu(self._h1(x)))))


def torch_trpo_step(actor, log_std, shift, scale, obs, act, adv, logp_old):
    """MushroomRL's TRPO policy step with autograd: obs [M, D], act [M, k], adv and logp_old [M], contiguous.  Updates the
    actor's parameters and log_std in place -> dict as trpo_step."""
    params = list(actor.parameters()) + [log_std]
    k = act.shape[1]

    def dist():
        return actor((obs - shift) * scale), log_std.exp()

    def logp(mu, std):
        return (-0.5 * ((act - mu) / std) ** 2 - std.log()).sum(-1) - 0.5 * k * math.log(2 * math.pi)

    def loss(mu, std):
        return ((logp(mu, std) - logp_old).exp() * adv).mean() + ENT_COEFF * (std.log().sum() + 0.5 * k * (1 + math.log(2 * math.pi)))

    def kl(mu, std, mu_old, std_old):
        return ((std / std_old).log() + (std_old ** 2 + (mu_old - mu) ** 2) / (2 * std ** 2) - 0.5).sum(-1).mean()

    def flat(ts):
        return torch.cat([t.reshape(-1) for t in ts])

    mu, std = dist()
    mu_old, std_old = mu.detach(), std.detach()
    loss_old = loss(mu, std)
    g = flat(torch.autograd.grad(loss_old, params)).detach()

    def fvp(v):
        m, s = dist()
        grads = flat(torch.autograd.grad(kl(m, s, mu_old, std_old), params, create_graph=True))
        return flat(torch.autograd.grad((grads * v).sum(), params)).detach() + CG_DAMPING * v

    x, r, p = torch.zeros_like(g), g.clone(), g.clone()
    r2 = r.dot(r)
    for _ in range(CG_ITERS):
        z = fvp(p)
        a = r2 / p.dot(z)
        x += a * p
        r -= a * z
        r2n = r.dot(r)
        p = r + (r2n / r2) * p
        r2 = r2n
        if r2 < CG_TOL:
            break
    full = x / torch.sqrt(0.5 * x.dot(fvp(x)) / MAX_KL)
    old = flat(params).detach().clone()
    out = dict(loss_old=loss_old.item(), loss_new=loss_old.item(), kl=0.0, halvings=LINE_SEARCH, accepted=False, cg_residual=r2.item())

    def write(theta):
        o = 0
        with torch.no_grad():
            for t in params:
                t.copy_(theta[o:o + t.numel()].view_as(t))
                o += t.numel()

    for j in range(LINE_SEARCH):
        write(old + full * 0.5 ** j)
        with torch.no_grad():
            m, s = dist()
            new, d = loss(m, s).item(), kl(m, s, mu_old, std_old).item()
        if d <= 1.5 * MAX_KL and new - out['loss_old'] >= 0.0:
            out.update(loss_new=new, kl=d, halvings=j, accepted=True)
            return out
    write(old)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--env', default='planar')
    ap.add_argument('--task', default='H', choices=['H', 'D'], help="planar only: 'D' = defending (horizon 180 in the reference)")
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--horizon', type=int, default=120)
    ap.add_argument('--lr', type=float, default=3e-4, help='of the critic')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--update', default='device', choices=['device', 'torch'],
                    help="'device': trpo_step, the Fisher-vector product in one launch; 'torch': autograd's double backward")
    args = ap.parse_args(argv)
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
    gamma, lam, epochs, mb = 0.99, 0.95, 4, 16384
    lay = RecordLayout([B], D, k)
    # The networks as the kernels see them, made once: the weights are the modules' own storage, so the line search's candidates
    # and Adam's in-place steps are seen by the next launch; std is a tensor of the policy that trpo_step keeps at exp(log_std).
    std = log_std.detach().exp()
    pol, cri = MlpPolicy.from_module(actor, std=std), MlpPolicy.from_module(critic)
    for net in (pol, cri):
        net.tensors['obs_shift'], net.tensors['obs_scale'] = shift, scale
    gc = None                                                                 # the critic's gradient buffers, reused by every call
    opt = Adam([dict(net=cri)], lr=args.lr)
    rec = torch.zeros((T, B, lay.F), device=dev)
    ret, adv = torch.zeros((T, B), device=dev), torch.zeros((T, B), device=dev)
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
        v, nv = values_from_records(lay, rec, cri)
        gae_from_records(lay, rec, v, nv, gamma, lam, normalize=True, out=(ret, adv))
        logp_old = log_prob_from_records(lay, rec, pol)
        d = lay.unpack(rec)
        rew, last = d['reward'], d['last']
        # ---- the critic: epochs of minibatches, gradients gathered from the records, Adam on the device
        for _ in range(epochs):
            perm = torch.randperm(T * B, device=dev)
            for i in range(0, T * B, mb):
                gc = value_gradient_from_records(lay, rec, ret, cri, idx=perm[i:i + mb], out=gc)
                opt.step(gc)
        # ---- the policy: one trust-region step over the whole collection
        if args.update == 'device':
            res = trpo_step(lay, rec, adv, logp_old, pol, log_std, max_kl=MAX_KL, ent_coeff=ENT_COEFF, cg_iters=CG_ITERS,
                            cg_damping=CG_DAMPING, cg_residual_tol=CG_TOL, line_search=LINE_SEARCH)
        else:
            res = torch_trpo_step(actor, log_std, shift, scale, d['obs'].reshape(T * B, D).contiguous(),
                                  d['action'].reshape(T * B, k).contiguous(), adv.reshape(-1), logp_old.reshape(-1))
            std.copy_(log_std.detach().exp())
        torch.cuda.synchronize()
        t_fit += time.perf_counter() - t0
        ep_ret = rew.sum(0).mean().item() if not last[:-1].any() else (rew.sum() / last.sum().clamp_min(1)).item()
        goals = ((rew > 70) if args.task == 'H' else (rew < -40)).sum().item()      # task 'D': goals CONCEDED
        hits = (rew > 0.99).any(0).float().mean().item()
        print('iter %3d  return/episode %8.3f  goals %5d  frac envs with a hit %.3f  c_max %.4f  c_dq_max %.4f  std %.3f  '
              'kl %.5f  halvings %d  accepted %d' % (it, ep_ret, goals, hits, c_max, c_dq, log_std.exp().mean().item(),
                                                     res['kl'], res['halvings'], res['accepted']), flush=True)
    print('collection %.2f s (%.3g env-steps/s incl. policy), fitting %.2f s' % (
        t_collect, args.iters * T * B / t_collect, t_fit))


if __name__ == '__main__':
    main()
