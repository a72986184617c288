#!/usr/bin/env python3
"""Times the gradients of one PPO minibatch as libatacom_fit.so computes them (rl_on_manifold_amd/fit.py) against the torch
code they replace: the inner loop body of examples/ppo_air_hockey.py before this library -- the gathers fo[idx], fa[idx], ...,
the two forward passes, the two loss expressions and backward() -- with the optimiser step left out on both sides.  float32,
iiwa-sized networks (D = 18, k = 5), T = 120, B = 8192: M = 16384 rows gathered through idx from 983040, and all 983040 rows.
Needs a GPU; results: profiles/fit.md.

    python profiles/tools/time_fit.py [--reps 20] [--only new|torch] [--out FILE]

Reported per configuration and head: the time of a call from device events over `reps` back-to-back repetitions (what the GPU
spends: kernels and the gaps between them) and the host's wall time of one call that ends in a synchronise.  Kernel times proper
come from a run of this script under `rocprofv3 --kernel-trace --stats` with --only new.  The two variants alternate inside one
process, and their gradients are compared before anything is timed.
"""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from rl_on_manifold_amd import (MlpPolicy, RecordLayout, policy_gradient_from_records, value_gradient_from_records)      # noqa: E402


class Net(nn.Module):      # the example's network (the reference's PPONetwork)
    def __init__(self, n_in, n_out, h=64):
        super().__init__()
        self._h1, self._h2, self._h3 = nn.Linear(n_in, h), nn.Linear(h, h), nn.Linear(h, n_out)

    def forward(self, x):
        return self._h3(torch.relu(self._h2(torch.relu(self._h1(x)))))


def timed(fn, reps):
    """(ms per repetition by device events over `reps` back-to-back calls, ms of one call by the host clock with a synchronise)."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--only', choices=['new', 'torch'], default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_fit.py measures on a GPU; there is none')
    dev, T, B, D, k, clip = torch.device('cuda:0'), 120, 8192, 18, 5, 0.2
    torch.manual_seed(0)
    actor, critic = Net(D, k).to(dev), Net(D, 1).to(dev)
    shift, scale = torch.randn(D, device=dev) * 0.1, torch.rand(D, device=dev) + 0.5
    log_std = torch.full((k,), -0.7, device=dev, requires_grad=True)
    pol, cri = MlpPolicy.from_module(actor, std=log_std.detach().exp()), MlpPolicy.from_module(critic)
    for p in (pol, cri):
        p.tensors['obs_shift'], p.tensors['obs_scale'] = shift, scale
    lay = RecordLayout([B], D, k)
    rec = torch.randn((T, B, lay.F), device=dev)
    adv, ret = torch.randn((T, B), device=dev), torch.randn((T, B), device=dev)
    d = lay.unpack(rec)
    log_norm = 0.5 * k * math.log(2.0 * math.pi)
    with torch.no_grad():
        mu = actor((d['obs'] - shift) * scale)
        logp_old = (-0.5 * ((d['action'] - mu) / log_std.exp()) ** 2 - log_std).sum(-1) - log_norm + 0.2 * torch.randn((T, B), device=dev)
    # what the example held before its inner loop
    flat = lambda x: x.reshape(T * B, *x.shape[2:])                       # noqa: E731
    fo, fa, fadv, fret, flp = flat((d['obs'] - shift) * scale), flat(d['action']), flat(adv), flat(ret), flat(logp_old)
    params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    rows_out = []
    for label, idx in (('M = 16384 of 983040 through idx', torch.randperm(T * B, device=dev)[:16384]), ('M = 983040, all rows', None)):
        sel = (lambda x: x) if idx is None else (lambda x: x[idx])

        def torch_policy():
            mu = actor(sel(fo))
            logp = (-0.5 * ((sel(fa) - mu) / log_std.exp()) ** 2 - log_std).sum(-1) - log_norm
            ratio = (logp - sel(flp)).exp()
            pl = -torch.min(ratio * sel(fadv), ratio.clamp(1 - clip, 1 + clip) * sel(fadv)).mean()
            for p in params:
                p.grad = None
            pl.backward()
            return pl

        def torch_value():
            vl = (critic(sel(fo)).squeeze(-1) - sel(fret)).pow(2).mean()
            for p in params:
                p.grad = None
            vl.backward()
            return vl

        out = {}

        def new_policy():
            out['p'] = policy_gradient_from_records(lay, rec, adv, logp_old, pol, clip=clip, idx=idx, out=out.get('p'))
            return out['p']

        def new_value():
            out['v'] = value_gradient_from_records(lay, rec, ret, cri, idx=idx, out=out.get('v'))
            return out['v']

        for head, old, new, net in (('policy', torch_policy, new_policy, actor), ('value', torch_value, new_value, critic)):
            loss = old()
            ref = torch.cat([p.grad.reshape(-1) for p in net.parameters()] + ([log_std.grad] if head == 'policy' else []))
            g = new()
            torch.cuda.synchronize()
            row = dict(rows=label, head=head, loss_torch=float(loss.detach()), loss_new=float(g.stats[0]),
                       rel_diff=float((g.flat - ref).norm() / ref.norm()))
            for _ in range(2):                                                    # alternate: torch, new, torch, new
                for tag, fn in (('torch', old), ('new', new)):
                    if args.only in (None, tag):
                        ev, wall = timed(fn, args.reps)
                        row.setdefault(tag + '_event_ms', []).append(round(ev, 4))
                        row.setdefault(tag + '_wall_ms', []).append(round(wall, 4))
            print(json.dumps(row), flush=True)
            rows_out.append(row)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(rows_out, fh, indent=1)


if __name__ == '__main__':
    main()
