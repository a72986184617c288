#!/usr/bin/env python3
"""Times the Fisher-vector product of libatacom_trust.so (rl_on_manifold_amd/trust.py) and the TRPO policy step built on it
against what they replace: MushroomRL's product, autograd's double backward through the KL divergence on contiguous copies of
the rows (examples/trpo_air_hockey.py --update torch), and against the project's own policy_gradient on the same rows.  float32,
the iiwa-sized policy of profiles/fit.md (D = 18, k = 5, ReLU, shift / scale), full records, T = 120, B = 8192: M = 16384 rows
gathered through idx from 983040, and all 983040 rows.  Needs a GPU; results: profiles/trust.md.

    python profiles/tools/time_trust.py [--reps 20] [--out FILE]

Every figure is the median (with min and max) of `reps` repetitions, each between its own pair of HIP events, after a warm-up
call; the variants alternate inside one process, and the products are compared before anything is timed.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import trpo_air_hockey as ex                                                       # noqa: E402
from rl_on_manifold_amd import (MlpPolicy, RecordLayout, fisher_vector_product_from_records, policy_gradient_from_records,      # noqa: E402
                                trpo_step, FisherProduct)


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_trust.py measures on a GPU; there is none')
    dev, T, B, D, k = torch.device('cuda:0'), 120, 8192, 18, 5
    torch.manual_seed(0)
    actor = ex.Net(D, k).to(dev)
    shift, scale = torch.randn(D, device=dev) * 0.1, torch.rand(D, device=dev) + 0.5
    log_std = torch.full((k,), -0.7, device=dev, requires_grad=True)
    std = log_std.detach().exp()
    pol = MlpPolicy.from_module(actor, std=std)
    pol.tensors['obs_shift'], pol.tensors['obs_scale'] = shift, scale
    lay = RecordLayout([B], D, k)
    rec = torch.randn((T, B, lay.F), device=dev)
    d = lay.unpack(rec)
    with torch.no_grad():
        mu = actor((d['obs'] - shift) * scale)
        d['action'].copy_(mu + std * torch.randn((T, B, k), device=dev))
    adv = torch.randn((T, B), device=dev)
    params = list(actor.parameters()) + [log_std]
    flat = lambda ts: torch.cat([t.reshape(-1) for t in ts])                  # noqa: E731
    v = torch.randn(sum(p.numel() for p in params), device=dev) * 0.05
    rows_out = []
    for label, idx in (('M = 16384 of 983040 through idx', torch.randperm(T * B, device=dev)[:16384]), ('M = 983040, all rows', None)):
        obs = d['obs'].reshape(T * B, D)
        obs = (obs if idx is None else obs[idx]).contiguous()                 # the baseline's contiguous copy, made once
        with torch.no_grad():
            mu_old, std_old = actor((obs - shift) * scale), log_std.exp()

        def torch_fvp():
            m, s = actor((obs - shift) * scale), log_std.exp()
            kl = ((s / std_old).log() + (std_old ** 2 + (mu_old - m) ** 2) / (2 * s ** 2) - 0.5).sum(-1).mean()
            grads = flat(torch.autograd.grad(kl, params, create_graph=True))
            return flat(torch.autograd.grad((grads * v).sum(), params)) + ex.CG_DAMPING * v

        out = FisherProduct.like(pol, d['obs'], idx=idx)
        gout = {}

        def new_fvp():
            return fisher_vector_product_from_records(lay, rec, v, pol, damping=ex.CG_DAMPING, idx=idx, out=out)

        def new_gradient():
            gout['p'] = policy_gradient_from_records(lay, rec, adv, adv, pol, clip=0.2, idx=idx, out=gout.get('p'))

        ref, got = torch_fvp(), new_fvp()
        torch.cuda.synchronize()
        row = dict(rows=label, rel_diff=float((got - ref).norm() / ref.norm()))
        for _ in range(2):                                                    # alternate: torch, new, gradient, torch, ...
            for tag, fn in (('torch_fvp', torch_fvp), ('fvp', new_fvp), ('policy_gradient', new_gradient)):
                row.setdefault(tag, []).append(timed(fn, args.reps))
        row['fvp_over_gradient'] = round(row['fvp'][-1]['median_ms'] / row['policy_gradient'][-1]['median_ms'], 3)
        row['torch_over_fvp'] = round(row['torch_fvp'][-1]['median_ms'] / row['fvp'][-1]['median_ms'], 2)
        print(json.dumps(row), flush=True)
        rows_out.append(row)
    # ---- a whole policy step over all rows, both ways, from the same parameters each time (accepted at j = 0 is reported)
    with torch.no_grad():
        logp_old = (-0.5 * ((d['action'] - actor((d['obs'] - shift) * scale)) / std) ** 2 - log_std).sum(-1) - 0.5 * k * 1.8378770664093453
    saved = [p.detach().clone() for p in params]
    res = {}

    def restore():
        with torch.no_grad():
            for p, s in zip(params, saved):
                p.copy_(s)
            std.copy_(log_std.exp())

    def new_step():
        restore()
        res['new'] = trpo_step(lay, rec, adv, logp_old, pol, log_std, max_kl=ex.MAX_KL, ent_coeff=ex.ENT_COEFF)

    fo, fa = d['obs'].reshape(T * B, D).contiguous(), d['action'].reshape(T * B, k).contiguous()

    def torch_step():
        restore()
        res['torch'] = ex.torch_trpo_step(actor, log_std, shift, scale, fo, fa, adv.reshape(-1), logp_old.reshape(-1))

    row = dict(rows='trpo_step, M = 983040')
    for _ in range(2):
        for tag, fn in (('torch', torch_step), ('new', new_step)):
            row.setdefault(tag, []).append(timed(fn, args.reps, warmup=1))
    row['results'] = {k_: {n: (round(x, 6) if isinstance(x, float) else x) for n, x in r.items()} for k_, r in res.items()}
    row['torch_over_new'] = round(row['torch'][-1]['median_ms'] / row['new'][-1]['median_ms'], 2)
    print(json.dumps(row), flush=True)
    rows_out.append(row)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(rows_out, fh, indent=1)


if __name__ == '__main__':
    main()
