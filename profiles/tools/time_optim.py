#!/usr/bin/env python3
"""Times the optimiser step of a PPO minibatch as libatacom_optim.so makes it (rl_on_manifold_amd/optim.py) against the torch
code it replaces, and a whole epoch of minibatches three ways.  float32, iiwa-sized networks (D = 18, k = 5).  Needs a GPU;
results: profiles/optim.md.

    python profiles/tools/time_optim.py [--reps 50] [--epochs 5] [--out FILE]

(a) one update, on the same gradients: `Adam.step(gp, gc)` -- one launch -- against what examples/ppo_air_hockey.py did after
    its two gradient calls: gc.flat.mul_(0.5), the two to_module(), torch.optim.Adam.step() and std.copy_(log_std.exp()).
(b) one epoch: 30 minibatches of 16384 rows gathered from T x B = 120 x 4096 = 491520, as (1) that loop with torch's Adam, (2) the
    same Python loop with the new Adam, (3) GraphedUpdate.replay().  Each includes drawing its permutation.

Reported per variant: the time from device events over back-to-back repetitions (what the GPU spends: kernels and the gaps
between them) and the host's wall time of one repetition that ends in a synchronise, named separately.  The variants alternate
inside one process (torch, new, graph, torch, new, graph, ...), every round is kept, and the parameters are put back to the same
start before each timing so that no variant runs on another's weights.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from rl_on_manifold_amd import (Adam, GraphedUpdate, MlpPolicy, RecordLayout, log_prob_from_records,      # noqa: E402
                                policy_gradient_from_records, value_gradient_from_records)


class Net(nn.Module):      # the example's network (the reference's PPONetwork)
    def __init__(self, n_in, n_out, h=64):
        super().__init__()
        self._h1, self._h2, self._h3 = nn.Linear(n_in, h), nn.Linear(h, h), nn.Linear(h, n_out)


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
    ap.add_argument('--reps', type=int, default=50, help='repetitions of one update per timing')
    ap.add_argument('--epochs', type=int, default=5, help='repetitions of one epoch per timing')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_optim.py measures on a GPU; there is none')
    dev, T, B, D, k, clip, mb, lr = torch.device('cuda:0'), 120, 4096, 18, 5, 0.2, 16384, 3e-4
    torch.manual_seed(0)
    actor, critic = Net(D, k).to(dev), Net(D, 1).to(dev)
    log_std = torch.full((k,), -0.7, device=dev, requires_grad=True)
    std = log_std.detach().exp()
    pol, cri = MlpPolicy.from_module(actor, std=std), MlpPolicy.from_module(critic)
    lay = RecordLayout([B], D, k)
    rec = torch.randn((T, B, lay.F), device=dev)
    rec[..., lay.fields['action']] *= 0.3
    adv, ret = torch.randn((T, B), device=dev), torch.randn((T, B), device=dev)
    logp_old = (log_prob_from_records(lay, rec, pol) + 0.2 * torch.randn((T, B), device=dev)).contiguous()
    old = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()) + [log_std], lr=lr)
    new = Adam([dict(net=pol, log_std=log_std, std=std), dict(net=cri, scale=0.5)], lr=lr)
    start = new.snapshot()                                                # parameters, log std, std (and the new Adam's state)
    idx = torch.randperm(T * B, device=dev)[:mb]
    gp = policy_gradient_from_records(lay, rec, adv, logp_old, pol, clip=clip, idx=idx)
    gc = value_gradient_from_records(lay, rec, ret, cri, idx=idx)
    rows = []

    # ---- (a) one update on the same gradients
    def torch_update():
        gc.flat.mul_(1.0)                                                 # the loop's mul_(0.5), without shrinking the one gradient
        gp.to_module(actor, log_std)
        gc.to_module(critic)
        old.step()
        std.copy_(log_std.detach().exp())

    def new_update():
        new.step(gp, gc)

    row = dict(what='(a) one update, 18 -> 5 with log std and 18 -> 1')
    for _ in range(args.rounds):
        for tag, fn in (('torch', torch_update), ('new', new_update)):
            new.restore(start)
            ev, wall = timed(fn, args.reps)
            row.setdefault(tag + '_event_ms', []).append(round(ev, 4))
            row.setdefault(tag + '_wall_ms', []).append(round(wall, 4))
    print(json.dumps(row), flush=True)
    rows.append(row)

    # ---- (b) one epoch of 30 minibatches
    out = {}

    def epoch_torch():
        perm = torch.randperm(T * B, device=dev)
        for i in range(0, T * B, mb):
            ix = perm[i:i + mb]
            out['p'] = policy_gradient_from_records(lay, rec, adv, logp_old, pol, clip=clip, idx=ix, out=out.get('p'))
            out['c'] = value_gradient_from_records(lay, rec, ret, cri, idx=ix, out=out.get('c'))
            out['c'].flat.mul_(0.5)
            out['p'].to_module(actor, log_std)
            out['c'].to_module(critic)
            old.step()
            std.copy_(log_std.detach().exp())

    def epoch_new():
        perm = torch.randperm(T * B, device=dev)
        for i in range(0, T * B, mb):
            ix = perm[i:i + mb]
            out['p'] = policy_gradient_from_records(lay, rec, adv, logp_old, pol, clip=clip, idx=ix, out=out.get('p'))
            out['c'] = value_gradient_from_records(lay, rec, ret, cri, idx=ix, out=out.get('c'))
            new.step(out['p'], out['c'])

    new.restore(start)
    graph = GraphedUpdate(lay, rec, adv, ret, logp_old, pol, cri, new, mb, clip=clip)
    row = dict(what='(b) one epoch: %d minibatches of %d rows from %d' % (len(graph._slices), mb, T * B))
    for _ in range(args.rounds):
        for tag, fn in (('torch_loop', epoch_torch), ('new_adam_loop', epoch_new), ('graph_replay', graph.replay)):
            new.restore(start)
            ev, wall = timed(fn, args.epochs)
            row.setdefault(tag + '_event_ms', []).append(round(ev, 3))
            row.setdefault(tag + '_wall_ms', []).append(round(wall, 3))
    print(json.dumps(row), flush=True)
    rows.append(row)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(rows, fh, indent=1)


if __name__ == '__main__':
    main()
