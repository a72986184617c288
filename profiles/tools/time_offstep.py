#!/usr/bin/env python3
"""Times the optimiser step of a TD3 fit as libatacom_offstep.so makes it (rl_on_manifold_amd/offstep.py) against the calls it
replaces, and a graph replay of two fits against the eager body.  float32, planar-sized networks (D = 20, k = 2, TD3 critics of
22 first-layer inputs).  Needs a GPU; results: profiles/offstep.md.

    python profiles/tools/time_offstep.py [--minibatch 16384] [--blocks 11] [--reps 20]

(a) one step, on the same gradients: `TrackedAdam.step(ga, gq1, gq2)` -- one launch: three Adam steps, three targets follow --
    against torch.optim.Adam over the two critics (their .grad set once by QGradients.to_module), the device Adam over the actor
    and soft_update of the three pairs: what examples/td3_air_hockey.py --step torch does after its gradient calls.
(b) `GraphedFit.replay()` against `GraphedFit.eager()`: two fits, each drawing its row numbers and noise inside the timed region.

Reported per variant: the MEDIAN over `blocks` timed blocks of `reps` back-to-back repetitions, by device events (what the GPU
spends: kernels and the gaps between them) and by the host clock around a block that ends in a synchronise, per repetition.  The
variants alternate block by block inside one process, and the parameters are put back to one start before each block.
"""
import argparse
import copy
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from rl_on_manifold_amd import Adam, GraphedFit, MlpPolicy, QCritic, ReplayMemory, TrackedAdam, soft_update      # noqa: E402

D, K = 20, 2


class Actor(nn.Module):
    def __init__(self, h=64):
        super().__init__()
        self._h1, self._h2, self._h3 = nn.Linear(D, h), nn.Linear(h, h), nn.Linear(h, K)


class Critic(nn.Module):
    def __init__(self, h=64):
        super().__init__()
        self._h1, self._h2_s, self._h2_a, self._h3 = nn.Linear(D + K, h), nn.Linear(h, h), nn.Linear(K, h, bias=False), nn.Linear(h, 1)


def block(fn, reps):
    """(ms per repetition by device events, by the host clock) of one block of `reps` back-to-back calls."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, (time.perf_counter() - t0) * 1e3 / reps


def compare(variants, reset, blocks, reps):
    """{name: (median event ms, median wall ms)} with the variants alternating block by block."""
    got = {name: ([], []) for name, _ in variants}
    for name, fn in variants:                                # warm-up, not timed
        reset()
        fn()
    for _ in range(blocks):
        for name, fn in variants:
            reset()
            ev, wall = block(fn, reps)
            got[name][0].append(ev)
            got[name][1].append(wall)
    return {name: (statistics.median(ev), statistics.median(wall)) for name, (ev, wall) in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--minibatch', type=int, default=16384)
    ap.add_argument('--rows', type=int, default=65536)
    ap.add_argument('--blocks', type=int, default=11)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    torch.manual_seed(0)
    dev = torch.device('cuda:0')
    scaling = torch.ones(K, device=dev)
    low, high = -scaling, scaling.clone()
    actor, critics = Actor().to(dev), [Critic().to(dev) for _ in range(2)]
    actor_t, critics_t = copy.deepcopy(actor), [copy.deepcopy(c) for c in critics]

    def policy(net):
        pol = MlpPolicy.from_module(net)
        pol.mean_mode, pol.tensors['act_scale'] = 1, scaling
        return pol

    def critic(net):
        c = QCritic.from_module(net, D)
        c.tensors['act_scale'] = scaling
        return c

    pol, pol_t = policy(actor), policy(actor_t)
    cri, cri_t = [critic(c) for c in critics], [critic(c) for c in critics_t]
    mem = ReplayMemory(args.rows, D, K, device=dev)
    z = lambda *s: torch.randn(*s, device=dev)               # noqa: E731
    mem.add_fields(z(args.rows, D), torch.rand(args.rows, K, device=dev) * 2 - 1, z(args.rows), z(args.rows, D),
                   (torch.rand(args.rows, device=dev) < 0.05).float(), torch.zeros(args.rows, device=dev))
    M = args.minibatch
    idx = mem.sample(M)
    y = mem.td_target(pol_t, cri_t, idx, 0.99, eps=z(M, K), noise_std=0.2, noise_clip=0.5, low=low, high=high)
    gq = mem.critic_gradient(cri, idx, y)
    ga = mem.actor_gradient(pol, cri[0], idx)
    for g, net in zip(gq, critics):
        g.to_module(net)
    opt_c = torch.optim.Adam([p for c in critics for p in c.parameters()], lr=3e-4)
    opt_a = Adam([{'net': pol}], lr=1e-4)
    tracked = TrackedAdam([dict(net=pol, target=pol_t, lr=1e-4)] + [dict(net=c, target=ct, lr=3e-4) for c, ct in zip(cri, cri_t)], tau=5e-3)
    start = tracked.snapshot()

    def torch_step():
        opt_c.step()
        opt_a.step(ga)
        soft_update([pol_t] + cri_t, [pol] + cri, 5e-3)

    print('minibatch %d rows, %d blocks of %d repetitions, medians; ms per repetition' % (M, args.blocks, args.reps))
    a = compare([('torch Adam (critics) + Adam (actor) + soft_update', torch_step), ('TrackedAdam.step', lambda: tracked.step(ga, *gq))],
                lambda: tracked.restore(start), args.blocks, args.reps)
    fit = GraphedFit(mem, pol, pol_t, cri, cri_t, tracked, M, 0.99, policy_delay=2, noise_std=0.2, noise_clip=0.5, low=low, high=high)
    b = compare([('GraphedFit.eager() (two fits)', fit.eager), ('GraphedFit.replay() (two fits)', fit.replay)],
                lambda: tracked.restore(start), args.blocks, args.reps)
    for res in (a, b):
        base = None
        for name, (ev, wall) in res.items():
            base = base or (ev, wall)
            print('%-52s event %8.4f  wall %8.4f   ratio to the first: event %.3f, wall %.3f' % (name, ev, wall, ev / base[0], wall / base[1]))


if __name__ == '__main__':
    main()
