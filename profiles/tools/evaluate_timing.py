#!/usr/bin/env python3
"""Times the network evaluation of one PPO iteration -- V(obs), V(next_obs) and the log-probability of the recorded actions --
as libatacom_evaluate.so runs it (rl_on_manifold_amd/evaluate.py) against the torch code it replaces: the module calls and the
log-probability expression of examples/ppo_air_hockey.py before this library, on the same tensors, under torch.no_grad() and
after warm-up.  T = 120, float32, B = 8192 and 65536, an iiwa-sized (D = 18, k = 5) and a point-sized (D = 12, k = 2) pair of
networks, on separate arrays, on full packed records and on compact records.  Needs a GPU; results: profiles/evaluate.md.

    python profiles/tools/evaluate_timing.py [--reps 20] [--only new|torch] [--batches 8192,65536] [--out FILE]

Reported per configuration: the time of the whole stage from device events over `reps` back-to-back repetitions (what the GPU
spends: kernels and the gaps between them), the host's wall time of one call that ends in a synchronise, and the share of the
HBM peak that the ALGORITHMIC bytes make of the event time -- every input row read once, every output written once.  Kernel
times proper come from a run of this script under `rocprofv3 --kernel-trace --stats` with --only new (one variant, few reps).
The two variants alternate inside one process, and their outputs are compared before anything is timed.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from rl_on_manifold_amd import (CompactRecordLayout, MlpPolicy, RecordLayout, evaluate_mlp, gaussian_log_prob,      # noqa: E402
                                log_prob_from_records, values_from_compact, values_from_records)

HBM_PEAK = 8.0e12          # bytes / s, MI355X


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
    ap.add_argument('--batches', default='8192,65536')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('evaluate_timing.py measures on a GPU; there is none')
    dev, T = torch.device('cuda:0'), 120
    torch.manual_seed(0)
    rows_out = []
    for B in [int(b) for b in args.batches.split(',')]:
        for label, D, k in (('iiwa', 18, 5), ('point', 12, 2)):
            actor, critic = Net(D, k).to(dev), Net(D, 1).to(dev)
            shift, scale = torch.randn(D, device=dev) * 0.1, torch.rand(D, device=dev) + 0.5
            log_std = torch.full((k,), -0.7, device=dev)
            pol = MlpPolicy.from_module(actor, std=log_std.exp())
            cri = MlpPolicy.from_module(critic)
            for p in (pol, cri):
                p.tensors['obs_shift'], p.tensors['obs_scale'] = shift, scale
            norm = lambda o: (o - shift) * scale                                     # noqa: E731
            lay, clay = RecordLayout([B], D, k), CompactRecordLayout([B], D, k, T)
            full = torch.randn((T, B, lay.F), device=dev)
            comp = torch.randn((T + 1, B, clay.Fc), device=dev)
            M = T * B // 60                                    # one episode end per environment and 60 steps
            ends = torch.randn((M, clay.E), device=dev)
            d = lay.unpack(full)
            obs, nobs, act = d['obs'].contiguous(), d['next_obs'].contiguous(), d['action'].contiguous()
            R = T * B

            def torch_stage(o, no, a):
                with torch.no_grad():
                    v, nv = critic(norm(o)).squeeze(-1), critic(norm(no)).squeeze(-1)
                    mu = actor(norm(o))
                    return v, nv, (-0.5 * ((a - mu) / log_std.exp()) ** 2 - log_std).sum(-1)

            def torch_compact():
                with torch.no_grad():
                    o = comp[..., clay.compact_fields['obs']]
                    v, ve = critic(norm(o)).squeeze(-1), critic(norm(ends[:, 2:])).squeeze(-1)
                    mu = actor(norm(o[:T]))
                    return v, ve, (-0.5 * ((comp[:T, :, clay.compact_fields['action']] - mu) / log_std.exp()) ** 2 - log_std).sum(-1)

            half_log_2pi_k = 0.5 * k * 1.8378770664093453
            variants = {
                'arrays': (lambda: torch_stage(obs, nobs, act),
                           lambda: (evaluate_mlp(cri, obs).squeeze(-1), evaluate_mlp(cri, nobs).squeeze(-1), gaussian_log_prob(pol, obs, act)),
                           R * 4 * (2 * D + 2 + D + k + 1)),
                'full records': (lambda: torch_stage(d['obs'], d['next_obs'], d['action']),
                                 lambda: values_from_records(lay, full, cri) + (log_prob_from_records(lay, full, pol),),
                                 R * 4 * (2 * D + 2 + D + k + 1)),
                'compact records': (torch_compact,
                                    lambda: values_from_compact(clay, comp, ends, M, cri) + (log_prob_from_records(clay, comp, pol),),
                                    4 * (((T + 1) * B + M) * (D + 1) + R * (D + k + 1))),
            }
            for name, (old, new, nbytes) in variants.items():
                a, b = old(), new()
                torch.cuda.synchronize()
                diff = [float((x - y).abs().max()) for x, y in zip(a[:2], b[:2])]
                diff.append(float((a[2] - half_log_2pi_k - b[2]).abs().max()))       # the example's expression leaves the constant out
                del a, b
                row = dict(B=B, net=label, layout=name, rows=R, max_abs_diff=diff, algorithmic_MB=nbytes / 1e6)
                for _ in range(2):                                                    # alternate: torch, new, torch, new
                    for tag, fn in (('torch', old), ('new', new)):
                        if args.only in (None, tag):
                            ev, wall = timed(fn, args.reps)
                            row.setdefault(tag + '_event_ms', []).append(round(ev, 4))
                            row.setdefault(tag + '_wall_ms', []).append(round(wall, 4))
                if 'new_event_ms' in row:
                    row['new_hbm_share'] = round(nbytes / (min(row['new_event_ms']) * 1e-3) / HBM_PEAK, 4)
                if 'torch_event_ms' in row:
                    row['torch_hbm_share'] = round(nbytes / (min(row['torch_event_ms']) * 1e-3) / HBM_PEAK, 4)
                print(json.dumps(row), flush=True)
                rows_out.append(row)
            del full, comp, ends, d, obs, nobs, act
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(rows_out, fh, indent=1)


if __name__ == '__main__':
    main()
