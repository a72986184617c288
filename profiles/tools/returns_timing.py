"""Time libatacom_returns.so against the Python loop it replaces (profiles/returns.md), with HIP events on one GPU.

    python profiles/tools/returns_timing.py [--sizes 8192,65536,1048576] [--dtypes f32,f64] [--layouts arrays,full,compact]
                                            [--steps 120] [--reps 200] [--sets 4] [--no-loop] [--out FILE.json]

Per (size, layout, dtype): microseconds per call -- HIP events around `reps` calls enqueued back to back, so the figure includes
whatever of the Python enqueue the GPU does not hide; kernel times come from a rocprofv3 --kernel-trace run of this tool -- of
compute_gae (plain and with normalize=True) and of compute_J, the algorithmic
bytes (what the recurrence must read and write: five inputs and two outputs per sample) over that time, and the same computation
by the loop `for t in reversed(range(T))` of examples/ppo_air_hockey.py before it called the library (five torch kernels per
step, then the normalisation) on the same data as contiguous arrays.  Record widths: iiwa (D 18, k 5) up to 65536 environments,
the collision-avoidance task (D 20, k 2) above.  ATACOM_RETURNS_LIB selects another build of the library (load-ahead depth)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from rl_on_manifold_amd import compute_gae, compute_J                                  # noqa: E402
from rl_on_manifold_amd.rollout import compact_record_fields, record_columns, record_fields       # noqa: E402

DEV = 'cuda:0'
HBM = 8.0e12          # bytes / s, MI355X peak


def timed(fn, reps, warmup=3):
    """fn(i) is call number i: the caller rotates its buffer sets with it."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # microseconds per call


def loop_gae(rew, ab, last, v, nv, gamma, lam, normalize):
    """examples/ppo_air_hockey.py:74-84 of the parent commit, the critic left out."""
    T, B = rew.shape
    nv = torch.where(ab, torch.zeros_like(nv), nv)
    adv = torch.zeros_like(rew)
    g = torch.zeros(B, device=rew.device, dtype=rew.dtype)
    for t in reversed(range(T)):
        delta = rew[t] + gamma * nv[t] - v[t]
        g = delta + gamma * lam * torch.where(last[t], torch.zeros_like(g), g)
        adv[t] = g
    ret = adv + v
    if normalize:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    return ret, adv


def inputs(T, B, dtype, layout, D, k, gen):
    """(reward, absorbing, last, v, v_next) of the layout, and the same as contiguous arrays with bool flags."""
    r = torch.randn((T, B), device=DEV, dtype=dtype, generator=gen)
    last = torch.rand((T, B), device=DEV, generator=gen) < 0.01
    ab = last & (torch.rand((T, B), device=DEV, generator=gen) < 0.5)
    v = torch.randn((T + 1, B), device=DEV, dtype=dtype, generator=gen)
    vn = torch.randn((T, B), device=DEV, dtype=dtype, generator=gen)
    arrays = (r, ab, last, v[:T].contiguous(), vn)
    if layout == 'arrays':
        return arrays, arrays
    if layout == 'full':
        fields, F = record_fields(D, k)
        rec = torch.empty((T, B, F), device=DEV, dtype=dtype)
        body = rec
    else:
        fields, F, _ = compact_record_fields(D, k)
        rec = torch.empty((T + 1, B, F), device=DEV, dtype=dtype)
        body = rec[:T]
    for name, x in (('reward', r), ('absorbing', ab), ('last', last)):
        body[..., fields[name]] = x.to(dtype)
    c = record_columns(body, {n: fields[n] for n in ('reward', 'absorbing', 'last')})
    return (c['reward'], c['absorbing'], c['last'], v[:T] if layout == 'compact' else arrays[3], vn), arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='8192,65536,1048576')
    ap.add_argument('--dtypes', default='f32,f64')
    ap.add_argument('--layouts', default='arrays,full,compact')
    ap.add_argument('--steps', type=int, default=120)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--sets', type=int, default=4, help='distinct buffer sets used in turn (up to 65536 environments)')
    ap.add_argument('--no-loop', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    T, gamma, lam = args.steps, 0.99, 0.95
    rows = []
    for B in (int(s) for s in args.sizes.split(',')):
        D, k = (18, 5) if B <= 65536 else (20, 2)
        for dt in args.dtypes.split(','):
            dtype = {'f32': torch.float32, 'f64': torch.float64}[dt]
            elem = 4 if dt == 'f32' else 8
            loop = {}
            for layout in args.layouts.split(','):
                # `sets` distinct copies of the inputs and outputs, used in turn: consecutive calls do not find their data in the
                # 256 MB last-level cache (one set is 173 MB at 65536 environments in float32); above 65536 one set is far larger
                n_sets = args.sets if B <= 65536 else 1
                sets = []
                for i in range(n_sets):
                    gen = torch.Generator(device=DEV).manual_seed(1 + i)
                    xi, ai = inputs(T, B, dtype, layout, D, k, gen)
                    sets.append((xi, ai, (torch.empty((T, B), device=DEV, dtype=dtype), torch.empty((T, B), device=DEV, dtype=dtype))))
                x, arrays, out = sets[0]
                pick = lambda i: sets[i % n_sets]                  # noqa: E731
                row = dict(envs=B, steps=T, dtype=dt, layout=layout, sets=n_sets, reps=args.reps,
                           lib=os.environ.get('ATACOM_RETURNS_LIB', 'default'))
                row['gae_us'] = timed(lambda i: compute_gae(*pick(i)[0], gamma, lam, out=pick(i)[2]), args.reps)
                row['gae_normalize_us'] = timed(lambda i: compute_gae(*pick(i)[0], gamma, lam, out=pick(i)[2], normalize=True), args.reps)
                row['J_us'] = timed(lambda i: compute_J(pick(i)[0][0], pick(i)[0][2], gamma), args.reps)
                flag = 1 if layout == 'arrays' else elem
                row['algorithmic_bytes'] = T * B * (5 * elem + 2 * flag)
                row['algorithmic_GBps'] = row['algorithmic_bytes'] / row['gae_us'] / 1e3
                row['algorithmic_rate_over_hbm_peak'] = row['algorithmic_bytes'] / (row['gae_us'] * 1e-6) / HBM
                if not args.no_loop:
                    if not loop:          # the loop reads contiguous arrays whatever the collection's layout: measured once per (B, dtype)
                        reps = max(2, min(args.reps, 30))
                        loop['loop_us'] = timed(lambda i: loop_gae(*pick(i)[1], gamma, lam, False), reps, warmup=1)
                        loop['loop_normalize_us'] = timed(lambda i: loop_gae(*pick(i)[1], gamma, lam, True), reps, warmup=1)
                        ref = loop_gae(*arrays, gamma, lam, False)
                        got = compute_gae(*x, gamma, lam)
                        loop['max_abs_difference_from_loop'] = float((got[1] - ref[1]).abs().max())
                    row.update(loop)
                    row['speedup'] = row['loop_us'] / row['gae_us']
                    row['speedup_normalize'] = row['loop_normalize_us'] / row['gae_normalize_us']
                rows.append(row)
                print(json.dumps(row), flush=True)
                del x, arrays, out, sets
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
