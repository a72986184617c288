"""Per-step time of the collision-avoidance task's record kernels in the full and the compact format (GPU).

    python profiles/tools/point_compact_timing.py [--rounds 5] [--reps 20] [--cases 8192x120,1048576x30] [--json FILE]

float32, 4 obstacles, random_walk, generator draws, in-kernel auto-reset at the task's horizon of 1000; pre-generated actions
and a Gaussian MlpPolicy.  ONE process: per case and path the two C calls -- atacom_point_policy_rollout_packed (full) and
atacom_point_compact_rollout (compact, with its counter memset) -- are alternated launch by launch on the same handle, each
between two HIP events; a figure is the median over --reps launches divided by the T steps, repeated over --rounds rounds
(median, min .. max of the rounds reported).  The episode step counters are staggered b % 1000 before the first launch, so
every launch sees its steady share of horizon hits, B T / 1000, and the exception list is sized to that (twice it plus a
margin), not to the worst case.  The compact call's count is read back outside the timed region.

Bytes per env-step are algorithmic: the record written (the tail row and the exception rows included) plus the action read (8 B)
or the noise read (8 B); the share of the HBM roof uses 8.0 TB/s, as profiles/point_policy.md does.  Before timing, at the first
case, one launch of each format on twin handles is compared through CompactRecordLayout.unpack (equality on every key).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HORIZON, N_OBJ, HBM = 1000, 4, 8.0e12


def _policy(D, dev):
    import torch
    from rl_on_manifold_amd import MlpPolicy
    g = torch.Generator().manual_seed(0)
    return MlpPolicy(torch.randn(64, D, generator=g) * 0.2, torch.randn(64, generator=g) * 0.1,
                     torch.randn(64, 64, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1,
                     torch.randn(2, 64, generator=g) * 0.1, torch.zeros(2), std=torch.full((2,), 0.3))


def _env(B, dev):
    import torch
    from rl_on_manifold_amd import BatchedPointReachEnv
    env = BatchedPointReachEnv(B, n_objects=N_OBJ, random_walk=True, horizon=HORIZON, seed=3, auto_reset=True, device=dev)
    env.reset()
    st = env.get_state()
    steps = (torch.arange(B, device=dev) % HORIZON).to(st.dtype)
    st[:, -3], st[:, -4] = steps, steps * 0.01           # [..., _time, steps taken, episodes started, centres set]
    env.set_state(st)
    return env


def check_equal(B, T, dev):
    import torch
    from rl_on_manifold_amd import CompactRecordLayout, RecordLayout
    a, b = _env(B, dev), _env(B, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    acts = torch.rand((T, B, 2), device=dev, generator=g) * 2 - 1
    full = RecordLayout([B], a.obs_dim, 2).unpack(a.rollout_packed(actions=acts))
    rec, ends, n = b.rollout_compact(actions=acts, ends_capacity=2 * B * T // HORIZON + 1024)
    got = CompactRecordLayout([B], a.obs_dim, 2, T).unpack(rec, ends, n)
    assert all(torch.equal(got[k], full[k]) for k in full), 'compact and full records differ'
    assert n == int(full['last'][:T - 1].sum()) and n > 0
    a.close(), b.close()
    return n


def measure(B, T, dev, reps, rounds):
    import torch
    from rl_on_manifold_amd import _lib_point_compact, _lib_point_policy
    env = _env(B, dev)
    D = env.obs_dim
    F, Fc, E = 2 * D + 5, D + 5, D + 2
    cap = 2 * B * T // HORIZON + 1024
    g = torch.Generator(device=dev).manual_seed(2)
    acts = torch.rand((T, B, 2), device=dev, generator=g) * 2 - 1
    noise = torch.randn((T, B, 2), device=dev, generator=g)
    full = torch.empty((T, B, F), device=dev)
    rec = torch.empty((T + 1, B, Fc), device=dev)
    ends = torch.empty((cap, E), device=dev)
    cnt = torch.zeros((1,), device=dev, dtype=torch.int32)
    net = _policy(D, dev).as_struct(env)
    plib, clib, h, s = _lib_point_policy.load(), _lib_point_compact.load(), env._h, env._stream()
    out = {}
    for path in ('actions', 'gaussian'):
        a, n, z = (acts.data_ptr(), None, None) if path == 'actions' else (None, C.byref(net), noise.data_ptr())
        calls = {'full': lambda: plib.atacom_point_policy_rollout_packed(h, T, a, n, z, None, full.data_ptr(), B, s),
                 'compact': lambda: clib.atacom_point_compact_rollout(h, T, a, n, z, None, rec.data_ptr(), B, ends.data_ptr(), cap,
                                                                      cnt.data_ptr(), s)}
        for fmt in calls:                                        # warm-up: code objects, the buffers' first touch
            for _ in range(2):
                assert calls[fmt]() == 0
        torch.cuda.synchronize()
        med = {fmt: [] for fmt in calls}
        n_ends = []
        for _ in range(rounds):
            times = {fmt: [] for fmt in calls}
            for _ in range(reps):
                for fmt in calls:                                # alternated launch by launch
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    assert calls[fmt]() == 0
                    e1.record()
                    e1.synchronize()
                    times[fmt].append(e0.elapsed_time(e1) * 1e3 / T)
                    if fmt == 'compact':
                        n_ends.append(int(cnt.item()))
            for fmt in calls:
                med[fmt].append(statistics.median(times[fmt]))
        assert max(n_ends) <= cap, (max(n_ends), cap)
        rows = statistics.mean(n_ends)
        written = {'full': 4.0 * F, 'compact': 4.0 * (Fc * (T + 1) / T + E * rows / (B * T))}
        for fmt in calls:
            us = statistics.median(med[fmt])
            traffic = written[fmt] + 8.0
            out['%s/%s' % (path, fmt)] = {'us_per_step': us, 'rounds_min': min(med[fmt]), 'rounds_max': max(med[fmt]),
                                          'bytes_written_per_env_step': written[fmt],
                                          'hbm_share': B * traffic / (us * 1e-6) / HBM}
        out['%s/n_ends_mean' % path] = rows
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--cases', default='8192x120,1048576x30')
    ap.add_argument('--json', default=None, help='also write the figures to this file')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    dev = torch.device('cuda:0')
    cases = [tuple(int(v) for v in c.split('x')) for c in args.cases.split(',')]
    print('equality at %d x %d: ok, %d exception rows' % (cases[0][0], cases[0][1], check_equal(cases[0][0], cases[0][1], dev)),
          flush=True)
    res = {}
    for B, T in cases:
        res['%dx%d' % (B, T)] = r = measure(B, T, dev, args.reps, args.rounds)
        print('\n%d environments x %d steps, float32, %d obstacles: us per step, median of %d rounds (min .. max) of medians of %d'
              % (B, T, N_OBJ, args.rounds, args.reps))
        print('%-10s %-8s %28s %12s %10s' % ('path', 'format', 'us per step', 'B written', 'HBM share'))
        for path in ('actions', 'gaussian'):
            for fmt in ('full', 'compact'):
                v = r['%s/%s' % (path, fmt)]
                print('%-10s %-8s %9.2f (%8.2f .. %8.2f) %12.1f %10.3f' % (path, fmt, v['us_per_step'], v['rounds_min'],
                                                                           v['rounds_max'], v['bytes_written_per_env_step'],
                                                                           v['hbm_share']))
            f, c = r[path + '/full'], r[path + '/compact']
            print('%-10s compact / full = %.3f; spread of the full format over the rounds %.1f %%; %.0f exception rows per launch'
                  % (path, c['us_per_step'] / f['us_per_step'], 100 * (f['rounds_max'] / f['rounds_min'] - 1),
                     r[path + '/n_ends_mean']), flush=True)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
