"""Per-step time of the packed rollout kernels in the full and the compact record format (GPU).

    python profiles/tools/compact_collection_timing.py [--rounds 5] [--base-root build/ab/parent]

iiwa and planar, float32, 8192 environments x 120 steps, with pre-generated actions and with the actor MLP in the kernel.
Every round runs one child process per tree, alternating: this tree times the full format and the compact format (alternated
call by call), the base tree (--base-root: a checkout of the parent commit with its library built) the full format only -- the
A/B of the full-format kernel against its previous build in the same job.  Each figure is the median over --reps launches
of the HIP-event time around the C call (atacom_rollout_packed / atacom_rollout_compact with the counter memset), divided by
the 120 steps; the compact call's count read-back is outside the timed region.  --child runs one such measurement and prints
one JSON line (for rocprofv3: `rocprofv3 --kernel-trace --stats -d DIR -- python profiles/tools/compact_collection_timing.py
--child`).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, T = 8192, 120


def child(root, reps, formats):
    sys.path.insert(0, root)
    import torch
    import bench
    from rl_on_manifold_amd import MlpPolicy
    dev = torch.device('cuda:0')
    out = {}
    for name in ('iiwa', 'planar'):
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234)
        env, _, _ = bench.make_env(name, B, dev, gen)
        D, k = env.obs_dim, env.dims['null']
        acts = torch.rand((T, B, k), device=dev, generator=gen) * 2 - 1
        g = torch.Generator().manual_seed(0)
        pol = MlpPolicy(torch.randn(64, D, generator=g) * 0.2, torch.randn(64, generator=g) * 0.1,
                        torch.randn(64, 64, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1,
                        torch.randn(k, 64, generator=g) * 0.1, torch.zeros(k), std=torch.full((k,), 0.3))
        net = pol.as_struct(env)
        noise = torch.randn((T, B, k), device=dev, generator=gen)
        full = torch.empty((T, B, 2 * D + k + 3), device=dev)
        rec = torch.empty((T + 1, B, D + k + 3), device=dev)
        ends = torch.empty(((T - 1) * B, D + 2), device=dev)
        cnt = torch.zeros((1,), device=dev, dtype=torch.int32)
        lib, h, s = env._lib, env._h, env._stream()
        calls = {}
        for path in ('actions', 'mlp'):
            a = acts.data_ptr() if path == 'actions' else None
            n = None if path == 'actions' else C.byref(net)
            z = None if path == 'actions' else noise.data_ptr()
            calls[(path, 'full')] = lambda a=a, n=n, z=z: lib.atacom_rollout_packed(h, T, a, n, z, full.data_ptr(), B, s)
            calls[(path, 'compact')] = lambda a=a, n=n, z=z: lib.atacom_rollout_compact(
                h, T, a, n, z, rec.data_ptr(), B, ends.data_ptr(), ends.shape[0], cnt.data_ptr(), s)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for path in ('actions', 'mlp'):
            for fmt in formats:                                   # warm-up
                assert calls[(path, fmt)]() == 0
            times = {fmt: [] for fmt in formats}
            for i in range(reps):
                for fmt in formats:                               # alternated launch by launch
                    e0, e1 = ev[i]
                    e0.record()
                    assert calls[(path, fmt)]() == 0
                    e1.record()
                    e1.synchronize()
                    times[fmt].append(e0.elapsed_time(e1) * 1e3 / T)
            for fmt in formats:
                out['%s/%s/%s' % (name, path, fmt)] = statistics.median(times[fmt])
            if 'compact' in formats:
                out['%s/%s/n_ends' % (name, path)] = int(cnt.item())
        env.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--base-root', default=None, help='a checkout of the parent commit, library built (full format only)')
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--formats', default='full,compact')
    args = ap.parse_args()
    if args.child:
        return child(args.root, args.reps, args.formats.split(','))
    runs = [('branch', ROOT, 'full,compact')] + ([('base', os.path.abspath(args.base_root), 'full')] if args.base_root else [])
    res = {tag: [] for tag, _, _ in runs}
    for r in range(args.rounds):
        for tag, root, fmts in (runs if r % 2 == 0 else runs[::-1]):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--root', root, '--reps', str(args.reps),
                                '--formats', fmts], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit('child %s failed (exit %d)' % (tag, p.returncode))
            res[tag].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print('round %d %-6s %s' % (r, tag, res[tag][-1]), flush=True)
    print('\nmedian over %d rounds, us per step (8192 environments x 120 steps, float32):' % args.rounds)
    print('%-16s %10s %10s %8s %10s %8s %8s' % ('case', 'full', 'compact', 'delta', 'base full', 'delta', 'n_ends'))
    for name in ('iiwa', 'planar'):
        for path in ('actions', 'mlp'):
            key = '%s/%s' % (name, path)
            med = lambda tag, f: statistics.median(x['%s/%s' % (key, f)] for x in res[tag])      # noqa: E731
            full, comp = med('branch', 'full'), med('branch', 'compact')
            base = med('base', 'full') if res.get('base') else float('nan')
            n = res['branch'][-1]['%s/n_ends' % key]
            print('%-16s %10.3f %10.3f %+7.2f%% %10.3f %+7.2f%% %8d' % (key, full, comp, 100 * (comp / full - 1), base,
                                                                      100 * (full / base - 1), n))


if __name__ == '__main__':
    main()
