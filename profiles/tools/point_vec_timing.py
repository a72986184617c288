"""The collision-avoidance task driven step by step: masked step, graphed loop and checkpoint, timed (GPU).

    python profiles/tools/point_vec_timing.py step     [--json FILE]     masked against plain step, 8192 and 1 M environments
    python profiles/tools/point_vec_timing.py graph    [--json FILE]     GraphedRollout against the host loop of rollout_policy
    python profiles/tools/point_vec_timing.py snapshot [--json FILE]     snapshot() and restore() at 1 M environments

One process per mode (a job runs them one after the other, each under its own time limit).  float32, 4 obstacles,
random_walk, generator draws, in-kernel auto-reset at the task's horizon of 1000 with the episode step counters staggered
b % 1000 (profiles/tools/point_compact_timing.py).  Every figure is between two HIP events; the sides of a comparison alternate
in the one process, burst by burst, after a warm-up of every side.

step      bursts of --burst calls of step_into() / step_into(mask=ones) / step_into(mask=half), --bursts bursts of each (20 x 15 =
          300 calls a side); a figure is a burst's time over its calls, the median over the bursts reported with min .. max.  Back to
          back calls of a 2 us kernel measure the launch path, which is what a caller of step() pays.  Bytes per environment and
          call are computed from the shapes, as the kernel is written: a masked-in lane reads its 9 state groups, its counters, its
          action and its mask byte and writes them back with the observation row, the reward and two flags; a masked-out lane
          reads 8 groups, _time, three counters and its mask byte and writes the row, the reward and two flags.
graph     T = 120 at 8192 environments with the same torch callable, a 2 x 64 nn.Sequential that is not an MlpPolicy:
          loop.replay() against env.rollout_policy(net, T) (the host loop), alternated call by call, --reps of each.
snapshot  --reps of snapshot(out=image) and restore(image) alternated; bytes = the image read or written once and the
          handle's buffers once; the share of the HBM roof uses 8.0 TB/s, as profiles/point_policy.md does.  restore()
          synchronises the stream twice to read the 64-byte header (inspect, then restore): its figure includes that.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HORIZON, N_OBJ, HBM = 1000, 4, 8.0e12


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


def _timed(fn):
    """microseconds between two events around fn(), and on the host clock up to the second event's completion"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, (time.perf_counter() - t0) * 1e6


def _summary(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'n': len(v)}


def step_bytes(n=N_OBJ, elem=4):
    groups = (4 * (1 + n) + 3 * n + 3 + 3) // 4                  # csrc/atacom_point.h: Layout<N>::GROUPS
    row = 4 * (1 + n) * elem
    state = groups * 4 * elem + 16                               # every group and the int4 of counters
    active = (state + 2 * elem + 1) + (state + row + elem + 2)
    sitting = ((groups - 1) * 4 * elem + elem + 12 + 1) + (row + elem + 2)
    ideal_sitting = (row + 1) + (row + elem + 2)                 # a lane that read its observation groups only
    return {'plain': active - 1, 'masked_in': active, 'masked_out': sitting, 'masked_out_obs_groups_only': ideal_sitting}


def mode_step(args, dev):
    import torch
    res = {'bytes_per_env_call': step_bytes()}
    by = res['bytes_per_env_call']
    for B in (8192, 1 << 20):
        env = _env(B, dev)
        g = torch.Generator().manual_seed(1)
        act = (torch.rand((B, 2), generator=g) * 2 - 1).to(dev)
        half = (torch.rand((B,), generator=g) < 0.5).to(torch.uint8).to(dev)
        ones = torch.ones((B,), dtype=torch.uint8, device=dev)
        io = dict(obs=torch.empty((B, env.obs_dim), device=dev), reward=torch.empty((B,), device=dev),
                  absorbing=torch.empty((B,), device=dev, dtype=torch.uint8), last=torch.empty((B,), device=dev, dtype=torch.uint8))
        sides = {'plain': None, 'mask=ones': ones, 'mask=half': half}

        def burst(mask):
            for _ in range(args.burst):
                env.step_into(act, mask=mask, **io)
        for m in sides.values():
            burst(m)
        torch.cuda.synchronize()
        times = {k: [] for k in sides}
        for _ in range(args.bursts):
            for k, m in sides.items():
                times[k].append(_timed(lambda: burst(m))[0] / args.burst)
        share = float(half.float().mean())
        per_env = {'plain': by['plain'], 'mask=ones': by['masked_in'],
                   'mask=half': share * by['masked_in'] + (1 - share) * by['masked_out']}
        res[str(B)] = r = {k: dict(_summary(v), bytes_per_call=B * per_env[k]) for k, v in times.items()}
        r['half_mask_share_in'] = share
        print('\n%d environments: us per call, median (min .. max) of %d bursts of %d calls' % (B, args.bursts, args.burst))
        for k in sides:
            v = r[k]
            print('%-10s %9.2f (%8.2f .. %8.2f)   %12.0f B per call   %6.3f of the HBM roof'
                  % (k, v['median'], v['min'], v['max'], v['bytes_per_call'], v['bytes_per_call'] / (v['median'] * 1e-6) / HBM), flush=True)
        env.close()
    return res


def mode_graph(args, dev):
    import torch
    from rl_on_manifold_amd import GraphedRollout
    B, T = 8192, 120
    env = _env(B, dev)
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(env.obs_dim, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                              torch.nn.Linear(64, 2)).to(dev)
    for p in net.parameters():
        p.requires_grad_(False)
    loop = GraphedRollout(env, net, T)
    sides = {'graph': loop.replay, 'host loop': lambda: env.rollout_policy(net, T)}
    for fn in sides.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ev, host = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(args.reps):
        for k, fn in sides.items():
            a, b = _timed(fn)
            ev[k].append(a / T)
            host[k].append(b / T)
    res = {'B': B, 'T': T}
    print('\n%d environments x %d steps, 2 x 64 nn.Sequential: us per step, median (min .. max) of %d collections' % (B, T, args.reps))
    for k in sides:
        res[k] = {'events': _summary(ev[k]), 'host_clock': _summary(host[k])}
        print('%-10s events %8.2f (%8.2f .. %8.2f)   host clock %8.2f (%8.2f .. %8.2f)'
              % (k, res[k]['events']['median'], res[k]['events']['min'], res[k]['events']['max'],
                 res[k]['host_clock']['median'], res[k]['host_clock']['min'], res[k]['host_clock']['max']), flush=True)
    print('host loop / graph = %.1f' % (res['host loop']['events']['median'] / res['graph']['events']['median']))
    env.close()
    return res


def mode_snapshot(args, dev):
    import torch
    B = 1 << 20
    env = _env(B, dev)
    image = torch.empty_like(env.snapshot())
    sides = {'snapshot': lambda: env.snapshot(out=image), 'restore': lambda: env.restore(image)}
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ev, host = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(args.reps):
        for k, fn in sides.items():
            a, b = _timed(fn)
            ev[k].append(a)
            host[k].append(b)
    moved = 2 * (image.numel() - 64) + 64
    res = {'B': B, 'image_bytes': image.numel(), 'bytes_moved': moved}
    print('\n%d environments, image of %d bytes, %d bytes moved per call: us per call, median (min .. max) of %d'
          % (B, image.numel(), moved, args.reps))
    for k in sides:
        res[k] = {'events': _summary(ev[k]), 'host_clock': _summary(host[k])}
        v = res[k]['events']
        print('%-10s events %8.2f (%8.2f .. %8.2f)   host clock %8.2f   %6.3f of the HBM roof'
              % (k, v['median'], v['min'], v['max'], res[k]['host_clock']['median'], moved / (v['median'] * 1e-6) / HBM), flush=True)
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('step', 'graph', 'snapshot'))
    ap.add_argument('--burst', type=int, default=20)
    ap.add_argument('--bursts', type=int, default=15)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--json', default=None, help='also write the figures to this file')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    res = {'step': mode_step, 'graph': mode_graph, 'snapshot': mode_snapshot}[args.mode](args, torch.device('cuda:0'))
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
