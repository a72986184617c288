"""Time k_point_rollout (the T-step kernel of the collision-avoidance task) with HIP events, the way bench.py times blocks.

    python profiles/tools/point_reach_bench.py [--out FILE.json]          (from the repository root, on the GPU)

Configurations: n_objects 4, random_walk True, float32, generator draws, at 8192 and at 1 M environments.  Per env-step it
reports the time and the fraction of the HBM roof, from the ALGORITHMIC bytes of a launch:

    actions in            2 values                       (counted ONCE: out['action'] is the input tensor, not an output)
    obs, next_obs out     2 x 4 (1 + n) values
    reward out            1 value
    absorbing, last out   2 bytes
    state in + out        the handle's per-environment record, once per launch (amortised over the T steps)

The same kernel is also timed without next_obs (what a collector that rebuilds it from obs needs).  Each figure is the
median of REPEATS windows of `reps` launches each, after warm-up launches of the same shape; the spread is printed.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from rl_on_manifold_amd import BatchedPointReachEnv     # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X: HBM3E 8 TB/s (the constant bench.py uses)
REPEATS = 5


def algorithmic_bytes(n, B, T, want_next_obs, esz=4):
    per_step = 2 * esz + (2 if want_next_obs else 1) * 4 * (1 + n) * esz + esz + 2
    state = 2 * (4 * ((7 * n + 7 + 3) // 4) * esz + 16)           # float groups of four + one int4, read and written
    return B * (T * per_step + state)


def time_config(B, T, reps, n=4, want_next_obs=True, dev='cuda:0'):
    env = BatchedPointReachEnv(B, n_objects=n, random_walk=True, device=dev, dtype=torch.float32, auto_reset=True, seed=1)
    env.reset()
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    acts = torch.rand((T, B, 2), device=dev, generator=g) * 2 - 1
    out = env.rollout(acts, want_next_obs=want_next_obs)
    for _ in range(2):
        env.rollout(acts, out=out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            env.rollout(acts, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    assert torch.isfinite(out['reward']).all().item()
    ms.sort()
    med = ms[len(ms) // 2]
    nbytes = algorithmic_bytes(n, B, T, want_next_obs)
    gbs = nbytes / med / 1e6
    c_avg, c_max, _ = env.get_constraints_logs()
    return {'batch': B, 'T': T, 'n_objects': n, 'next_obs': want_next_obs, 'ms_per_launch': med, 'ms_min': ms[0], 'ms_max': ms[-1],
            'us_per_step': med / T * 1e3, 'ns_per_env_step': med / T / B * 1e6, 'env_steps_per_s': B * T / med * 1e3,
            'algorithmic_bytes_per_env_step': nbytes / (B * T), 'achieved_GBs': gbs, 'hbm_frac': gbs / HBM_PEAK_GBS,
            'c_avg': c_avg, 'c_max': c_max}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    rows = []
    for B, T, reps in ((8192, 500, 4), (1048576, 60, 4)):
        for nobs in (True, False):
            r = time_config(B, T, reps, want_next_obs=nobs)
            rows.append(r)
            print('point reach n=4 random walk f32 B=%d T=%d next_obs=%s: %.3f ms per launch (min %.3f max %.3f), %.2f us per step, '
                  '%.4f ns per env-step, %.3g env-steps/s, %.1f B per env-step -> %.0f GB/s = %.3f of the 8 TB/s HBM roof; c_max %.3f'
                  % (B, T, nobs, r['ms_per_launch'], r['ms_min'], r['ms_max'], r['us_per_step'], r['ns_per_env_step'],
                     r['env_steps_per_s'], r['algorithmic_bytes_per_env_step'], r['achieved_GBs'], r['hbm_frac'], r['c_max']),
                  flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
