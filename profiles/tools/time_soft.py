"""python profiles/tools/time_soft.py [--reps N] [--trace]

soft_td_target, soft_critic_gradient (a pair) and soft_actor_gradient of libatacom_soft.so (float32, iiwa-sized networks) on the
columns of a replay memory in place: blocks of back-to-back calls between device events, medians and spread, at 256 rows and at
16384 rows gathered from 983040.  --reps N: the calls of a block (default 50; 21 blocks).  ATACOM_SOFT_LIB selects the build under
test: the tool behind the timing tables of profiles/offpolicy_backward_shared.md, run there on the parent's library, this
commit's and the parent's again, a fresh process each.  With --trace: 200 calls of each at 16384 and 256 rows and nothing else,
the workload of rocprofv3 --kernel-trace --stats -- python profiles/tools/time_soft.py --trace."""
import math, os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rl_on_manifold_amd import MlpPolicy, ReplayMemory, SoftCritic

dev = torch.device('cuda:0')
torch.manual_seed(0)
D, k, N = 18, 5, 983040
calls = int(sys.argv[sys.argv.index('--reps') + 1]) if '--reps' in sys.argv else 50

def net(n_in, n_out):
    lin = lambda o, i: [torch.randn(o, i, device=dev) / math.sqrt(i), 0.1 * torch.randn(o, device=dev)]      # noqa: E731
    return lin(64, n_in) + lin(64, 64) + lin(n_out, 64)

pol = MlpPolicy(*net(D, k), sigma_weights=net(D, k), squash=True, log_std_min=-20.0, log_std_max=2.0)
crs, tgs = ([SoftCritic(*net(D + k, 1), n_act=k) for _ in range(2)] for _ in range(2))
la = torch.tensor([math.log(0.2)], device=dev)
mem = ReplayMemory(N, D, k, device=dev)
mem.storage.normal_()
mem.size = N

def say(s):
    print(s, flush=True)

def block(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3          # microseconds per call

def measure(fns, blocks=21):
    for fn in fns.values():                          # warm-up of every call
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = {n: [] for n in fns}
    for _ in range(blocks):
        for n, fn in fns.items():                    # alternating
            t[n].append(block(fn))
    for n, v in t.items():
        v.sort()
        say('%-40s median %9.2f us  min %9.2f  max %9.2f  (%d blocks of %d calls)' % (n, statistics.median(v), v[0], v[-1], blocks, calls))

for M in (16384, 256):
    idx, eps = mem.sample(M), torch.randn(M, k, device=dev).clamp_(-2.0, 2.0)
    y = mem.soft_td_target(pol, tgs, idx, 0.99, la, eps)
    gs = mem.soft_critic_gradient(crs, idx, y)
    ga = mem.soft_actor_gradient(pol, crs, idx, eps, la, -float(k))
    assert all(torch.isfinite(t).all() for t in (y, gs[0].flat, gs[1].flat, ga.mu.flat, ga.sigma.flat, ga.stats))
    if '--trace' in sys.argv:
        for _ in range(200):
            mem.soft_td_target(pol, tgs, idx, 0.99, la, eps, out=y)
            mem.soft_critic_gradient(crs, idx, y, out=gs)
            mem.soft_actor_gradient(pol, crs, idx, eps, la, -float(k), out=ga)
        torch.cuda.synchronize()
        continue
    measure({'soft_td_target %d rows' % M: lambda: mem.soft_td_target(pol, tgs, idx, 0.99, la, eps, out=y),
             'soft_critic_gradient (pair) %d rows' % M: lambda: mem.soft_critic_gradient(crs, idx, y, out=gs),
             'soft_actor_gradient %d rows' % M: lambda: mem.soft_actor_gradient(pol, crs, idx, eps, la, -float(k), out=ga)})
