"""python profiles/tools/time_offpolicy.py [--trace]

td_target (float32, TD3, iiwa-sized networks) against the torch expression it replaces, and soft_update of three pairs against
the torch loop over parameters: blocks of calls between device events, the two versions alternating, medians and spread.
With --trace: 200 calls of td_target and q_values at 16384, 256 and 65536 rows and 200 soft updates and nothing else, the workload of  rocprofv3 --kernel-trace --stats -- python profiles/tools/time_offpolicy.py --trace  (the two network
launches alternate: even dispatches of k_offpolicy_net are targets, odd ones Q-values)."""
import os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))
from rl_on_manifold_amd import MlpPolicy, QCritic, ReplayMemory, soft_update
from td3_air_hockey import Actor, Critic

dev = torch.device('cuda:0')
torch.manual_seed(0)
D, k, N = 18, 5, 983040
scaling = torch.ones(k, device=dev)
low, high = -scaling, scaling.clone()
actor, critics = Actor(D, k, scaling).to(dev), [Critic(D, k, scaling).to(dev) for _ in range(2)]
pol = MlpPolicy.from_td3(actor, 0.01, low=-1.0, high=1.0)
pol.tensors.update(act_scale=scaling, act_low=low, act_high=high, std=torch.full((k,), 0.1, device=dev))
cri = [QCritic.from_module(c, D) for c in critics]
for c in cri:
    c.tensors['act_scale'] = scaling
mem = ReplayMemory(N, D, k, device=dev)
mem.storage.normal_()
mem.storage[:, mem.fields['absorbing']] = (torch.rand(N, device=dev) < 0.1).float()
mem.size = N
gamma, ns, nc = 0.99, 0.2, 0.5

def say(s):
    print(s, flush=True)

def torch_target(idx, eps):
    with torch.no_grad():
        c = mem.columns(idx)
        a = actor(c['next_obs'])
        a = torch.minimum(torch.maximum(a + torch.clamp(ns * eps, -nc, nc), low), high)
        q = torch.minimum(critics[0](c['next_obs'], a), critics[1](c['next_obs'], a))
        return c['reward'] + gamma * (q * (1.0 - c['absorbing']))

def block(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3          # microseconds per call

def compare(name, fns, calls=50, blocks=21):
    for fn in fns.values():                          # warm-up of every shape
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = {n: [] for n in fns}
    for _ in range(blocks):
        for n, fn in fns.items():                    # alternating
            t[n].append(block(fn, calls))
    for n, v in t.items():
        v.sort()
        say('%-28s %-8s median %9.1f us  min %9.1f  max %9.1f  (%d blocks of %d calls)' % (name, n, statistics.median(v), v[0], v[-1], blocks, calls))

if '--trace' in sys.argv:
    import copy
    for M in (16384, 256, 65536):
        idx, eps, y = mem.sample(M), torch.randn(M, k, device=dev), torch.empty(M, device=dev)
        for _ in range(200):
            mem.td_target(pol, cri, idx, gamma, eps=eps, noise_std=ns, noise_clip=nc, low=low, high=high, out=y)
            mem.q_values(cri[0], idx, out=y)
    actor_t, critics_t = copy.deepcopy(actor), [copy.deepcopy(c) for c in critics]
    pol_t, cri_t = MlpPolicy.from_module(actor_t), [QCritic.from_module(c, D) for c in critics_t]
    for _ in range(200):
        soft_update([pol_t] + cri_t, [pol] + cri, 5e-3)
    torch.cuda.synchronize()
    sys.exit(0)

for M in (16384, 256):
    idx = mem.sample(M)
    eps = torch.randn(M, k, device=dev)
    y = torch.empty(M, device=dev)
    fused = lambda: mem.td_target(pol, cri, idx, gamma, eps=eps, noise_std=ns, noise_clip=nc, low=low, high=high, out=y)
    ref = torch_target(idx, eps)
    fused()
    torch.cuda.synchronize()
    say('td_target %d rows: max |fused - torch| = %.3g' % (M, (y - ref).abs().max().item()))
    compare('td_target %d rows of %d' % (M, N), dict(fused=fused, torch=lambda: torch_target(idx, eps)))

# soft update: the three target networks of TD3
import copy
actor_t, critics_t = copy.deepcopy(actor), [copy.deepcopy(c) for c in critics]
pol_t = MlpPolicy.from_module(actor_t)
cri_t = [QCritic.from_module(c, D) for c in critics_t]
tau = 5e-3
def torch_soft():
    with torch.no_grad():
        for tn, on in ((actor_t, actor), (critics_t[0], critics[0]), (critics_t[1], critics[1])):
            for pt, po in zip(tn.parameters(), on.parameters()):
                pt.copy_(tau * po + (1 - tau) * pt)
def torch_foreach():
    with torch.no_grad():
        ts = [p for n in (actor_t, *critics_t) for p in n.parameters()]
        os_ = [p for n in (actor, *critics) for p in n.parameters()]
        torch._foreach_mul_(ts, 1 - tau)
        torch._foreach_add_(ts, os_, alpha=tau)
compare('soft_update 3 pairs', dict(fused=lambda: soft_update([pol_t] + cri_t, [pol] + cri, tau), torch=torch_soft, foreach=torch_foreach), calls=100)
