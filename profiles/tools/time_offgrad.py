"""python profiles/tools/time_offgrad.py [--trace]

critic_gradient (a pair) and actor_gradient (float32, TD3, iiwa-sized networks) against the torch autograd loop body they
replace -- the gather, the forward and backward passes and zero_grad, the optimiser step left out on both sides: blocks of
calls between device events, the two versions alternating, medians and spread, at 256 rows and at 16384 rows gathered from 983040.
With --trace: 200 calls of each at 16384 and 256 rows and nothing else, the workload of
rocprofv3 --kernel-trace --stats -- python profiles/tools/time_offgrad.py --trace."""
import os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))
from rl_on_manifold_amd import MlpPolicy, QCritic, ReplayMemory
from td3_air_hockey import Actor, Critic

dev = torch.device('cuda:0')
torch.manual_seed(0)
D, k, N = 18, 5, 983040
scaling = torch.ones(k, device=dev)
actor, critics = Actor(D, k, scaling).to(dev), [Critic(D, k, scaling).to(dev) for _ in range(2)]
pol = MlpPolicy.from_td3(actor, 0.01, low=-1.0, high=1.0)
pol.tensors.update(act_scale=scaling, act_low=-scaling, act_high=scaling.clone(), std=torch.full((k,), 0.1, device=dev))
cri = [QCritic.from_module(c, D) for c in critics]
for c in cri:
    c.tensors['act_scale'] = scaling
mem = ReplayMemory(N, D, k, device=dev)
mem.storage.normal_()
mem.size = N
critic_params = [p for c in critics for p in c.parameters()]
actor_params = list(actor.parameters())

def say(s):
    print(s, flush=True)

def torch_critics(idx, tgt):
    c = mem.columns(idx)
    lq = sum(((cr(c['obs'], c['action']) - tgt) ** 2).mean() for cr in critics)
    for p in critic_params:
        p.grad = None
    lq.backward()

def torch_actor(idx):
    c = mem.columns(idx)
    la = -critics[0](c['obs'], actor(c['obs'])).mean()
    for p in actor_params:
        p.grad = None
    la.backward()

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
    med = {}
    for n, v in t.items():
        v.sort()
        med[n] = statistics.median(v)
        say('%-32s %-8s median %9.1f us  min %9.1f  max %9.1f  (%d blocks of %d calls)' % (name, n, med[n], v[0], v[-1], blocks, calls))
    say('%-32s torch / fused = %.2f' % (name, med['torch'] / med['fused']))

if '--trace' in sys.argv:
    for M in (16384, 256):
        idx, tgt = mem.sample(M), torch.randn(M, device=dev)
        gs, ga = mem.critic_gradient(cri, idx, tgt), mem.actor_gradient(pol, cri[0], idx)
        for _ in range(200):
            mem.critic_gradient(cri, idx, tgt, out=gs)
            mem.actor_gradient(pol, cri[0], idx, out=ga)
    torch.cuda.synchronize()
    sys.exit(0)

for M in (16384, 256):
    idx, tgt = mem.sample(M), torch.randn(M, device=dev)
    gs, ga = mem.critic_gradient(cri, idx, tgt), mem.actor_gradient(pol, cri[0], idx)
    torch_critics(idx, tgt)
    ref = torch.cat([p.grad.reshape(-1) for c in critics[:1] for p in (c._h1.weight, c._h1.bias, c._h2_s.weight, c._h2_s.bias, c._h3.weight,
                                                                       c._h3.bias, c._h2_a.weight)])
    say('critic_gradient %d rows: max |fused - torch| = %.3g' % (M, (gs[0].flat - ref).abs().max().item()))
    torch_actor(idx)
    ref = torch.cat([p.grad.reshape(-1) for p in actor_params])
    say('actor_gradient %d rows: max |fused - torch| = %.3g' % (M, (ga.flat - ref).abs().max().item()))
    compare('critic_gradient (pair) %d rows' % M, dict(fused=lambda: mem.critic_gradient(cri, idx, tgt, out=gs),
                                                       torch=lambda: torch_critics(idx, tgt)))
    compare('actor_gradient %d rows' % M, dict(fused=lambda: mem.actor_gradient(pol, cri[0], idx, out=ga), torch=lambda: torch_actor(idx)))
