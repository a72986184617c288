"""The optimiser step of an off-policy update (DDPG, TD3, SAC) on the device -- the host side of libatacom_offstep.so
(include/atacom_offstep_hip.h states the arithmetic): torch's default Adam over plain networks AND two-branch critics, with the
soft update of each group's target network in the same launch, from the value the step has just written.  After the gradient
calls of offgrad.py it replaces

    gq.to_module(critic); torch_adam.step(); device_adam.step(ga); soft_update(targets, onlines, tau)

with one launch, and because nothing in it visits the host a whole TD3 or DDPG fit -- TD target, critic gradients, step, actor
gradient, step, targets -- can be captured once and replayed as one graph: GraphedFit.

The parameters and the targets are updated where they lie: the tensors an MlpPolicy or a QCritic holds (from a module: the
module's own storage).  Every call is enqueued on the current stream of the parameters' device; nothing synchronises or
allocates after construction.  No numerics here, and no fall-back: a missing library is an error.
"""
import math

import torch

from . import _lib_fit as _lf
from . import _lib_offstep as _ls
from . import fit as _fit
from ._rows import DTYPES, bound, stream

_KEYS = ('net', 'target', 'lr', 'scale')


def _finite(x):
    return isinstance(x, (int, float)) and math.isfinite(x)


def _params(net):
    """The six tensors of an MlpPolicy or the seven of a QCritic, in the order of a group."""
    from .offpolicy import QCritic
    return [net.tensors[name] for name in (_ls.PARAMS if isinstance(net, QCritic) else _ls.PARAMS[:6])]


class TrackedAdam:
    """TrackedAdam(groups, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, tau=5e-3): `groups` is a list of one to four dicts
        net      an MlpPolicy (its six weight and bias tensors) or a QCritic (those and W2a), updated in place
        target   None, or an object of the same kind and shapes: after each step  target = tau * net + (1 - tau) * target
        lr       None = the optimiser's
        scale    1.0; the group's gradient is multiplied by it
    Every tensor must already be a contiguous CUDA tensor of one device in float32 or float64 (one dtype for all groups):
    anything else would reach the kernel as a copy, and the update would be lost.

    step(*grads) takes one gradient per group, in order -- a fit.Gradients of the value head's key for an MlpPolicy (what
    offgrad.actor_gradient returns), a QGradients for a QCritic, or None: the group is not stepped and only its target follows --
    and makes one launch.  step(..., only=(1, 2)) leaves every other group out of the launch altogether: neither stepped nor
    followed.  steps() reads the step counts back (it synchronises); snapshot() / restore(s) cover the optimiser's state, the
    parameters and the targets."""

    def __init__(self, groups, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, tau=5e-3):
        from .engine import MlpPolicy
        from .offpolicy import QCritic
        if not isinstance(groups, (list, tuple)) or not 1 <= len(groups) <= _ls.MAX_GROUPS:
            raise ValueError("groups must be a list of 1 .. %d dicts" % _ls.MAX_GROUPS)
        if not _finite(lr) or lr < 0:
            raise ValueError("lr must be >= 0 and finite, got %r" % (lr,))
        if not (isinstance(betas, (list, tuple)) and len(betas) == 2 and all(_finite(b) and 0.0 <= b < 1.0 for b in betas)):
            raise ValueError("betas must be two numbers in [0, 1), got %r" % (betas,))
        if not _finite(eps) or not eps > 0:
            raise ValueError("eps must be > 0 and finite, got %r" % (eps,))
        if not _finite(tau) or not 0.0 <= tau <= 1.0:
            raise ValueError("tau must be in [0, 1], got %r" % (tau,))
        self.betas, self.eps, self.tau = (float(betas[0]), float(betas[1])), float(eps), float(tau)
        self.groups = []
        first = None
        for k, g in enumerate(groups):
            if not isinstance(g, dict) or 'net' not in g or set(g) - set(_KEYS):
                raise ValueError("groups[%d] must be a dict with the key 'net' and any of %s" % (k, ', '.join(_KEYS[1:])))
            net, target, scale, glr = g['net'], g.get('target'), g.get('scale', 1.0), g.get('lr')
            glr = lr if glr is None else glr
            if not isinstance(net, (MlpPolicy, QCritic)):
                raise ValueError("groups[%d]: net must be an MlpPolicy or a QCritic" % k)
            if target is not None and (type(target) is not type(net) or target is net):
                raise ValueError("groups[%d]: target must be another %s, or None" % (k, type(net).__name__))
            if not _finite(glr) or glr < 0:
                raise ValueError("groups[%d]: lr must be >= 0 and finite, got %r" % (k, glr))
            if not _finite(scale):
                raise ValueError("groups[%d]: scale must be finite, got %r" % (k, scale))
            par = _params(net)
            if not all(isinstance(t, torch.Tensor) for t in par) or par[0].dim() != 2 or par[4].dim() != 2 or \
                    (len(par) == 7 and par[6].dim() != 2):
                raise ValueError("groups[%d]: the weights and biases of the network must be tensors" % k)
            n_in, n_out, n_act = par[0].shape[1], par[4].shape[0], (par[6].shape[1] if len(par) == 7 else 0)
            if not 1 <= n_in <= _ls.MAX_IN or not 1 <= n_out <= _ls.MAX_OUT or not (len(par) == 6 or 1 <= n_act <= _ls.MAX_ACT):
                raise ValueError("groups[%d]: a %d -> %d network with %d action columns is outside n_in 1 .. %d, n_out 1 .. %d, "
                                 "n_act 1 .. %d" % (k, n_in, n_out, n_act, _ls.MAX_IN, _ls.MAX_OUT, _ls.MAX_ACT))
            shapes = ((64, n_in), (64,), (64, 64), (64,), (n_out, 64), (n_out,), (64, n_act))[:len(par)]
            tpar = None
            if target is not None:
                tpar = _params(target)
                if not all(isinstance(t, torch.Tensor) for t in tpar):
                    raise ValueError("groups[%d]: the weights and biases of the target must be tensors" % k)
            named = list(zip(_ls.PARAMS, par, shapes)) + \
                ([] if tpar is None else [('target ' + name, t, s) for name, t, s in zip(_ls.PARAMS, tpar, shapes)])
            for name, t, shape in named:
                if tuple(t.shape) != shape:
                    raise ValueError("groups[%d]: %s must be a tensor of shape %s (Linear(n_in, 64) - Linear(64, 64) - "
                                     "Linear(64, n_out), W2a [64, n_act])" % (k, name, shape))
                if t.dtype not in DTYPES:
                    raise ValueError("groups[%d]: %s must be float32 or float64, got %s" % (k, name, t.dtype))
                first = t if first is None else first
                if t.dtype != first.dtype or t.device != first.device:
                    raise ValueError("groups[%d]: %s is %s on %s where the first parameter is %s on %s: one launch updates one "
                                     "dtype on one device" % (k, name, t.dtype, t.device, first.dtype, first.device))
                if not t.is_contiguous():
                    raise ValueError("groups[%d]: %s must be contiguous: the kernel would update a copy" % (k, name))
            self.groups.append(dict(net=net, target=target, n_in=n_in, n_out=n_out, n_act=n_act, critic=len(par) == 7,
                                    scale=float(scale), lr=float(glr), params=[t.detach() for t in par],
                                    targets=None if tpar is None else [t.detach() for t in tpar]))
        if first.device.type != 'cuda':                      # the last check that needs no device
            raise ValueError("the kernels of libatacom_offstep.so run on a GPU; got parameters on %s: move the networks there "
                             "first (the update of a copy would be lost)" % first.device)
        self.dtype, self.device = first.dtype, first.device
        lib = _ls.load()
        a = _ls.new_args()
        a.device = torch.cuda.current_device() if self.device.index is None else self.device.index
        a.dtype, a.n_groups = DTYPES[self.dtype], len(self.groups)
        a.beta1, a.beta2, a.eps, a.tau = self.betas[0], self.betas[1], self.eps, self.tau
        es = first.element_size()
        for g, s in zip(self.groups, a.groups):
            size = lib.atacom_offstep_state_size(a.dtype, g['n_in'], g['n_out'], g['n_act'])
            if size == 0:
                _ls.check(_ls.E_INVALID)
            N = _ls.group_size(g['n_in'], g['n_out'], g['n_act'])
            g['N'] = N
            g['state'] = torch.empty(size, dtype=torch.uint8, device=self.device)
            g['step'] = g['state'][:8].view(torch.int64)
            g['pows'] = g['state'][8:24].view(torch.float64)
            g['m'] = g['state'][_ls.HEAD:_ls.HEAD + N * es].view(self.dtype)
            g['v'] = g['state'][_ls.HEAD + N * es:].view(self.dtype)
            # what a gradient of this group is: the key of a QGradients, or of a fit.Gradients of the value head
            g['key'] = (g['n_in'], g['n_act'], self.dtype, self.device) if g['critic'] else \
                (g['n_in'], g['n_out'], _lf.VALUE, self.dtype, self.device)
            s.n_in, s.n_out, s.n_act = g['n_in'], g['n_out'], g['n_act']
            for j, (name, t) in enumerate(zip(_ls.PARAMS, g['params'])):
                setattr(s, name, t.data_ptr())
                if g['targets'] is not None:
                    s.target[j] = g['targets'][j].data_ptr()
            s.state, s.lr, s.grad_scale = g['state'].data_ptr(), g['lr'], g['scale']
        self._args, self._lib, self._subsets = a, lib, {}
        self.zero_state()

    def zero_state(self):
        """A fresh state for every group: step 0, zero moments (one launch)."""
        a = self._args
        for s in a.groups:
            s.grad = None                                    # init reads no gradient
        a.stream = stream(a.device)
        _ls.check(self._lib.atacom_offstep_adam_init(a))

    def _subset(self, only):
        """The argument struct of a launch over the groups `only` names: the groups' structs copied once, in their order."""
        n = len(self.groups)
        if not isinstance(only, (list, tuple)) or not only or any(type(i) is not int or not 0 <= i < n for i in only) or \
                list(only) != sorted(set(only)):
            raise ValueError("only must name groups 0 .. %d, each once and in order, got %r" % (n - 1, only))
        only = tuple(only)
        if only not in self._subsets:
            a, full = _ls.new_args(), self._args
            a.device, a.dtype, a.n_groups = full.device, full.dtype, len(only)
            a.beta1, a.beta2, a.eps, a.tau = full.beta1, full.beta2, full.eps, full.tau
            for j, i in enumerate(only):
                a.groups[j] = full.groups[i]
            self._subsets[only] = a
        return self._subsets[only]

    def step(self, *grads, only=None):
        """One step of every group from its gradient, in the order of the groups, and of every target after it: one launch.
        A gradient of None leaves its group as it is and only lets the target follow.  `only`: the numbers of the groups
        that take part; the others are neither stepped nor followed (their entry of `grads` is not looked at)."""
        from .offgrad import QGradients
        if len(grads) != len(self.groups):
            raise ValueError("step takes one gradient (or None) per group: %d, got %d" % (len(self.groups), len(grads)))
        chosen = tuple(range(len(self.groups))) if only is None else tuple(only)
        a = self._args if only is None else self._subset(only)
        for s, k in zip(a.groups, chosen):
            g, gr = self.groups[k], grads[k]
            if gr is None:
                s.grad = None
                continue
            if not isinstance(gr, QGradients if g['critic'] else _fit.Gradients) or gr.key != g['key'] or gr.flat.numel() != g['N']:
                raise ValueError("grads[%d] must be None or the %s of a %d -> %d network%s in %s on %s" % (
                    k, 'QGradients' if g['critic'] else 'Gradients (value head)', g['n_in'], g['n_out'],
                    ' with %d action columns' % g['n_act'] if g['critic'] else '', self.dtype, self.device))
            s.grad = gr.flat.data_ptr()
        a.stream = stream(a.device)
        _ls.check(self._lib.atacom_offstep_adam_step(a))

    def steps(self):
        """The step count of every group, read back from the device (synchronises)."""
        return [int(g['step'].item()) for g in self.groups]

    def _tensors(self):
        for g in self.groups:
            yield g['state']
            for t in g['params']:
                yield t
            for t in g['targets'] or ():
                yield t

    def snapshot(self):
        """Device clones of the optimiser's state, the parameters and the targets.  Not capturable: it allocates."""
        return [t.clone() for t in self._tensors()]

    def restore(self, s):
        """Put back what snapshot() returned, in place."""
        ts = list(self._tensors())
        if not isinstance(s, (list, tuple)) or len(s) != len(ts) or any(a.shape != b.shape or a.dtype != b.dtype for a, b in zip(s, ts)):
            raise ValueError("not a snapshot of this optimiser")
        for t, c in zip(ts, s):
            t.copy_(c)


class GraphedFit:
    """`policy_delay` consecutive TD3 fits -- or one DDPG fit: one critic, policy_delay=1, no smoothing noise -- captured ONCE in
    a HIP graph and replayed with one host call.

        opt = TrackedAdam([dict(net=actor, target=actor_t, lr=1e-4), dict(net=q1, target=q1_t), dict(net=q2, target=q2_t)])
        fit = GraphedFit(mem, actor, actor_t, (q1, q2), (q1_t, q2_t), opt, minibatch=256, gamma=0.99, noise_std=0.2, noise_clip=0.5,
                         low=low, high=high)
        fit.replay()                      # fresh row numbers and noise, drawn on the device, then the graph

    Fit j of the graph reads idx[j] and eps[j] and is MushroomRL's DDPG.fit in its order: the TD target from the target networks
    (mem.td_target into a static y), the critics' gradients and step, on fit 0 -- where fit_count % policy_delay == 0: a graph
    starts at a multiple of policy_delay -- the actor's gradient THROUGH THE UPDATED first critic and its step, then the soft
    update of all the targets.  The launches of the fit whose actor steps are
        td_target, critic_gradient, step(critics, their targets follow; the actor left out), actor_gradient, step(actor, its
        target follows)
    and of every other fit
        td_target, critic_gradient, step(critics step; all targets follow)
    (DESIGN.md section 7i says why this split equals the reference's order).

    `mem.storage`, `idx` [policy_delay, M] (int64) and `eps` [policy_delay, M, k] are STATIC: the graph reads them where they
    lie, and replay() raises if one of them, or a parameter or a target, has moved.  replay() draws idx with torch.randint(0,
    mem.size, out=) -- mem.size is a host number that grows, so it is read outside the graph -- and eps with torch.randn(out=);
    replay(idx=, eps=) copies given ones in.  eager() runs the same body without the graph.

    The graph is a linear chain on one stream (no forks).  The learning rates, the betas, eps, tau, gamma and the noise
    parameters are BAKED INTO THE GRAPH at capture: changing them afterwards needs a new GraphedFit.  The constructor warms up on
    a side stream (real updates) and undoes them completely with optimizer.restore(), so the parameters, the targets and the
    optimiser's state after construction are bit for bit those before it."""

    def __init__(self, mem, actor, actor_target, critics, critic_targets, optimizer, minibatch, gamma, policy_delay=2, noise_std=0.0,
                 noise_clip=0.0, low=None, high=None, warmup=2):
        from .offpolicy import QCritic, ReplayMemory
        critics = (critics,) if isinstance(critics, QCritic) else tuple(critics)
        critic_targets = (critic_targets,) if isinstance(critic_targets, QCritic) else tuple(critic_targets)
        if len(critics) not in (1, 2) or len(critic_targets) != len(critics):
            raise ValueError("critics and critic_targets are one QCritic each or a pair each")
        nets, targets = (actor,) + critics, (actor_target,) + critic_targets
        if not isinstance(optimizer, TrackedAdam) or len(optimizer.groups) != len(nets) or \
                any(g['net'] is not n or g['target'] is not t for g, n, t in zip(optimizer.groups, nets, targets)):
            raise ValueError("optimizer must be a TrackedAdam of the groups [actor, critic_1 (, critic_2)] with their targets attached")
        if not isinstance(mem, ReplayMemory):
            raise ValueError("mem must be a ReplayMemory")
        if not 1 <= int(minibatch) or not 1 <= int(policy_delay):
            raise ValueError("minibatch and policy_delay must be >= 1, got %r and %r" % (minibatch, policy_delay))
        if (low is None) != (high is None):
            raise ValueError("low and high are given together or not at all")
        dev, dtype = optimizer.device, optimizer.dtype
        if mem.storage.device != dev or mem.storage.dtype != dtype:
            raise ValueError("the memory's storage is %s on %s where the networks are %s on %s" % (
                mem.storage.dtype, mem.storage.device, dtype, dev))
        self.mem, self.actor, self.actor_target, self.critics, self.critic_targets = mem, actor, actor_target, critics, critic_targets
        self.optimizer, self.minibatch, self.policy_delay = optimizer, int(minibatch), int(policy_delay)
        self.gamma, self.noise_std, self.noise_clip = float(gamma), float(noise_std), float(noise_clip)
        M, k = self.minibatch, mem.k
        self.low = None if low is None else bound(low, k, mem.storage, 'low')
        self.high = None if high is None else bound(high, k, mem.storage, 'high')
        self.idx = torch.zeros((self.policy_delay, M), dtype=torch.int64, device=dev)
        self.eps = torch.zeros((self.policy_delay, M, k), dtype=dtype, device=dev)
        self.y = torch.empty(M, dtype=dtype, device=dev)
        self.gq = self.ga = None
        self._critic_groups = tuple(range(1, len(nets)))
        saved = optimizer.snapshot()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                        # outside the capture: lazy initialisation, and the gradients' buffers
            for _ in range(max(1, int(warmup))):
                self._body()
        torch.cuda.current_stream(dev).wait_stream(side)
        optimizer.restore(saved)                             # the warm-up made real updates: undo them completely
        self._static = self._pointers()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._body()
        optimizer.restore(saved)                             # (the capture itself does not run the kernels)

    def _body(self):
        opt, none = self.optimizer, (None,) * len(self.critics)
        for j in range(self.policy_delay):
            idx = self.idx[j]
            self.mem.td_target(self.actor_target, self.critic_targets, idx, self.gamma, eps=self.eps[j] if self.noise_std > 0.0 else None,
                               noise_std=self.noise_std, noise_clip=self.noise_clip, low=self.low, high=self.high, out=self.y)
            self.gq = self.mem.critic_gradient(self.critics, idx, self.y, out=self.gq)
            if j == 0:
                opt.step(None, *self.gq, only=self._critic_groups)
                self.ga = self.mem.actor_gradient(self.actor, self.critics[0], idx, out=self.ga)
                opt.step(self.ga, *none, only=(0,))
            else:
                opt.step(None, *self.gq)

    def _pointers(self):
        ts = [self.mem.storage, self.idx, self.eps, self.y] + [t for t in (self.low, self.high) if t is not None]
        for net in (self.actor, self.actor_target) + self.critics + self.critic_targets:
            ts += [v for v in net.tensors.values() if isinstance(v, torch.Tensor)]
        return [t.data_ptr() for t in ts]

    def _fill(self, idx, eps):
        if self._pointers() != self._static:
            raise RuntimeError("a static tensor of this GraphedFit (the memory's storage, idx, eps, a bound, a parameter or a "
                               "target) has moved since the capture: refill them in place")
        if idx is None:
            if self.mem.size < 1:
                raise ValueError("the memory is empty")
            torch.randint(0, self.mem.size, tuple(self.idx.shape), out=self.idx)
        else:
            if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.shape != self.idx.shape:
                raise ValueError("idx must be an int64 tensor of shape %s" % (tuple(self.idx.shape),))
            self.idx.copy_(idx)
        if eps is None:
            torch.randn(tuple(self.eps.shape), out=self.eps)
        else:
            if not isinstance(eps, torch.Tensor) or eps.shape != self.eps.shape:
                raise ValueError("eps must be a tensor of shape %s" % (tuple(self.eps.shape),))
            self.eps.copy_(eps)

    def replay(self, idx=None, eps=None):
        """Replay the `policy_delay` fits over `idx` and `eps` (copied into the static buffers; the caller answers for the row
        numbers being in range) or over fresh ones drawn into those buffers."""
        self._fill(idx, eps)
        self.graph.replay()

    def eager(self, idx=None, eps=None):
        """The same fits as replay(), call by call on the current stream."""
        self._fill(idx, eps)
        self._body()

    @property
    def critic_losses(self):
        """The critics' losses of the last fit of the graph: device scalars."""
        return [g.loss for g in self.gq]

    @property
    def actor_loss(self):
        """The actor's loss of fit 0 of the graph: a device scalar."""
        return self.ga.loss
