"""The optimiser step of an on-policy update, on the device: torch's default Adam (no amsgrad, no weight decay) over the
networks of the project's architecture and the log std of a policy, ONE launch for all of them, with the step count and the
running powers of the betas in device memory -- the host side of libatacom_optim.so (include/atacom_optim_hip.h states the
arithmetic).  It replaces, after the two gradient calls of fit.py,

    gc.flat.mul_(0.5); gp.to_module(actor, log_std); gc.to_module(critic); opt.step(); std.copy_(log_std.exp())

and, because nothing in it visits the host, the whole inner loop of an epoch -- gradients of the policy, gradients of the
critic, step, for every minibatch -- can be captured once and replayed as one graph: GraphedUpdate.

The parameters are updated where they lie: the tensors an MlpPolicy holds (from a module: the module's own storage), so the
rollout, evaluation and gradient kernels see each step at their next launch.  Every call is enqueued on the current stream of
the parameters' device; nothing synchronises or allocates after construction.  No numerics here, and no fall-back: a missing
library is an error.
"""
import math

import torch

from . import _lib_fit as _lf
from . import _lib_optim as _lo
from . import fit as _fit
from ._rows import columns, stream

_DTYPES = {torch.float32: _lo.F32, torch.float64: _lo.F64}
_KEYS = ('net', 'log_std', 'std', 'scale', 'lr')


def _finite(x):
    return isinstance(x, (int, float)) and math.isfinite(x)


class Adam:
    """Adam(groups, lr=3e-4, betas=(0.9, 0.999), eps=1e-8): `groups` is a list of one to four dicts
        net      an MlpPolicy whose six weight and bias tensors are updated in place
        log_std  None, or the [n_out] tensor of the policy's log std, updated with the network
        std      None, or the [n_out] tensor (the policy's tensors['std']) that each step refreshes with exp(log_std)
        scale    1.0; the group's gradient is multiplied by it (0.5 for the value loss of  policy + 0.5 value)
        lr       None = the optimiser's
    Every parameter must already be a contiguous CUDA tensor of one device in float32 or float64 (one dtype for all groups):
    anything else would reach the kernels as a copy, and the update would be lost.

    step(*grads) takes one fit.Gradients per group, in order, and makes one launch; steps() reads the step counts back (it
    synchronises); snapshot() / restore(s) cover the optimiser's state, the parameters, log_std and std."""

    def __init__(self, groups, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
        from .engine import MlpPolicy
        if not isinstance(groups, (list, tuple)) or not 1 <= len(groups) <= _lo.MAX_GROUPS:
            raise ValueError("groups must be a list of 1 .. %d dicts" % _lo.MAX_GROUPS)
        if not _finite(lr) or lr < 0:
            raise ValueError("lr must be >= 0 and finite, got %r" % (lr,))
        if not (isinstance(betas, (list, tuple)) and len(betas) == 2 and all(_finite(b) and 0.0 <= b < 1.0 for b in betas)):
            raise ValueError("betas must be two numbers in [0, 1), got %r" % (betas,))
        if not _finite(eps) or not eps > 0:
            raise ValueError("eps must be > 0 and finite, got %r" % (eps,))
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.groups = []
        first = None
        for k, g in enumerate(groups):
            if not isinstance(g, dict) or 'net' not in g or set(g) - set(_KEYS):
                raise ValueError("groups[%d] must be a dict with the key 'net' and any of %s" % (k, ', '.join(_KEYS[1:])))
            net, log_std, std = g['net'], g.get('log_std'), g.get('std')
            scale, glr = g.get('scale', 1.0), g.get('lr')
            glr = lr if glr is None else glr
            if not isinstance(net, MlpPolicy):
                raise ValueError("groups[%d]: net must be an MlpPolicy" % k)
            if not _finite(glr) or glr < 0:
                raise ValueError("groups[%d]: lr must be >= 0 and finite, got %r" % (k, glr))
            if not _finite(scale):
                raise ValueError("groups[%d]: scale must be finite, got %r" % (k, scale))
            if std is not None and log_std is None:
                raise ValueError("groups[%d]: std without log_std" % k)
            par = [net.tensors[name] for name in _lo.PARAMS]
            if not all(isinstance(t, torch.Tensor) for t in par) or par[0].dim() != 2 or par[4].dim() != 2:
                raise ValueError("groups[%d]: the weights and biases of the network must be tensors" % k)
            n_in, n_out = par[0].shape[1], par[4].shape[0]
            if not 1 <= n_in <= _lo.MAX_IN or not 1 <= n_out <= _lo.MAX_OUT:
                raise ValueError("groups[%d]: a %d -> %d network is outside n_in 1 .. %d, n_out 1 .. %d" % (
                    k, n_in, n_out, _lo.MAX_IN, _lo.MAX_OUT))
            shapes = ((64, n_in), (64,), (64, 64), (64,), (n_out, 64), (n_out,), (n_out,), (n_out,))
            named = list(zip(_lo.PARAMS + ('log_std', 'std'), par + [log_std, std], shapes))
            for name, t, shape in named:
                if t is None:
                    continue
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                    raise ValueError("groups[%d]: %s must be a tensor of shape %s (Linear(n_in, 64) - Linear(64, 64) - "
                                     "Linear(64, n_out))" % (k, name, shape))
                if t.dtype not in _DTYPES:
                    raise ValueError("groups[%d]: %s must be float32 or float64, got %s" % (k, name, t.dtype))
                first = t if first is None else first
                if t.dtype != first.dtype or t.device != first.device:
                    raise ValueError("groups[%d]: %s is %s on %s where the first parameter is %s on %s: one launch updates one "
                                     "dtype on one device" % (k, name, t.dtype, t.device, first.dtype, first.device))
                if not t.is_contiguous():
                    raise ValueError("groups[%d]: %s must be contiguous: the kernel would update a copy" % (k, name))
            self.groups.append(dict(net=net, n_in=n_in, n_out=n_out, scale=float(scale), lr=float(glr),
                                    params=[t.detach() for t in par],
                                    log_std=None if log_std is None else log_std.detach(),
                                    std=None if std is None else std.detach()))
        if first.device.type != 'cuda':                      # the last check that needs no device
            raise ValueError("the kernels of libatacom_optim.so run on a GPU; got parameters on %s: move the networks there "
                             "first (the update of a copy would be lost)" % first.device)
        self.dtype, self.device = first.dtype, first.device
        lib = _lo.load()
        a = _lo.new_args()
        a.device, a.dtype, a.n_groups = torch.cuda.current_device() if self.device.index is None else self.device.index, _DTYPES[self.dtype], len(self.groups)
        a.beta1, a.beta2, a.eps = self.betas[0], self.betas[1], self.eps
        es = first.element_size()
        for g, s in zip(self.groups, a.groups):
            has = g['log_std'] is not None
            size = lib.atacom_optim_state_size(a.dtype, g['n_in'], g['n_out'], int(has))
            if size == 0:
                _lo.check(_lo.E_INVALID)
            N = _lo.group_size(g['n_in'], g['n_out'], has)
            g['N'] = N
            g['state'] = torch.empty(size, dtype=torch.uint8, device=self.device)
            g['step'] = g['state'][:8].view(torch.int64)
            g['pows'] = g['state'][8:24].view(torch.float64)
            g['m'] = g['state'][_lo.HEAD:_lo.HEAD + N * es].view(self.dtype)
            g['v'] = g['state'][_lo.HEAD + N * es:].view(self.dtype)
            g['key'] = (g['n_in'], g['n_out'], _lf.PPO_CLIP if has else _lf.VALUE, self.dtype, self.device)
            s.n_in, s.n_out = g['n_in'], g['n_out']
            for name, t in zip(_lo.PARAMS, g['params']):
                setattr(s, name, t.data_ptr())
            s.log_std = None if g['log_std'] is None else g['log_std'].data_ptr()
            s.std = None if g['std'] is None else g['std'].data_ptr()
            s.state, s.lr, s.grad_scale = g['state'].data_ptr(), g['lr'], g['scale']
        self._args, self._lib = a, lib
        self.zero_state()

    def zero_state(self):
        """A fresh state for every group: step 0, zero moments (one launch)."""
        a = self._args
        for s in a.groups:
            s.grad = None                                    # init reads no gradient and accepts none
        a.stream = stream(a.device)
        _lo.check(self._lib.atacom_optim_adam_init(a))

    def step(self, *grads):
        """One Adam step of every group from its fit.Gradients, in the order of the groups: one launch."""
        if len(grads) != len(self.groups):
            raise ValueError("step takes one Gradients per group: %d, got %d" % (len(self.groups), len(grads)))
        a = self._args
        for k, (g, s, gr) in enumerate(zip(self.groups, a.groups, grads)):
            if not isinstance(gr, _fit.Gradients) or gr.key != g['key']:
                raise ValueError("grads[%d] must be the Gradients of a %s call for a %d -> %d network in %s on %s" % (
                    k, 'PPO' if g['log_std'] is not None else 'value', g['n_in'], g['n_out'], self.dtype, self.device))
            s.grad = gr.flat.data_ptr()
        a.stream = stream(a.device)
        _lo.check(self._lib.atacom_optim_adam_step(a))

    def steps(self):
        """The step count of every group, read back from the device (synchronises)."""
        return [int(g['step'].item()) for g in self.groups]

    def _tensors(self):
        for g in self.groups:
            yield g['state']
            for t in g['params']:
                yield t
            for t in (g['log_std'], g['std']):
                if t is not None:
                    yield t

    def snapshot(self):
        """Device clones of the optimiser's state, the parameters, log_std and std.  Not capturable: it allocates."""
        return [t.clone() for t in self._tensors()]

    def restore(self, s):
        """Put back what snapshot() returned, in place."""
        ts = list(self._tensors())
        if not isinstance(s, (list, tuple)) or len(s) != len(ts) or any(a.shape != b.shape or a.dtype != b.dtype for a, b in zip(s, ts)):
            raise ValueError("not a snapshot of this optimiser")
        for t, c in zip(ts, s):
            t.copy_(c)


class GraphedUpdate:
    """One PPO epoch -- for every minibatch: the policy's gradients, the critic's gradients, one Adam step -- captured ONCE in
    a HIP graph and replayed with one host call.

        upd = GraphedUpdate(layout, rec, adv, ret, logp_old, policy, critic, optimizer, minibatch=16384)
        for _ in range(epochs):
            upd.replay()                  # a fresh permutation of the rows, drawn on the device, then the graph

    `rec` (full or compact records of `layout`), `adv`, `ret` and `logp_old` are STATIC: the graph reads them where they lie,
    so the caller refills them in place each iteration (rollout_packed(out=), gae_from_records(out=), logp_old.copy_()), and
    replay() raises if one of them, or a parameter, has moved.  `optimizer` is an Adam of exactly two groups, the policy's and
    the critic's, in that order.  The rows are cut into slices perm[i : i + minibatch], the last possibly shorter, of a static
    int64 permutation `perm` of all T * B rows; replay(perm) copies a given permutation into it, replay() draws one with
    torch.randperm(out=).

    The graph is a linear chain on one stream (no forks).  `clip`, the learning rates, the betas, eps and the gradient scales
    are BAKED INTO THE GRAPH at capture: changing them afterwards needs a new GraphedUpdate.  The constructor warms up on a side stream
    (real updates) and undoes them completely with optimizer.restore(), so the parameters and the optimiser's state after
    construction are bit for bit those before it."""

    def __init__(self, layout, rec, adv, ret, logp_old, policy, critic, optimizer, minibatch, clip=0.2, warmup=2):
        if not isinstance(optimizer, Adam) or len(optimizer.groups) != 2 or optimizer.groups[0]['net'] is not policy or \
                optimizer.groups[1]['net'] is not critic:
            raise ValueError("optimizer must be an Adam of two groups: the policy's, then the critic's")
        cols = columns(layout, rec)
        n = 1
        for s in cols.shape[:-1]:
            n *= s
        if not 1 <= int(minibatch):
            raise ValueError("minibatch must be >= 1, got %r" % (minibatch,))
        self.layout, self.rec, self.adv, self.ret, self.logp_old = layout, rec, adv, ret, logp_old
        self.policy, self.critic, self.optimizer, self.clip = policy, critic, optimizer, float(clip)
        self.n_rows, self.minibatch = n, min(int(minibatch), n)
        dev = optimizer.device
        self.perm = torch.arange(n, dtype=torch.int64, device=dev)
        self._slices = [self.perm[i:i + self.minibatch] for i in range(0, n, self.minibatch)]
        self.gp = self.gc = None
        saved = optimizer.snapshot()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                        # outside the capture: lazy initialisation, and the two Gradients
            ends = self._slices[:1] + (self._slices[-1:] if len(self._slices) > 1 else [])
            for _ in range(max(1, int(warmup))):             # (at least once: the first slice is the largest workspace)
                self._body(ends)
        torch.cuda.current_stream(dev).wait_stream(side)
        optimizer.restore(saved)                             # the warm-up made real updates: undo them completely
        self._static = self._pointers()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._body(self._slices)
        optimizer.restore(saved)                             # (the capture itself does not run the kernels)

    def _body(self, slices):
        for idx in slices:
            self.gp = _fit.policy_gradient_from_records(self.layout, self.rec, self.adv, self.logp_old, self.policy, clip=self.clip,
                                                        idx=idx, out=self.gp)
            self.gc = _fit.value_gradient_from_records(self.layout, self.rec, self.ret, self.critic, idx=idx, out=self.gc)
            self.optimizer.step(self.gp, self.gc)

    def _pointers(self):
        ts = [self.rec, self.adv, self.ret, self.logp_old, self.perm]
        for net in (self.policy, self.critic):
            ts += [v for v in net.tensors.values() if isinstance(v, torch.Tensor)]
        return [t.data_ptr() for t in ts]

    def replay(self, perm=None):
        """Replay the epoch over `perm` (int64 [T * B], copied into the static buffer; the caller answers for its being a
        list of row numbers in range) or over a fresh torch.randperm drawn into that buffer."""
        if self._pointers() != self._static:
            raise RuntimeError("a static tensor of this GraphedUpdate (records, adv, ret, logp_old, perm or a parameter) has "
                               "moved since the capture: refill them in place")
        if perm is None:
            torch.randperm(self.n_rows, out=self.perm)
        else:
            if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int64 or tuple(perm.shape) != (self.n_rows,):
                raise ValueError("perm must be an int64 tensor of %d row numbers" % self.n_rows)
            self.perm.copy_(perm)
        self.graph.replay()
