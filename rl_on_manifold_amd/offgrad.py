"""The backward half of an off-policy update (DDPG, TD3) on the device -- the host side of libatacom_offgrad.so
(include/atacom_offgrad_hip.h states the arithmetic): the gradient of the critics' mean-squared TD error and the deterministic
policy gradient of the actor, each one launch over a minibatch gathered through row numbers from a replay memory in place (plus
a small launch that adds the workgroups' partial sums).  They replace, in a learner's inner loop,

    ((critic_j(obs[idx], action[idx]) - y) ** 2).mean().backward()                # j = 1, 2
    (-critic_1(obs[idx], actor(obs[idx])).mean()).backward()                      # the actor's step; the critic is only read

-- the gathered copies, three forward and three backward passes of autograd.  The objects are those of offpolicy.py (QCritic) and
engine.py (MlpPolicy), used where their tensors lie: networks made once with from_module see the optimiser's in-place steps.
QGradients.to_module() hands the critic's gradient to torch.optim.Adam; the actor's gradient is a fit.Gradients with the value
head's key, which the device Adam of optim.py accepts for a group without log_std.

Every call is enqueued on the current stream of the tensors' device and nothing synchronises.  With `out=` a call allocates
nothing and can be captured in a graph.  No numerics here, and no fall-back: a missing library is an error.
"""
import torch

from . import _lib_fit as _lf
from . import _lib_offgrad as _lg
from .evaluate import _check_rows
from .fit import Gradients
from .offpolicy import QCritic, _idx, _one_launch, _rows_out
from .returns import _overlap, _stream

_DTYPES = {torch.float32: _lg.F32, torch.float64: _lg.F64}
_KINDS = {'ddpg': _lg.DDPG, 'td3': _lg.TD3}
_CRITIC_KEYS = ('W1', 'b1', 'W2', 'b2', 'W2a', 'W3', 'b3', 'obs_shift', 'obs_scale', 'act_scale')
PARAMS = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'W2a')          # the order of QGradients.flat: that of _lib_offpolicy.PARAMS


class QGradients:
    """What critic_gradient writes for one critic: `flat`, one buffer in the order dW1 [64, n1], db1, dW2, db2, dW3 [1, 64], db3,
    dW2a [64, k], the views W1, b1, W2, b2, W3, b3, W2a into it, `stats` [4] = loss, 0, 0, 0 and the `workspace` of the call (a
    pair shares one: the second's is a view of the first's).  Passed back as `out=`, all of it is reused."""

    def __init__(self, n1, n_act, dtype, device, workspace, key):
        self.n1, self.n_act, self.key = n1, n_act, key
        self.flat = torch.empty(_lg.grad_size(n1, 1, n_act), dtype=dtype, device=device)
        self.stats = torch.empty(_lg.STATS, dtype=dtype, device=device)
        self.workspace = workspace
        o = 0
        for name, shape in (('W1', (64, n1)), ('b1', (64,)), ('W2', (64, 64)), ('b2', (64,)), ('W3', (1, 64)), ('b3', (1,)),
                            ('W2a', (64, n_act))):
            n = 1
            for s in shape:
                n *= s
            setattr(self, name, self.flat[o:o + n].view(shape))
            o += n

    @property
    def loss(self):
        return self.stats[0]

    def to_module(self, net):
        """Make the views the .grad of net._h1, _h2_s, _h3 (weights and biases) and _h2_a (weight): after it
        torch.optim.Adam.step() works unchanged.  The parameters then share the buffer: the next call with out=self overwrites
        their .grad in place."""
        for par, g in ((net._h1.weight, self.W1), (net._h1.bias, self.b1), (net._h2_s.weight, self.W2), (net._h2_s.bias, self.b2),
                       (net._h3.weight, self.W3), (net._h3.bias, self.b3), (net._h2_a.weight, self.W2a)):
            if tuple(par.shape) != tuple(g.shape) or par.dtype != g.dtype or par.device != g.device:
                raise ValueError("a parameter is %s %s on %s where its gradient is %s %s on %s" % (
                    tuple(par.shape), par.dtype, par.device, tuple(g.shape), g.dtype, g.device))
            par.grad = g
        return self


def _critic_struct(critic, device, dtype):
    """The atacom_offgrad_critic of a QCritic: its own ctypes struct, filled from QCritic.tensors like QCritic.as_struct_on (tensors
    already on the device in the dtype are used as they are; the copies live as long as the critic or until the next call)."""
    device = torch.device(device)
    dev = {k: (None if v is None else torch.as_tensor(v).detach().to(device=device, dtype=dtype).contiguous())
           for k, v in critic.tensors.items()}
    critic._keep_offgrad = dev
    D, k = critic.n_obs, critic.n_act
    n1 = D + k if critic.kind == 'td3' else D
    for name, shape in (('W1', (64, n1)), ('b1', (64,)), ('W2', (64, 64)), ('b2', (64,)), ('W2a', (64, k)), ('W3', (1, 64)),
                        ('b3', (1,)), ('obs_shift', (D,)), ('obs_scale', (D,)), ('act_scale', (k,))):
        if dev[name] is not None and tuple(dev[name].shape) != shape:
            raise ValueError("%s has the shape %s where the critic needs %s" % (name, tuple(dev[name].shape), shape))
    c = _lg.Critic()
    c.kind, c.n_obs, c.n_act, c.activation = _KINDS[critic.kind], D, k, critic.activation
    for name in _CRITIC_KEYS:
        setattr(c, name, None if dev[name] is None else dev[name].data_ptr())
    return c, n1


def _sizes(critic):
    D, k = critic.n_obs, critic.n_act
    n1 = D + k if critic.kind == 'td3' else D
    if not 1 <= D <= _lg.MAX_IN or not 1 <= k <= _lg.MAX_ACT:
        raise ValueError("a critic of %d observation and %d action elements is outside 1 .. %d and 1 .. %d" % (D, k, _lg.MAX_IN, _lg.MAX_ACT))
    if n1 > _lg.MAX_IN:
        raise ValueError("n1 = %d first-layer inputs exceed %d" % (n1, _lg.MAX_IN))
    return D, k, n1


def _checked_blocks(n_blocks):
    if not isinstance(n_blocks, int) or not 0 <= n_blocks <= _lg.MAX_BLOCKS:
        raise ValueError("n_blocks must be 0 (the library chooses) or 1 .. %d" % _lg.MAX_BLOCKS)
    return n_blocks


def _obs_checks(obs, what='obs'):
    if not isinstance(obs, torch.Tensor) or obs.dim() < 1:
        raise ValueError("%s must be a tensor [..., n]" % what)
    if obs.dtype not in _DTYPES:
        raise ValueError("%s must be float32 or float64, got %s" % (what, obs.dtype))
    lead = tuple(obs.shape[:-1])
    if any(n == 0 for n in lead) or not lead:
        raise ValueError("%s holds no rows: %s" % (what, tuple(obs.shape)))
    return lead


def _needs_gpu(x):
    if x.device.type != 'cuda':                            # the last check that needs no device
        raise ValueError("the kernels of libatacom_offgrad.so run on a GPU; got tensors on %s" % x.device)


def critic_gradient(critics, obs, action, target, *, idx=None, out=None, n_blocks=0):
    """The gradient of  ((Q_j(obs, action) - target) ** 2).mean()  for one QCritic or a pair, over the rows of obs [..., D] and
    action [..., k] (strided views with contiguous rows, sharing their leading dimensions: the columns of a replay memory, read in
    place) -- or, with `idx` (int64 [M], flat numbers of those rows, repeats allowed, not guarded against the range), over the
    rows it names -- with respect to W1, b1, W2, b2, W3, b3 and W2a.  target [M] belongs to row r of the CALL, not to row
    idx[r] (the convention of td_target's eps).  -> QGradients, or a pair of them for a pair; `out`: the result of an earlier
    call of the same kind."""
    single = isinstance(critics, QCritic)
    critics = (critics,) if single else (tuple(critics) if isinstance(critics, (list, tuple)) else ())
    if len(critics) not in (1, 2) or not all(isinstance(c, QCritic) for c in critics):
        raise ValueError("critics must be one QCritic or a pair of them")
    c0 = critics[0]
    if any((c.kind, c.n_obs, c.n_act) != (c0.kind, c0.n_obs, c0.n_act) for c in critics):
        raise ValueError("the two critics differ in kind, observation or action size")
    D, k, n1 = _sizes(c0)
    lead = _obs_checks(obs)
    ts = [_check_rows(obs, 'obs', lead, D, obs), _check_rows(action, 'action', lead, k, obs)]
    offs, n_outer, n_inner, strides = _one_launch(ts, ('obs', 'action'), lead)
    idx = _idx(idx, obs)
    M = idx.numel() if idx is not None else n_outer * n_inner
    if not isinstance(target, torch.Tensor) or tuple(target.shape) != (M,):
        raise ValueError("target must be a tensor of shape (%d,): one value per row of the call" % M)
    if target.dtype != obs.dtype or target.device != obs.device:
        raise ValueError("target must be a %s tensor on %s" % (obs.dtype, obs.device))
    n_blocks = _checked_blocks(n_blocks)
    _needs_gpu(obs)
    lib = _lg.load()
    need = lib.atacom_offgrad_workspace_size(_DTYPES[obs.dtype], len(critics), n1, 1, k, M, n_blocks)
    if need == 0:
        _lg.check(_lg.E_INVALID)
    key = (n1, k, obs.dtype, obs.device)
    if out is None:
        ws = torch.empty(need, dtype=torch.uint8, device=obs.device)
        outs = tuple(QGradients(n1, k, obs.dtype, obs.device, ws, key) for _ in critics)
    else:
        outs = (out,) if isinstance(out, QGradients) else tuple(out)
        if len(outs) != len(critics) or not all(isinstance(o, QGradients) and o.key == key for o in outs):
            raise ValueError("out must be the QGradients (one per critic) of a call for critics of %d first-layer inputs and %d "
                             "action elements in %s on %s" % (n1, k, obs.dtype, obs.device))
        if outs[0].workspace.numel() < need:
            raise ValueError("out was made for fewer workgroups: its workspace holds %d bytes where this call needs %d" % (
                outs[0].workspace.numel(), need))
    ins = list(zip(ts, ('obs', 'action'))) + [(target, 'target')] + ([(idx, 'idx')] if idx is not None else [])
    for o in outs:
        for buf, oname in ((o.flat, 'the gradients'), (o.stats, 'the statistics'), (outs[0].workspace, 'the workspace')):
            for t, name in ins:
                if _overlap(buf, t):
                    raise ValueError("%s overlap %s: the call does not work in place" % (oname, name))
    a = _lg.new_args(_lg.CriticArgs)
    a.device, a.dtype, a.n_blocks, a.n_critics, a.n_outer, a.n_inner = obs.device.index, _DTYPES[obs.dtype], n_blocks, len(critics), n_outer, n_inner
    for j, c in enumerate(critics):
        a.critics[j] = _critic_struct(c, obs.device, obs.dtype)[0]
        a.grad[j], a.stats[j] = outs[j].flat.data_ptr(), outs[j].stats.data_ptr()
    size = obs.element_size()
    a.obs = _lg.View(ts[0].data_ptr() + offs[0] * size, *strides[0])
    a.action = _lg.View(ts[1].data_ptr() + offs[1] * size, *strides[1])
    a.target, a.target_stride = target.data_ptr(), (target.stride(0) if M > 1 else 1)
    if idx is not None:
        a.idx, a.n_idx = idx.data_ptr(), idx.numel()
    a.workspace, a.workspace_bytes = outs[0].workspace.data_ptr(), outs[0].workspace.numel()
    a.stream = _stream(obs.device.index)
    _lg.check(lib.atacom_offgrad_critic_gradient(a))
    return outs[0] if single else outs


def actor_gradient(actor, critic, obs, *, idx=None, out=None, action_out=None, dqda_out=None, n_blocks=0):
    """The deterministic policy gradient: the gradient of  -Q(obs, pi(obs)).mean()  over the rows of obs [..., D] (or those `idx`
    names) with respect to the six tensors of `actor` (an MlpPolicy; act_scale * tanh(.) for one of from_td3 / from_ddpg); the
    QCritic is only read.  -> fit.Gradients of the value head's key (stats: the loss, 0, 0, 0), which optim.Adam accepts for a
    group without log_std.  action_out [M, k] receives pi(obs), dqda_out [M, k] receives dQ/da; both are optional."""
    if not isinstance(critic, QCritic):
        raise ValueError("critic must be a QCritic")
    from .engine import MlpPolicy
    if not isinstance(actor, MlpPolicy):
        raise ValueError("actor must be an MlpPolicy")
    D, k, n1 = _sizes(critic)
    W1, W3 = actor.tensors['W1'], actor.tensors['W3']
    if (int(W1.shape[1]), int(W3.shape[0])) != (D, k):
        raise ValueError("the actor maps %d to %d where the critic takes %d observation and %d action elements" % (
            W1.shape[1], W3.shape[0], D, k))
    lead = _obs_checks(obs)
    ts = [_check_rows(obs, 'obs', lead, D, obs)]
    offs, n_outer, n_inner, strides = _one_launch(ts, ('obs',), lead)
    idx = _idx(idx, obs)
    M = idx.numel() if idx is not None else n_outer * n_inner
    n_blocks = _checked_blocks(n_blocks)
    _needs_gpu(obs)
    lib = _lg.load()
    need = lib.atacom_offgrad_workspace_size(_DTYPES[obs.dtype], 1, D, k, 0, M, n_blocks)
    if need == 0:
        _lg.check(_lg.E_INVALID)
    key = (D, k, _lf.VALUE, obs.dtype, obs.device)
    if out is None:
        out = Gradients(D, k, _lf.VALUE, obs.dtype, obs.device, need, key)
    elif not isinstance(out, Gradients) or out.key != key:
        raise ValueError("out must be the Gradients of an actor_gradient call for a %d -> %d network in %s on %s" % (D, k, obs.dtype, obs.device))
    elif out.workspace.numel() < need:
        raise ValueError("out was made for fewer workgroups: its workspace holds %d bytes where this call needs %d" % (
            out.workspace.numel(), need))
    a = _lg.new_args(_lg.ActorArgs)
    outs = [(out.flat, 'the gradients'), (out.stats, 'the statistics'), (out.workspace, 'the workspace')]
    if action_out is not None:
        action_out, a.action_out_stride = _rows_out(action_out, 'action_out', M, k, obs)
        a.action_out = action_out.data_ptr()
        outs.append((action_out, 'action_out'))
    if dqda_out is not None:
        dqda_out, a.dqda_out_stride = _rows_out(dqda_out, 'dqda_out', M, k, obs)
        a.dqda_out = dqda_out.data_ptr()
        outs.append((dqda_out, 'dqda_out'))
    ins = [(ts[0], 'obs')] + ([(idx, 'idx')] if idx is not None else [])
    for o, oname in outs:
        for t, name in ins + [p for p in outs if p[0] is not o]:
            if _overlap(o, t):
                raise ValueError("%s overlap %s: the call does not work in place" % (oname, name))
    a.device, a.dtype, a.n_blocks, a.n_outer, a.n_inner = obs.device.index, _DTYPES[obs.dtype], n_blocks, n_outer, n_inner
    a.actor = actor.as_struct_on(obs.device, obs.dtype)
    a.critic = _critic_struct(critic, obs.device, obs.dtype)[0]
    a.obs = _lg.View(ts[0].data_ptr() + offs[0] * obs.element_size(), *strides[0])
    if idx is not None:
        a.idx, a.n_idx = idx.data_ptr(), idx.numel()
    a.grad, a.stats = out.flat.data_ptr(), out.stats.data_ptr()
    a.workspace, a.workspace_bytes = out.workspace.data_ptr(), out.workspace.numel()
    a.stream = _stream(obs.device.index)
    _lg.check(lib.atacom_offgrad_actor_gradient(a))
    return out
