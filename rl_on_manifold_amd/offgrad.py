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
from . import _rows
from ._rows import (DTYPES, buffers, carve, check_rows, checked_blocks, checked_idx, fill, inputs, n_rows, needs_gpu, network_struct,
                    no_overlap, one_launch, optional_rows, reuse, rows_of, run, sized)
from .fit import Gradients
from .offpolicy import QCritic

_KINDS = {'ddpg': _lg.DDPG, 'td3': _lg.TD3}
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
        carve(self, self.flat, (('W1', (64, n1)), ('b1', (64,)), ('W2', (64, 64)), ('b2', (64,)), ('W3', (1, 64)), ('b3', (1,)),
                                ('W2a', (64, n_act))))

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
    """The atacom_offgrad_critic of a QCritic: this library's own ctypes struct, filled like QCritic.as_struct_on; its copies
    live beside those of the forward calls, as long as the critic or until the next gradient call."""
    c = network_struct(critic, critic.shapes(), _lg.Critic, device, dtype, keep='_keep_offgrad')
    c.kind, c.n_obs, c.n_act, c.activation = _KINDS[critic.kind], critic.n_obs, critic.n_act, critic.activation
    return c


def _fresh(n, need, key):
    """n QGradients of `key` = (n1, k, dtype, device) on one workspace of `need` bytes."""
    ws = torch.empty(need, dtype=torch.uint8, device=key[3])
    return tuple(QGradients(*key, ws, key) for _ in range(n))


def _sizes(critic):
    D, k = critic.n_obs, critic.n_act
    n1 = D + k if critic.kind == 'td3' else D
    if not 1 <= D <= _lg.MAX_IN or not 1 <= k <= _lg.MAX_ACT:
        raise ValueError("a critic of %d observation and %d action elements is outside 1 .. %d and 1 .. %d" % (D, k, _lg.MAX_IN, _lg.MAX_ACT))
    if n1 > _lg.MAX_IN:
        raise ValueError("n1 = %d first-layer inputs exceed %d" % (n1, _lg.MAX_IN))
    return D, k, n1


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
    outs = _rows.critic_gradient(_lg, 'offgrad', critics, (D, k), obs, action, target, idx, out, n_blocks, (
        QGradients, (n1, k), (n1, 1, k), _fresh, _critic_struct,
        "QGradients (one per critic) of a call for critics of %d first-layer inputs and %d action elements" % (n1, k)))
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
    lead = rows_of(obs, 'obs')
    ts = [check_rows(obs, 'obs', lead, D, obs)]
    launch = one_launch(ts, ('obs',), lead)
    idx = checked_idx(idx, obs)
    M = n_rows(idx, launch)
    n_blocks = checked_blocks(n_blocks, _lg.MAX_BLOCKS)
    needs_gpu(obs, 'offgrad')
    lib = _lg.load()
    need = sized(_lg, lib.atacom_offgrad_workspace_size(DTYPES[obs.dtype], 1, D, k, 0, M, n_blocks))
    key = (D, k, _lf.VALUE, obs.dtype, obs.device)
    if out is None:
        out = Gradients(D, k, _lf.VALUE, obs.dtype, obs.device, need, key)
    else:
        reuse((out,), Gradients, key, need, lambda: "Gradients of an actor_gradient call for a %d -> %d network in %s on %s" % (
            D, k, obs.dtype, obs.device))
    a = _lg.new_args(_lg.ActorArgs)
    outs = buffers(out)
    optional_rows(a, outs, obs, M, [('action_out', action_out, k), ('dqda_out', dqda_out, k)])
    no_overlap(outs, inputs(ts, ('obs',), idx))
    fill(a, obs, n_blocks, launch, ('obs',), ts, idx)
    a.actor = actor.as_struct_on(obs.device, obs.dtype)
    a.critic = _critic_struct(critic, obs.device, obs.dtype)
    a.grad, a.stats = out.flat.data_ptr(), out.stats.data_ptr()
    run(a, lib.atacom_offgrad_actor_gradient, _lg.check, obs, out.workspace)
    return out
