"""The gradients of an on-policy update, on the device and in one launch per network (plus a small one that adds the workgroups'
partial sums): the mean-squared-error loss of a critic and PPO's clipped surrogate of an actor with a state-independent
Gaussian, differentiated through the project's architecture (MlpPolicy: Linear(n_in, 64) - act - Linear(64, 64) - act -
Linear(64, n_out)) over a minibatch of the rows of a finished collection -- the host side of libatacom_fit.so
(include/atacom_fit_hip.h states the arithmetic).  It replaces, in a learner's inner loop,

    mu = actor(obs[idx]); logp = ...; ratio = (logp - logp_old[idx]).exp()
    (-torch.min(ratio * adv[idx], ratio.clamp(1 - clip, 1 + clip) * adv[idx]).mean()).backward()
    ((critic(obs[idx]).squeeze(-1) - ret[idx]).pow(2).mean()).backward()

-- the gathered copies, two forward and two backward passes of autograd -- by two calls that read the obs and action columns of
packed records in place, gather through `idx` in the kernel's row loads and write every gradient into one flat buffer.  The
optimiser stays torch's: Gradients.to_module() hands the buffer's views to the parameters as their .grad.

The weights are used where they lie (MlpPolicy.as_struct_on takes tensors that are on the device in the dtype as they are), so
a policy made once with MlpPolicy.from_module(actor, std=std) sees the optimiser's in-place steps at the next call.  std is a
tensor of the policy, not a function of the learner's log_std: the caller refreshes it in place after a step,
`policy.tensors['std'].copy_(log_std.exp())`.  The entropy bonus of a state-independent Gaussian, sum_k log std_k + const, has
the constant gradient 1 per log std; a learner that wants it adds  -coefficient  to Gradients.log_std itself -- it is not part
of the library.

Every call is enqueued on the current stream of the tensors' device and nothing synchronises.  With `out=` a call allocates
nothing and can be captured in a graph.  No numerics here, and no fall-back: a missing library is an error.
"""
import torch

from . import _lib_fit as _lf
from ._rows import (buffers, carve, check_rows, checked_blocks, checked_idx, column, columns, fill, inputs, needs_gpu, no_overlap,
                    one_launch, reuse, rows_of, run, sized)

_HEADS = {_lf.VALUE: 'value', _lf.PPO_CLIP: 'PPO'}


class Gradients:
    """What a gradient call writes: `flat`, one buffer in the order dW1, db1, dW2, db2, dW3, db3 (and d log std for a policy),
    the views W1 [64, n_in], b1, W2, b2, W3 [n_out, 64], b3 and log_std [n_out] (None for a critic) into it, `stats` [4] = loss,
    the share of rows whose ratio term is inactive, mean(logp_old - logp), 0 (a critic: loss, 0, 0, 0) and the `workspace` of the
    call.  Passed back as `out=`, all of it is reused."""

    def __init__(self, n_in, n_out, head, dtype, device, workspace_bytes, key):
        self.n_in, self.n_out, self.head, self.key = n_in, n_out, head, key
        self.flat = torch.empty(_lf.grad_size(n_in, n_out, head), dtype=dtype, device=device)
        self.stats = torch.empty(_lf.STATS, dtype=dtype, device=device)
        self.workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=device)
        carve(self, self.flat, (('W1', (64, n_in)), ('b1', (64,)), ('W2', (64, 64)), ('b2', (64,)), ('W3', (n_out, 64)), ('b3', (n_out,)),
                                ('log_std', (n_out,) if head == _lf.PPO_CLIP else None)))

    @property
    def loss(self):
        return self.stats[0]

    def to_module(self, net, log_std=None):
        """Make the views the .grad of net._h1 / _h2 / _h3's weights and biases (and of `log_std`, for a policy): after it
        torch.optim.Adam.step() works unchanged.  The parameters then share the buffer: the next call with out=self overwrites
        their .grad in place."""
        for lin, W, b in ((net._h1, self.W1, self.b1), (net._h2, self.W2, self.b2), (net._h3, self.W3, self.b3)):
            for par, g in ((lin.weight, W), (lin.bias, b)):
                if tuple(par.shape) != tuple(g.shape) or par.dtype != g.dtype or par.device != g.device:
                    raise ValueError("a parameter is %s %s on %s where its gradient is %s %s on %s" % (
                        tuple(par.shape), par.dtype, par.device, tuple(g.shape), g.dtype, g.device))
                par.grad = g
        if log_std is not None:
            if self.log_std is None:
                raise ValueError("the gradient of a critic holds no d log std")
            if tuple(log_std.shape) != tuple(self.log_std.shape) or log_std.dtype != self.log_std.dtype:
                raise ValueError("log_std must be a %s tensor of shape %s" % (self.log_std.dtype, tuple(self.log_std.shape)))
            log_std.grad = self.log_std
        return self


def check_idx(idx, n_rows):
    """The library does not guard a row number out of range (its header says so); this does, on request: it reads idx back,
    so it synchronises.  Raises ValueError."""
    lo, hi = int(idx.min()), int(idx.max())
    if lo < 0 or hi >= n_rows:
        raise ValueError("idx holds row numbers from %d to %d where the rows are 0 .. %d" % (lo, hi, n_rows - 1))


def _gradient(net, head, x, action, weight, logp_old, clip, idx, out, n_blocks):
    lead = rows_of(x, 'obs')
    ppo = head == _lf.PPO_CLIP
    if ppo and net.tensors.get('std') is None:
        raise ValueError("the policy gradient needs a policy with std")
    if ppo and not float(clip) > 0.0:
        raise ValueError("clip must be > 0, got %r" % (clip,))
    m = net.as_struct_on(x.device, x.dtype)
    if x.shape[-1] != m.n_in:
        raise ValueError("obs has rows of %d where the network takes %d" % (x.shape[-1], m.n_in))
    if not ppo and m.n_out != 1:
        raise ValueError("the critic must map the %d observation elements to one value" % m.n_in)
    rows = [('x', 'obs', x, m.n_in), ('weight', 'target', column(weight), 1)]
    if ppo:
        rows = [rows[0], ('action', 'action', action, m.n_out), ('weight', 'adv', column(weight), 1),
                ('logp_old', 'logp_old', column(logp_old), 1)]
    slots, names, ts, _ = zip(*rows)
    for _, name, t, width in rows:
        check_rows(t, name, lead, width, x)
    launch = one_launch(ts, names, lead, 'a gradient')
    idx = checked_idx(idx, x)
    n_blocks = checked_blocks(n_blocks, _lf.MAX_BLOCKS)
    needs_gpu(x, 'fit')
    a = _lf.new_args()
    fill(a, x, n_blocks, launch, slots, ts, idx)
    a.head, a.net, a.clip = head, m, float(clip)
    lib = _lf.load()
    need = sized(_lf, lib.atacom_fit_workspace_size(a))
    key = (m.n_in, m.n_out, head, x.dtype, x.device)
    if out is None:
        out = Gradients(m.n_in, m.n_out, head, x.dtype, x.device, need, key)
    else:
        reuse((out,), Gradients, key, need, lambda: "Gradients of a %s call for a %d -> %d network in %s on %s" % (
            _HEADS[head], m.n_in, m.n_out, x.dtype, x.device))
    no_overlap(buffers(out), inputs(ts, names, idx))
    a.grad, a.stats = out.flat.data_ptr(), out.stats.data_ptr()
    run(a, lib.atacom_fit_gradient, _lf.check, x, out.workspace)
    return out


def value_gradient(critic, obs, target, *, idx=None, out=None, n_blocks=0):
    """The gradient of  (critic(obs) - target) ** 2 .mean()  over the rows of obs [..., n_in] and target [...] -- or, with `idx`
    (int64 [M], flat numbers of those rows, repeats allowed), over the rows it names -- with respect to the critic's weights
    and biases -> Gradients.  obs and target share their leading dimensions and may be strided views (the columns of packed
    records) as long as the leading dimensions collapse to one (outer, inner) pair.  `idx` is not checked against the number
    of rows (check_idx does that, and synchronises).  `out`: the Gradients of an earlier call of the same kind."""
    return _gradient(critic, _lf.VALUE, obs, None, target, None, 0.0, idx, out, n_blocks)


def policy_gradient(policy, obs, action, adv, logp_old, *, clip=0.2, idx=None, out=None, n_blocks=0):
    """The gradient of PPO's clipped surrogate  -min(rho adv, clamp(rho, 1 - clip, 1 + clip) adv).mean(),  rho = exp(logp -
    logp_old), logp the log-probability of action [..., n_out] under N(policy(obs), diag(std ** 2)), with respect to the
    policy's weights and biases and to log std -> Gradients (stats: loss, clipped share, mean(logp_old - logp), 0).  The
    arguments are as in value_gradient."""
    return _gradient(policy, _lf.PPO_CLIP, obs, action, adv, logp_old, clip, idx, out, n_blocks)


def value_gradient_from_records(layout, rec, target, critic, *, idx=None, out=None):
    """value_gradient with the obs column of packed records of `layout` read in place; target [W, T, Bm] (or [T, Bm]), `idx`
    numbers the flat [W * T * Bm] rows."""
    rec = columns(layout, rec)
    return value_gradient(critic, rec[..., layout.fields['obs']], target, idx=idx, out=out)


def policy_gradient_from_records(layout, rec, adv, logp_old, policy, *, clip=0.2, idx=None, out=None):
    """policy_gradient with the obs and action columns of packed records of `layout` read in place; adv and logp_old
    [W, T, Bm] (or [T, Bm]), `idx` numbers the flat [W * T * Bm] rows."""
    rec = columns(layout, rec)
    return policy_gradient(policy, rec[..., layout.fields['obs']], rec[..., layout.fields['action']], adv, logp_old, clip=clip,
                           idx=idx, out=out)
