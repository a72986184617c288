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
from .evaluate import _check_rows, _launches, _records
from .returns import _overlap, _stream

_DTYPES = {torch.float32: _lf.F32, torch.float64: _lf.F64}
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
        o = 0
        for name, shape in (('W1', (64, n_in)), ('b1', (64,)), ('W2', (64, 64)), ('b2', (64,)), ('W3', (n_out, 64)), ('b3', (n_out,)),
                            ('log_std', (n_out,) if head == _lf.PPO_CLIP else None)):
            if shape is None:
                setattr(self, name, None)
                continue
            n = 1
            for s in shape:
                n *= s
            setattr(self, name, self.flat[o:o + n].view(shape))
            o += n

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
    if not isinstance(x, torch.Tensor) or x.dim() < 1:
        raise ValueError("obs must be a tensor [..., n_in]")
    if x.dtype not in _DTYPES:
        raise ValueError("obs must be float32 or float64, got %s" % x.dtype)
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
    lead = tuple(x.shape[:-1])
    if any(n == 0 for n in lead):
        raise ValueError("obs holds no rows: %s" % (tuple(x.shape),))
    one = lambda t: t.unsqueeze(-1) if isinstance(t, torch.Tensor) else t           # noqa: E731
    wname = 'adv' if ppo else 'target'
    ts, slots, names = [_check_rows(x, 'obs', lead, m.n_in, x)], ['x'], ['obs']
    if ppo:
        ts.append(_check_rows(action, 'action', lead, m.n_out, x))
        slots.append('action')
        names.append('action')
    ts.append(_check_rows(one(weight), wname, lead, 1, x))
    slots.append('weight')
    names.append(wname)
    if ppo:
        ts.append(_check_rows(one(logp_old), 'logp_old', lead, 1, x))
        slots.append('logp_old')
        names.append('logp_old')
    launches = _launches(lead, [t.stride()[:-1] for t in ts])
    if len(launches) != 1:
        raise ValueError("the leading dimensions %s with strides %s do not collapse to one (outer, inner) pair: a gradient "
                         "cannot be split over launches" % (lead, [t.stride()[:-1] for t in ts]))
    offs, n_outer, n_inner, strides = launches[0]
    if idx is not None:
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.dim() != 1 or idx.numel() < 1:
            raise ValueError("idx must be a one-dimensional int64 tensor of at least one row number")
        if idx.device != x.device or not idx.is_contiguous():
            raise ValueError("idx must be contiguous and on %s, got %s" % (x.device, idx.device))
    if not 0 <= int(n_blocks) <= _lf.MAX_BLOCKS:
        raise ValueError("n_blocks must be 0 (the library chooses) .. %d, got %d" % (_lf.MAX_BLOCKS, n_blocks))
    if x.device.type != 'cuda':                        # the last check that needs no device: everything above is about shapes
        raise ValueError("the kernels of libatacom_fit.so run on a GPU; got tensors on %s" % x.device)
    a = _lf.new_args()
    a.device, a.dtype, a.n_blocks, a.head, a.net = x.device.index, _DTYPES[x.dtype], int(n_blocks), head, m
    a.n_outer, a.n_inner, a.clip = n_outer, n_inner, float(clip)
    if idx is not None:
        a.idx, a.n_idx = idx.data_ptr(), idx.numel()
    lib = _lf.load()
    need = lib.atacom_fit_workspace_size(a)
    if need == 0:
        _lf.check(_lf.E_INVALID)
    key = (m.n_in, m.n_out, head, x.dtype, x.device)
    if out is None:
        out = Gradients(m.n_in, m.n_out, head, x.dtype, x.device, need, key)
    elif not isinstance(out, Gradients) or out.key != key:
        raise ValueError("out must be the Gradients of a %s call for a %d -> %d network in %s on %s" % (
            _HEADS[head], m.n_in, m.n_out, x.dtype, x.device))
    elif out.workspace.numel() < need:
        raise ValueError("out was made for fewer workgroups: its workspace holds %d bytes where this call needs %d" % (
            out.workspace.numel(), need))
    for o, oname in ((out.flat, 'the gradients'), (out.stats, 'the statistics'), (out.workspace, 'the workspace')):
        for t, name in list(zip(ts, names)) + ([(idx, 'idx')] if idx is not None else []):
            if _overlap(o, t):
                raise ValueError("%s overlap %s: the call does not work in place" % (oname, name))
    size = x.element_size()
    for t, s, off, (so, si) in zip(ts, slots, offs, strides):
        setattr(a, s, _lf.View(t.data_ptr() + off * size, so, si))
    a.grad, a.stats = out.flat.data_ptr(), out.stats.data_ptr()
    a.workspace, a.workspace_bytes = out.workspace.data_ptr(), out.workspace.numel()
    a.stream = _stream(x.device.index)
    _lf.check(lib.atacom_fit_gradient(a))
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


def _columns(layout, rec):
    """Full records [W, T, Bm, F] (or [T, Bm, F]) or compact records [W, T + 1, Bm, Fc] (or [T + 1, Bm, Fc]), whose tail row
    holds no action and is left out, as log_prob_from_records reads them."""
    Fc = getattr(layout, 'Fc', None)
    if isinstance(rec, torch.Tensor) and Fc is not None and rec.shape[-1] == Fc and rec.dim() in (3, 4):
        if rec.shape[-3] != layout.T + 1:
            raise ValueError("compact records must hold %d rows of time (the tail included), got %d" % (layout.T + 1, rec.shape[-3]))
        return rec[..., :layout.T, :, :]
    return _records(layout, rec, layout.F, 'records')


def value_gradient_from_records(layout, rec, target, critic, *, idx=None, out=None):
    """value_gradient with the obs column of packed records of `layout` read in place; target [W, T, Bm] (or [T, Bm]), `idx`
    numbers the flat [W * T * Bm] rows."""
    rec = _columns(layout, rec)
    return value_gradient(critic, rec[..., layout.fields['obs']], target, idx=idx, out=out)


def policy_gradient_from_records(layout, rec, adv, logp_old, policy, *, clip=0.2, idx=None, out=None):
    """policy_gradient with the obs and action columns of packed records of `layout` read in place; adv and logp_old
    [W, T, Bm] (or [T, Bm]), `idx` numbers the flat [W * T * Bm] rows."""
    rec = _columns(layout, rec)
    return policy_gradient(policy, rec[..., layout.fields['obs']], rec[..., layout.fields['action']], adv, logp_old, clip=clip,
                           idx=idx, out=out)
