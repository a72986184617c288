"""The policy step of a trust-region update (TRPO) on the device -- the host side of libatacom_trust.so
(include/atacom_trust_hip.h states the arithmetic).  The one stage of TRPO that the collection, evaluation, GAE and fitting
libraries do not cover is the product of the policy's Fisher matrix with a vector, which MushroomRL forms as

    kl = kl_divergence(old_dist, policy.distribution(obs)).mean()
    grads = torch.autograd.grad(kl, params, create_graph=True)
    Fv = torch.autograd.grad((flat(grads) * v).sum(), params) + damping * v

eleven times an update over the WHOLE collection: a forward, a backward and a backward-of-backward pass of autograd that write
and re-read 64-wide activations.  fisher_vector_product is that product in one launch (plus a small one that adds the
workgroups' partial sums), with the activations, their tangents and the data gradients in registers and LDS, the obs column of
packed records read in place and a minibatch gathered through `idx` in the kernel's row loads.

A direction, like a gradient (fit.Gradients.flat), is ONE flat tensor [P + n_out] in the order W1 [64, n_in], b1, W2, b2,
W3 [n_out, 64], b3, log_std, P = 64 n_in + 64 + 4096 + 64 + 64 n_out + n_out.

natural_gradient is the conjugate-gradient solve of (F + damping I) x = g around it with no host synchronisation, and trpo_step
the whole policy step: the gradient of the surrogate (fit.policy_gradient_from_records with a clip so large that no row is
inactive), the solve, the step length and the backtracking line search on the KL divergence and the surrogate, whose candidates
are written into the policy's own tensors and evaluated with one launch each (evaluate.evaluate_rows).  The loops are
MushroomRL's TRPO, restated.  The critic's fit stays fit.value_gradient_from_records and optim.Adam.

Every call is enqueued on the current stream of the tensors' device.  No numerics of the product here, and no fall-back: a
missing library is an error.
"""
import math

import torch

from . import _lib_trust as _lt
from . import fit as _fit
from ._rows import (carve, check_rows, checked_blocks, checked_idx, columns, fill, inputs, needs_gpu, no_overlap, one_launch, reuse,
                    rows_of, run, sized)
from .evaluate import evaluate_rows

_NAMES = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')
BIG_CLIP = 1e30        # PPO's clip at which no row is inactive: 1 - clip and 1 + clip are finite in float32, and rho >= 0


def _shapes(n_in, n_out):
    return (('W1', (64, n_in)), ('b1', (64,)), ('W2', (64, 64)), ('b2', (64,)), ('W3', (n_out, 64)), ('b3', (n_out,)),
            ('log_std', (n_out,)))


class FisherProduct:
    """What a product call writes: `flat` [P + n_out] = F v + damping v in the order of a direction, the views W1 [64, n_in], b1,
    W2, b2, W3 [n_out, 64], b3 and log_std [n_out] into it, and the `workspace` of the call.  Passed back as `out=`, all of it
    is reused.  FisherProduct.like(policy, obs, idx=, n_blocks=) makes one for a call before the call."""

    def __init__(self, n_in, n_out, dtype, device, workspace_bytes, key):
        self.n_in, self.n_out, self.key = n_in, n_out, key
        self.flat = torch.empty(_lt.size(n_in, n_out), dtype=dtype, device=device)
        self.workspace = torch.empty(workspace_bytes, dtype=torch.uint8, device=device)
        carve(self, self.flat, _shapes(n_in, n_out))

    @classmethod
    def like(cls, policy, obs, *, idx=None, n_blocks=0):
        return _product(policy, obs, None, 0.0, idx, None, n_blocks, make_only=True)


def _product(policy, x, v, damping, idx, out, n_blocks, make_only=False):
    lead = rows_of(x, 'obs')
    if policy.tensors.get('std') is None:
        raise ValueError("the Fisher-vector product needs a policy with std")
    if not (isinstance(damping, (int, float)) and math.isfinite(damping) and damping >= 0.0):
        raise ValueError("damping must be >= 0 and finite, got %r" % (damping,))
    m = policy.as_struct_on(x.device, x.dtype)
    if x.shape[-1] != m.n_in:
        raise ValueError("obs has rows of %d where the network takes %d" % (x.shape[-1], m.n_in))
    check_rows(x, 'obs', lead, m.n_in, x)
    n_all = _lt.size(m.n_in, m.n_out)
    if not make_only:
        if not isinstance(v, torch.Tensor) or v.dim() != 1 or v.numel() != n_all:
            raise ValueError("v must be a one-dimensional tensor of %d values (P + n_out of a %d -> %d policy)" % (n_all, m.n_in, m.n_out))
        if v.dtype != x.dtype or v.device != x.device or not v.is_contiguous():
            raise ValueError("v must be contiguous, %s and on %s, got %s on %s" % (x.dtype, x.device, v.dtype, v.device))
    launch = one_launch((x,), ('obs',), lead, 'a product')
    idx = checked_idx(idx, x)
    n_blocks = checked_blocks(n_blocks, _lt.MAX_BLOCKS)
    key = (m.n_in, m.n_out, x.dtype, x.device)
    describe = lambda: "FisherProduct of a call for a %d -> %d policy in %s on %s" % (m.n_in, m.n_out, x.dtype, x.device)  # noqa: E731
    if out is not None:
        reuse((out,), FisherProduct, key, 0, describe)        # whose it is needs no device; what it holds needs the library
    needs_gpu(x, 'trust')
    a = _lt.new_args()
    fill(a, x, n_blocks, launch, ('x',), (x,), idx)
    a.net, a.damping = m, float(damping)
    lib = _lt.load()
    need = sized(_lt, lib.atacom_trust_workspace_size(a))
    if out is None:
        out = FisherProduct(m.n_in, m.n_out, x.dtype, x.device, need, key)
    else:
        reuse((out,), FisherProduct, key, need, describe)
    if make_only:
        return out
    no_overlap([(out.flat, 'out.flat'), (out.workspace, 'out.workspace')], inputs((x, v), ('obs', 'v'), idx))
    a.v, a.out = v.data_ptr(), out.flat.data_ptr()
    run(a, lib.atacom_trust_fvp, _lt.check, x, out.workspace)
    return out


def fisher_vector_product(policy, obs, v, *, damping=0.0, idx=None, out=None, n_blocks=0):
    """F v + damping v -> a tensor [P + n_out]: F the Fisher matrix of N(policy(obs), diag(std ** 2)) with respect to the
    policy's weights, biases and log std, averaged over the rows of obs [..., n_in] -- or, with `idx` (int64 [M], flat numbers of
    those rows, repeats allowed), over the rows it names; v a direction.  obs may be a strided view (the obs column of packed
    records) as long as its leading dimensions collapse to one (outer, inner) pair.  `idx` is not checked against the number of
    rows (fit.check_idx does that, and synchronises).  `out`: a FisherProduct (made once with FisherProduct.like for the
    same policy, obs and idx); with it the call allocates nothing, returns out.flat and can be captured in a graph."""
    return _product(policy, obs, v, damping, idx, out, n_blocks).flat


def fisher_vector_product_from_records(layout, rec, v, policy, *, damping=0.0, idx=None, out=None, n_blocks=0):
    """fisher_vector_product with the obs column of full or compact packed records of `layout` read in place (the tail row of
    compact records is left out); `idx` numbers the flat [W * T * Bm] rows."""
    rec = columns(layout, rec)
    return fisher_vector_product(policy, rec[..., layout.fields['obs']], v, damping=damping, idx=idx, out=out, n_blocks=n_blocks)


class CgWork:
    """The buffers of natural_gradient: x, r, p [P + n_out], the FisherProduct z and the 0-dim scalars of the loop.  Made by
    CgWork.like(policy, obs, idx=); passed as `work=`, the solve allocates nothing."""

    def __init__(self, product):
        f = product.flat
        self.z = product
        self.x, self.r, self.p = torch.empty_like(f), torch.empty_like(f), torch.empty_like(f)
        self.r2, self.r2n, self.pz, self.a, self.beta, self.cr, self.tol = (torch.zeros((), dtype=f.dtype, device=f.device) for _ in range(7))
        self.zero, self.one = torch.zeros((), dtype=f.dtype, device=f.device), torch.ones((), dtype=f.dtype, device=f.device)
        self.done, self.now = (torch.zeros((), dtype=torch.bool, device=f.device) for _ in range(2))

    @classmethod
    def like(cls, policy, obs, *, idx=None, n_blocks=0):
        return cls(FisherProduct.like(policy, obs, idx=idx, n_blocks=n_blocks))


def natural_gradient(policy, obs, g, *, iters=10, damping=1e-2, residual_tol=1e-10, idx=None, work=None):
    """x with (F + damping I) x ~ g by `iters` steps of conjugate gradients -> x [P + n_out] (work.x; work.r2 is the squared
    residual).  MushroomRL's loop, with its `break` as a device-side flag: once r . r < residual_tol, the coefficients of later
    iterations are chosen (torch.where) so that x, r and p stay as they are, bit for bit, so nothing visits the host.  With
    `work=` (CgWork.like) the solve allocates nothing and is a linear chain on the current stream, capturable in a graph."""
    if not isinstance(iters, int) or iters < 1:
        raise ValueError("iters must be an integer >= 1, got %r" % (iters,))
    if not (isinstance(residual_tol, (int, float)) and math.isfinite(residual_tol)):
        raise ValueError("residual_tol must be finite, got %r" % (residual_tol,))
    if work is None:
        work = CgWork.like(policy, obs, idx=idx)
    elif not isinstance(work, CgWork):
        raise ValueError("work must be a CgWork")
    w = work
    if not isinstance(g, torch.Tensor) or g.shape != w.x.shape or g.dtype != w.x.dtype or g.device != w.x.device:
        raise ValueError("g must be a %s tensor of %d values on %s" % (w.x.dtype, w.x.numel(), w.x.device))
    w.tol.fill_(float(residual_tol))
    w.done.fill_(False)
    w.x.zero_()
    w.r.copy_(g)
    w.p.copy_(g)
    torch.dot(w.r, w.r, out=w.r2)
    for _ in range(iters):
        _product(policy, obs, w.p, damping, idx, w.z, 0)
        torch.dot(w.p, w.z.flat, out=w.pz)
        torch.div(w.r2, w.pz, out=w.a)
        torch.where(w.done, w.zero, w.a, out=w.a)                   # frozen: x + 0 p, r - 0 z
        w.x.addcmul_(w.p, w.a)
        w.r.addcmul_(w.z.flat, w.a, value=-1.0)
        torch.dot(w.r, w.r, out=w.r2n)
        torch.div(w.r2n, w.r2, out=w.beta)
        torch.where(w.done, w.one, w.beta, out=w.beta)              # frozen: p = 0 r + 1 p
        torch.where(w.done, w.zero, w.one, out=w.cr)
        w.p.mul_(w.beta).addcmul_(w.r, w.cr)
        torch.where(w.done, w.r2, w.r2n, out=w.r2)
        torch.lt(w.r2, w.tol, out=w.now)
        w.done.logical_or_(w.now)
    return w.x


def _parameters(policy, log_std, ref):
    """The policy's six tensors and log_std as the kernels see them: on the records' device, in their dtype, contiguous -- a
    copy would take the candidate's values and lose them."""
    ts = [policy.tensors[n] for n in _NAMES] + [log_std, policy.tensors.get('std')]
    for name, t in zip(_NAMES + ('log_std', 'std'), ts):
        if not isinstance(t, torch.Tensor) or t.dtype != ref.dtype or t.device != ref.device or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor on %s: the line search writes its candidates into it" % (
                name, ref.dtype, ref.device))
    n_in, n_out = ts[0].shape[1], ts[4].shape[0]
    for (name, shape), t in zip(_shapes(n_in, n_out) + (('std', (n_out,)),), ts):
        if tuple(t.shape) != shape:
            raise ValueError("%s must have the shape %s" % (name, shape))
    return [t.detach() for t in ts[:7]], ts[7].detach(), n_in, n_out


def trpo_step(layout, rec, adv, logp_old, policy, log_std, *, max_kl=1e-2, ent_coeff=0.0, cg_iters=10, cg_damping=1e-2,
              cg_residual_tol=1e-10, line_search=10):
    """One TRPO policy step over the records `rec` of `layout` (full or compact), advantages `adv` and collection-time
    log-probabilities `logp_old` [W, T, Bm] (or [T, Bm]):
        g = grad (mean rho A + ent_coeff H),  x = natural_gradient(g),  full = x / sqrt(x . (F + damping) x / 2 / max_kl),
        theta = theta_old + full 2^-j  for the first j < line_search with KL(old || theta) <= 1.5 max_kl and L(theta) >= L(old).
    The candidates are written into policy.tensors and `log_std` in place, and exp(log_std) into policy.tensors['std']; if none
    is accepted everything is restored bit for bit.  -> dict(loss_old, loss_new, kl, halvings, accepted, cg_residual); rejected:
    loss_new = loss_old, kl = 0, halvings = line_search.  One read-back per candidate, as the reference."""
    cols = columns(layout, rec)
    if not isinstance(line_search, int) or line_search < 1:
        raise ValueError("line_search must be an integer >= 1, got %r" % (line_search,))
    if not (isinstance(max_kl, (int, float)) and max_kl > 0.0 and math.isfinite(max_kl)):
        raise ValueError("max_kl must be > 0 and finite, got %r" % (max_kl,))
    params, std, n_in, n_out = _parameters(policy, log_std, cols)
    obs, act = cols[..., layout.fields['obs']], cols[..., layout.fields['action']]
    lead = tuple(cols.shape[:-1])
    # ---- the gradient of the surrogate: -1 x PPO's with no row inactive; the entropy adds ent_coeff per log std
    grad = _fit.policy_gradient_from_records(layout, rec, adv, logp_old, policy, clip=BIG_CLIP)
    g = grad.flat.neg_()
    if ent_coeff:
        grad.log_std.add_(float(ent_coeff))
    # ---- the natural gradient and the full step
    work = CgWork.like(policy, obs)
    x = natural_gradient(policy, obs, g, iters=cg_iters, damping=cg_damping, residual_tol=cg_residual_tol, work=work)
    shs = 0.5 * torch.dot(x, _product(policy, obs, x, cg_damping, None, work.z, 0).flat)
    full = x / torch.sqrt(shs / max_kl)
    # ---- what the search compares against, saved once: the old parameters, means and std
    old = torch.cat([t.reshape(-1) for t in params])
    std_old = std.clone()
    mean_old, mean = torch.empty(lead + (n_out,), dtype=cols.dtype, device=cols.device), torch.empty(lead + (n_out,), dtype=cols.dtype, device=cols.device)
    lp = torch.empty(lead, dtype=cols.dtype, device=cols.device)
    const = 0.5 * n_out * (1.0 + math.log(2.0 * math.pi))

    def surrogate():
        return ((lp - logp_old).exp() * adv).mean() + ent_coeff * (params[6].sum() + const)

    evaluate_rows(policy, obs, act, y=mean_old, logp=lp)
    loss_old = float(surrogate())
    var_old = std_old * std_old
    out = dict(loss_old=loss_old, loss_new=loss_old, kl=0.0, halvings=line_search, accepted=False, cg_residual=float(work.r2))
    for j in range(line_search):
        o = 0
        for t in params:
            n = t.numel()
            torch.add(old[o:o + n].view_as(t), full[o:o + n].view_as(t), alpha=0.5 ** j, out=t)
            o += n
        torch.exp(params[6], out=std)
        evaluate_rows(policy, obs, act, y=mean, logp=lp)
        kl = ((std / std_old).log() + (var_old + (mean_old - mean) ** 2) / (2.0 * std * std) - 0.5).sum(-1).mean()
        kl, loss = torch.stack([kl, surrogate()]).tolist()
        if kl <= 1.5 * max_kl and loss - loss_old >= 0.0:
            out.update(loss_new=loss, kl=kl, halvings=j, accepted=True)
            return out
    o = 0
    for t in params:                                    # nothing accepted: everything as it was, bit for bit
        n = t.numel()
        t.copy_(old[o:o + n].view_as(t))
        o += n
    std.copy_(std_old)
    return out
