"""The network evaluation of an on-policy iteration, on the device and in one launch per network: a critic or an actor of the
project's architecture (MlpPolicy: Linear(n_in, 64) - act - Linear(64, 64) - act - Linear(64, n_out)) over every row of a
finished collection, and the log-probability of the recorded actions under the diagonal Gaussian around the actor's mean -- the
host side of libatacom_evaluate.so (include/atacom_evaluate_hip.h states the arithmetic).  It stands between the collection
(rollout_policy / rollout_compact) and the advantages (returns.py), where a learner otherwise runs critic(obs),
critic(next_obs), actor(obs) and the log-probability expression as chains of torch kernels over contiguous copies: the kernels
here read the obs, next_obs and action columns of packed records -- full [W, T, Bm, 2 D + k + 3] or compact
[W, T + 1, Bm, D + k + 3] -- in place, and a compact collection never has its next_obs built.

Every call is enqueued on the current stream of the tensors' device and nothing synchronises.  Forward passes only: nothing
here is differentiable.  No numerics here, and no fall-back: a missing library is an error.
"""
import torch

from . import _lib_evaluate as _le
from ._rows import check_rows, checked_blocks, column, columns, fill, launches, needs_gpu, no_overlap, records_of, rows_of, run


def evaluate_rows(net, x, action=None, *, y=None, logp=None, n_blocks=0):
    """One pass of the network over the rows of x [..., n_in] that writes what is given: y [..., n_out], the network's output,
    and / or logp [...], the log-probability of action [..., n_out] under N(y, diag(net std ** 2)).  The tensors share their
    leading dimensions and may be strided views (the columns of packed records) whose rows are contiguous; outputs overlap
    neither an input nor each other.  n_blocks workgroups walk the row tiles (0: the library chooses).  The general entry:
    evaluate_mlp, gaussian_log_prob and the *_from_records functions are written with it."""
    lead = rows_of(x, 'x')
    if y is None and logp is None:
        raise ValueError("neither y nor logp is given: nothing to compute")
    if logp is not None and (action is None or net.tensors.get('std') is None):
        raise ValueError("logp needs the actions and a policy with std")
    m = net.as_struct_on(x.device, x.dtype)
    if x.shape[-1] != m.n_in:
        raise ValueError("x has rows of %d where the network takes %d" % (x.shape[-1], m.n_in))
    ins, outs = [(check_rows(x, 'x', lead, m.n_in, x), 'x')], []
    if logp is not None:
        ins.append((check_rows(action, 'action', lead, m.n_out, x), 'action'))
    if y is not None:
        outs.append((check_rows(y, 'y', lead, m.n_out, x), 'y'))
    if logp is not None:
        outs.append((check_rows(column(logp), 'logp', lead, 1, x), 'logp'))
    no_overlap(outs, ins)
    n_blocks = checked_blocks(n_blocks, _le.MAX_BLOCKS)
    needs_gpu(x, 'evaluate')
    ts, slots = zip(*ins + outs)
    a = _le.new_args()
    a.net = m
    lib = _le.load()
    for launch in launches(lead, [t.stride()[:-1] for t in ts]):
        fill(a, x, n_blocks, launch, slots, ts)
        run(a, lib.atacom_evaluate_mlp, _le.check, x)


def _out(t, name, lead, width, x):
    if t is None:
        return torch.empty(tuple(lead) + ((width,) if width else ()), dtype=x.dtype, device=x.device)
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(lead) + ((width,) if width else ()):
        raise ValueError("%s must be a tensor of shape %s" % (name, tuple(lead) + ((width,) if width else ())))
    return t


def evaluate_mlp(net, x, *, out=None):
    """net(x) for x [..., n_in] -> [..., n_out]: the network of an MlpPolicy (MlpPolicy.from_module(critic) takes a one-output
    network) with its observation normalisation.  `out`: a tensor of that shape that does not overlap x; with it the call
    allocates nothing and can be captured in a graph."""
    n_out = int(torch.as_tensor(net.tensors['W3']).shape[0])
    y = _out(out, 'out', x.shape[:-1], n_out, x) if isinstance(x, torch.Tensor) and x.dim() >= 1 else out
    evaluate_rows(net, x, y=y)
    return y


def gaussian_log_prob(policy, obs, action, *, out=None, mean_out=None):
    """log N(action; mean(obs), diag(std ** 2)) for obs [..., n_in], action [..., n_out] -> [...]: the log_prob of MushroomRL's
    GaussianTorchPolicy (a state-independent std, policy.tensors['std']), i.e. of torch.distributions.MultivariateNormal(mean,
    diag(std ** 2)), in the same pass as the mean.  `mean_out` [..., n_out], if given, receives the mean."""
    lp = _out(out, 'out', obs.shape[:-1], 0, obs) if isinstance(obs, torch.Tensor) and obs.dim() >= 1 else out
    evaluate_rows(policy, obs, action, y=mean_out, logp=lp)
    return lp


def _critic(layout, critic):
    if int(torch.as_tensor(critic.tensors['W3']).shape[0]) != 1 or int(torch.as_tensor(critic.tensors['W1']).shape[1]) != layout.D:
        raise ValueError("the critic must map the %d observation elements to one value" % layout.D)


def values_from_records(layout, g, critic):
    """(v, v_next) = the critic on the obs and next_obs columns of full packed records g [W, T, Bm, F] (or [T, Bm, F]) of
    `layout` (a RecordLayout), read in place -> two tensors [W, T, Bm] (or [T, Bm]): the arguments of gae_from_records."""
    g = records_of(g, layout.F, 'full records')
    _critic(layout, critic)
    v, vn = torch.empty(g.shape[:-1], dtype=g.dtype, device=g.device), torch.empty(g.shape[:-1], dtype=g.dtype, device=g.device)
    evaluate_rows(critic, g[..., layout.fields['obs']], y=v.unsqueeze(-1))
    evaluate_rows(critic, g[..., layout.fields['next_obs']], y=vn.unsqueeze(-1))
    return v, vn


def values_from_compact(layout, records, ends, n_ends, critic):
    """(v, v_ends) = the critic on the obs column of compact records [W, T + 1, Bm, Fc] (or [T + 1, Bm, Fc]) of `layout` (a
    CompactRecordLayout), tail row included, and on the terminal observations ends[..., 2:] of the exception rows [W, M, D + 2]
    (or [M, D + 2]; None or M = 0: v_ends is None) -> [W, T + 1, Bm] and [W, M]: the two arguments of gae_from_compact.  The
    critic sees (T + 1) Bm + M rows per rank and next_obs is never built.  Every one of the M rows is evaluated; n_ends, which
    says how many of them are valid, is for gae_from_compact to apply."""
    records = records_of(records, layout.Fc, 'compact records')
    if records.shape[-3] != layout.T + 1:
        raise ValueError("compact records must hold %d rows of time (the tail included), got %d" % (layout.T + 1, records.shape[-3]))
    _critic(layout, critic)
    v = torch.empty(records.shape[:-1], dtype=records.dtype, device=records.device)
    evaluate_rows(critic, records[..., layout.compact_fields['obs']], y=v.unsqueeze(-1))
    if ends is None or ends.shape[-2] == 0:
        return v, None
    if ends.dim() != records.dim() - 1 or ends.shape[-1] != layout.E:
        raise ValueError("exception rows must be [%sM, %d], got %s" % ('W, ' if records.dim() == 4 else '', layout.E, tuple(ends.shape)))
    v_ends = torch.empty(ends.shape[:-1], dtype=records.dtype, device=records.device)
    evaluate_rows(critic, ends[..., 2:], y=v_ends.unsqueeze(-1))
    return v, v_ends


def log_prob_from_records(layout, rec, policy):
    """The log-probability of the recorded actions under `policy` at the recorded observations, both read in place: full
    records [W, T, Bm, F] (or [T, Bm, F]) or compact records [W, T + 1, Bm, Fc] (or [T + 1, Bm, Fc]) of `layout` -- obs and
    action sit at the same offsets in both -- -> [W, T, Bm] (or [T, Bm]); the tail row of compact records holds no action and
    is left out."""
    rec = columns(layout, rec)
    lp = torch.empty(rec.shape[:-1], dtype=rec.dtype, device=rec.device)
    evaluate_rows(policy, rec[..., layout.fields['obs']], rec[..., layout.fields['action']], logp=lp)
    return lp
