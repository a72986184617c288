"""What an on-policy learner computes from a finished collection, on the device: generalised advantage estimates with their
returns (MushroomRL's compute_gae), PPO's advantage normalisation, and the discounted episode returns (compute_J) -- the host
side of libatacom_returns.so (include/atacom_returns_hip.h states the arithmetic).  One launch per quantity instead of a Python
loop over time; the kernels read every array where it lies, so the reward and flag columns of packed records -- full
[W, T, Bm, 2 D + k + 3] or compact [W, T + 1, Bm, D + k + 3] -- are consumed in place and next_obs is never rebuilt.

Every call is enqueued on the current stream of the tensors' device and nothing synchronises (gae_from_compact checks the
(t, b) of its exception rows on the host, as CompactRecordLayout.unpack does).  Tensors are [T, B] or [W, T, Bm] views with any
strides; padding rows of ragged shards (`sizes`) are computed like any other row and left out of every statistic.  No numerics
here, and no fall-back: a missing library is an error.
"""
import torch

from . import _lib_returns as _lr
from ._rows import overlap, stream
from .rollout import record_columns

_DTYPES = {torch.float32: _lr.F32, torch.float64: _lr.F64}
_sizes_cache = {}


def _three(x, name, shape=None):
    """[T, B] -> [1, T, B]; [W, T, Bm] as it is."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3):
        raise ValueError("%s must be a [T, B] or [W, T, Bm] tensor" % name)
    x = x.unsqueeze(0) if x.dim() == 2 else x
    if shape is not None and tuple(x.shape) != tuple(shape):
        raise ValueError("%s has shape %s where the rewards have %s" % (name, tuple(x.shape), tuple(shape)))
    return x


def _view(x):
    return _lr.View(x.data_ptr(), x.stride(1), x.stride(2), x.stride(0))


def _flag(x, name, reward):
    """A flag tensor as the kernel reads it -> (tensor, flag kind): bool and uint8 as bytes, the value dtype as it is."""
    x = _three(x, name, reward.shape)
    if x.device != reward.device:
        raise ValueError("%s is on %s, the rewards on %s" % (name, x.device, reward.device))
    if x.dtype == torch.bool:
        return x.view(torch.uint8), _lr.FLAG_U8
    if x.dtype == torch.uint8:
        return x, _lr.FLAG_U8
    if x.dtype == reward.dtype:
        return x, _lr.FLAG_VALUE
    raise ValueError("%s must be bool, uint8 or %s, got %s" % (name, reward.dtype, x.dtype))


def _value(x, name, reward):
    x = _three(x, name, reward.shape)
    if x.dtype != reward.dtype or x.device != reward.device:
        raise ValueError("%s must be a %s tensor on %s" % (name, reward.dtype, reward.device))
    return x


def _sizes(sizes, W, Bm, device):
    """None, a list of W block sizes or an int32 device tensor [W] -> (the device tensor or None, its pointer).  A list is
    uploaded once per (sizes, device) and kept for the life of the process (a few bytes each; never evicted, because a captured
    graph holds the tensor's address): a call under graph capture copies nothing.  A list without a single real environment is
    refused: there is nothing to take statistics or episode returns of."""
    if sizes is None:
        return None, None
    if isinstance(sizes, torch.Tensor):
        if sizes.dtype != torch.int32 or tuple(sizes.shape) != (W,) or sizes.device != device or not sizes.is_contiguous():
            raise ValueError("sizes must be a contiguous int32 tensor of shape (%d,) on %s" % (W, device))
        return sizes, sizes.data_ptr()
    key = (tuple(int(s) for s in sizes), device)
    if len(key[0]) != W or any(s < 0 or s > Bm for s in key[0]):
        raise ValueError("sizes %s does not describe %d blocks of at most %d environments" % (list(key[0]), W, Bm))
    if sum(key[0]) == 0:
        raise ValueError("sizes %s leaves no real environment" % (list(key[0]),))
    t = _sizes_cache.get(key)
    if t is None:
        t = _sizes_cache[key] = torch.tensor(key[0], dtype=torch.int32, device=device)
    return t, t.data_ptr()


def _shape(reward, flag_kind, sizes_ptr):
    if reward.device.type != 'cuda':
        raise ValueError("the kernels of libatacom_returns.so run on a GPU; got tensors on %s" % reward.device)
    if reward.dtype not in _DTYPES:
        raise ValueError("rewards must be float32 or float64, got %s" % reward.dtype)
    W, T, Bm = reward.shape
    return _lr.Shape(reward.device.index, _DTYPES[reward.dtype], flag_kind, T, Bm, W, sizes_ptr)


def _same_kind(a, b):
    if a != b:
        raise ValueError("absorbing and last must both be bool / uint8 or both have the rewards' dtype")
    return a


def _workspace(reward):
    W, _, Bm = reward.shape
    return torch.empty((_lr.workspace_doubles(W, Bm),), dtype=torch.float64, device=reward.device)


def compute_gae(reward, absorbing, last, v, v_next, gamma, lam, *, sizes=None, normalize=False, out=None):
    """MushroomRL's compute_gae with the critic already evaluated: v = V(obs), v_next = V(next_obs) (both None: zeros, which
    with lam = 1 is the discounted return-to-go).  -> (ret, adv), MushroomRL's order, shaped like `reward`; with
    normalize=True -> (ret, adv, stats): adv <- (adv - mean) / (std + 1e-8) over the real rows, stats = float64 device tensor
    [count, mean, std] (population std).  v_next is never read where absorbing is set.  `out` = (ret, adv), contiguous
    tensors of the rewards' shape and dtype that overlap no input and not each other (refused otherwise); with them (and `sizes` None, a device tensor, or a list seen before) the call
    allocates nothing but its small workspace and can be captured in a graph."""
    shape_in = reward.shape
    r = _three(reward, 'reward')
    ab, ka = _flag(absorbing, 'absorbing', r)
    la, kl = _flag(last, 'last', r)
    if (v is None) != (v_next is None):
        raise ValueError("v and v_next must both be given or both be None")
    keep, sizes_ptr = _sizes(sizes, r.shape[0], r.shape[2], r.device)
    a = _lr.new_args(_lr.GaeArgs)
    a.shape = _shape(r, _same_kind(ka, kl), sizes_ptr)
    a.gamma, a.lam, a.normalize = float(gamma), float(lam), int(bool(normalize))
    a.reward, a.absorbing, a.last = _view(r), _view(ab), _view(la)
    if v is not None:
        vv, vn = _value(v, 'v', r), _value(v_next, 'v_next', r)
        a.v, a.v_next = _view(vv), _view(vn)
    if out is None:
        ret, adv = torch.empty(shape_in, dtype=r.dtype, device=r.device), torch.empty(shape_in, dtype=r.dtype, device=r.device)
    else:
        ret, adv = out
        for t in (ret, adv):
            if tuple(t.shape) != tuple(shape_in) or t.dtype != r.dtype or t.device != r.device or not t.is_contiguous():
                raise ValueError("out must be two contiguous %s tensors of shape %s on %s" % (r.dtype, tuple(shape_in), r.device))
        # a lane loads several steps ahead of the step it stores: an output laid over an input (or over the other output) would
        # be read after it was written
        if overlap(ret, adv):
            raise ValueError("out must be two tensors that do not overlap")
        for name, x in (('reward', r), ('absorbing', ab), ('last', la), ('v', v), ('v_next', v_next)):
            if x is not None and (overlap(ret, x) or overlap(adv, x)):
                raise ValueError("out overlaps %s: the call does not work in place" % name)
    a.ret, a.adv = _view(_three(ret, 'out[0]')), _view(_three(adv, 'out[1]'))
    stats = ws = None
    if normalize:
        ws, stats = _workspace(r), torch.empty((3,), dtype=torch.float64, device=r.device)
        a.d_workspace, a.d_stats = ws.data_ptr(), stats.data_ptr()
    a.stream = stream(r.device.index)
    _lr.check(_lr.load().atacom_returns_gae(a))
    return (ret, adv, stats) if normalize else (ret, adv)


def normalize_advantages(adv, *, sizes=None):
    """adv <- (adv - mean) / (std + 1e-8) in place over the real rows (what compute_gae(normalize=True) runs after its
    recurrence) -> stats, the float64 device tensor [count, mean, std]."""
    x = _three(adv, 'adv')
    keep, sizes_ptr = _sizes(sizes, x.shape[0], x.shape[2], x.device)
    a = _lr.new_args(_lr.NormalizeArgs)
    a.shape = _shape(x, _lr.FLAG_U8, sizes_ptr)
    a.adv = _view(x)
    ws, stats = _workspace(x), torch.empty((3,), dtype=torch.float64, device=x.device)
    a.d_workspace, a.d_stats, a.stream = ws.data_ptr(), stats.data_ptr(), stream(x.device.index)
    _lr.check(_lr.load().atacom_returns_normalize(a))
    return stats


def episode_returns(reward, last, gamma=1.0, *, sizes=None):
    """The sums behind compute_J -> float64 device tensor [sum of j over the episodes, number of episodes, sum of j * j]; an
    episode ends at last[t] or at the end of the collection."""
    r = _three(reward, 'reward')
    la, kind = _flag(last, 'last', r)
    keep, sizes_ptr = _sizes(sizes, r.shape[0], r.shape[2], r.device)
    a = _lr.new_args(_lr.EpisodesArgs)
    a.shape = _shape(r, kind, sizes_ptr)
    a.gamma = float(gamma)
    a.reward, a.last = _view(r), _view(la)
    ws, res = _workspace(r), torch.empty((3,), dtype=torch.float64, device=r.device)
    a.d_workspace, a.d_result, a.stream = ws.data_ptr(), res.data_ptr(), stream(r.device.index)
    _lr.check(_lr.load().atacom_returns_episodes(a))
    return res


def compute_J(reward, last, gamma=1.0, *, sizes=None):
    """mean(mushroom_rl.utils.dataset.compute_J(dataset, gamma)) of the collection, the trailing unfinished episodes included
    -> (mean, n_episodes) as float64 device scalars.  gamma = 1 gives the reference's R, its MDP's gamma gives J."""
    s = episode_returns(reward, last, gamma, sizes=sizes)
    return s[0] / s[1], s[1]


def gae_from_records(layout, g, v, v_next, gamma, lam, *, normalize=False, out=None):
    """compute_gae on full packed records g [W, T, Bm, F] (or [T, Bm, F]) of `layout` (a RecordLayout): reward, absorbing and
    last are read as columns of g, in place; v, v_next [W, T, Bm] (or [T, Bm]) are the critic on its obs and next_obs columns.
    The padding rows of ragged shards are left out of the normalisation."""
    if g.shape[-1] != layout.F or g.dim() not in (3, 4):
        raise ValueError("full records must be [W, T, Bm, %d] or [T, Bm, %d], got %s" % (layout.F, layout.F, tuple(g.shape)))
    c = record_columns(g, {k: layout.fields[k] for k in ('reward', 'absorbing', 'last')})
    return compute_gae(c['reward'], c['absorbing'], c['last'], v, v_next, gamma, lam, sizes=_layout_sizes(layout, g),
                       normalize=normalize, out=out)


def _layout_sizes(layout, rec):
    """The layout's block sizes, for records of all its blocks; one block [T, Bm, F] of several has no rank to look its size up
    with, and every row of it counts."""
    return layout.sizes if rec.dim() == 4 or layout.world == 1 else None


def compact_v_next(layout, records, ends, n_ends, v, v_ends):
    """V(next_obs) of a compact collection without next_obs: v [W, T + 1, Bm] is the critic on the obs column of the records,
    tail row included, v_ends [W, M] the critic on the terminal observations ends[..., 2:].  v_next = v[:, 1:], then the valid
    exception rows overwrite their (t, b): CompactRecordLayout.unpack on one number per sample in place of D, with its bounds
    check and its indifference to shuffled, duplicate and superfluous rows.  -> [W, T, Bm] (one rank: [T, Bm])."""
    one = records.dim() == 3
    if one:
        records, v = records.unsqueeze(0), v.unsqueeze(0)
        ends = None if ends is None else ends.unsqueeze(0)
        v_ends = None if v_ends is None else v_ends.unsqueeze(0)
        n_ends = None if n_ends is None else [n_ends]
    T = layout.T
    if records.dim() != 4 or records.shape[1] != T + 1 or records.shape[3] != layout.Fc:
        raise ValueError("compact records must be [W, %d, Bm, %d], got %s" % (T + 1, layout.Fc, tuple(records.shape)))
    if tuple(v.shape) != tuple(records.shape[:3]):
        raise ValueError("v must be %s (the tail row included), got %s" % (tuple(records.shape[:3]), tuple(v.shape)))
    vn = v[:, 1:].clone()
    if ends is not None and ends.shape[1] > 0:
        W, M = ends.shape[0], ends.shape[1]
        if ends.shape[2] != layout.E:
            raise ValueError("exception rows must hold %d floats, got %d" % (layout.E, ends.shape[2]))
        if v_ends is None or tuple(v_ends.shape) != (W, M):
            raise ValueError("v_ends must be [%d, %d], one value per exception row" % (W, M))
        counts = [M] * W if n_ends is None else [int(c) for c in n_ends]
        if len(counts) != W or any(c < 0 or c > M for c in counts):
            raise ValueError("n_ends %s does not fit exception blocks of %d rows for %d ranks" % (counts, M, W))
        live = torch.arange(M, device=ends.device)[None, :] < torch.tensor(counts, device=ends.device)[:, None]
        rows = ends[live]
        rank = torch.arange(W, device=ends.device)[:, None].expand(W, M)[live]
        if rows.shape[0] > 0:
            t, b = rows[:, 0].long(), rows[:, 1].long()
            bad = (t < 0) | (t >= T) | (b < 0) | (b >= records.shape[2])
            if bool(bad.any()):
                raise ValueError("an exception row names a (t, b) outside the [%d, %d] records" % (T, records.shape[2]))
            vn[rank.to(vn.device), t.to(vn.device), b.to(vn.device)] = v_ends[live].to(vn.device)
    return vn[0] if one else vn


def gae_from_compact(layout, records, ends, n_ends, v, v_ends, gamma, lam, *, normalize=False, out=None):
    """compute_gae on a compact collection of `layout` (a CompactRecordLayout): records [W, T + 1, Bm, Fc], exception rows ends
    [W, M, D + 2] of which the first n_ends[r] of block r are valid (one rank: [T + 1, Bm, Fc], [M, D + 2], an int).  v
    [W, T + 1, Bm] is the critic on the records' obs column including the tail row, v_ends [W, M] the critic on ends[..., 2:]:
    the critic sees (T + 1) Bm + M rows per rank instead of 2 T Bm, and next_obs is never materialised (compact_v_next)."""
    vn = compact_v_next(layout, records, ends, n_ends, v, v_ends)
    body = records[..., :layout.T, :, :]
    c = record_columns(body, {k: layout.compact_fields[k] for k in ('reward', 'absorbing', 'last')})
    return compute_gae(c['reward'], c['absorbing'], c['last'], v[..., :layout.T, :], vn, gamma, lam,
                       sizes=_layout_sizes(layout, records), normalize=normalize, out=out)
