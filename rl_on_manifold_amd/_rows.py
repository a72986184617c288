"""What the learner-side modules (evaluate, fit, trust, offpolicy, offgrad, soft and, for the stream and the overlap test,
returns and optim) share on the host: a call over "the rows" of strided tensors.  The checks of such a call in one wording,
the collapse of leading dimensions to the (outer, inner) pair a kernel walks, `out=` reuse, the flat buffers with named views,
the ctypes struct of a network's tensors, and the common head and tail of an argument struct.  No numerics and no library of
its own: the callers pass their binding (a _lib_*.py module) where one is needed.

The order of the checks a caller makes with these: the tensor itself (rows_of), what the call is about, the rows of every
tensor (check_rows), the collapse (one_launch), idx, the outputs that are plain tensors and their overlap, n_blocks, and last
of what needs no device, needs_gpu.  What depends on the library's workspace size (reuse, the overlap of its buffers) follows.
"""
import torch

from ._binding import F32, F64
from ._device_env import _raw_stream
from ._lib_evaluate import View

DTYPES = {torch.float32: F32, torch.float64: F64}


def _current_stream(index):
    return torch.cuda.current_stream(torch.device('cuda', index)).cuda_stream


# stream(index): the current stream of GPU `index` as the integer a library takes -- PyTorch's raw accessor where it has one
# (no Python frame of ours per call), the public one otherwise
stream = _raw_stream if _raw_stream is not None else _current_stream


# ---------------------------------------------------------------------- checks
def rows_of(x, name):
    """`x`, the tensor that sets a call's device and dtype, is a float32 or float64 tensor [..., n] that holds at least one row
    -> its leading dimensions."""
    if not isinstance(x, torch.Tensor) or x.dim() < 1:
        raise ValueError("%s must be a tensor [..., n_in]" % name)
    if x.dtype not in DTYPES:
        raise ValueError("%s must be float32 or float64, got %s" % (name, x.dtype))
    lead = tuple(x.shape[:-1])
    if 0 in lead:
        raise ValueError("%s holds no rows: %s" % (name, tuple(x.shape)))
    return lead


def needs_gpu(x, lib_name):
    """The last check that needs no device: everything before it is about shapes and can be met on any machine."""
    if x.device.type != 'cuda':
        raise ValueError("the kernels of libatacom_%s.so run on a GPU; got tensors on %s" % (lib_name, x.device))


def check_rows(t, name, lead, width, ref):
    """`t` is [*lead, width] with contiguous rows, of the dtype and on the device of `ref`."""
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(lead) + (width,):
        raise ValueError("%s must be a tensor of shape %s, got %s" % (name, tuple(lead) + (width,),
                                                                      tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)))
    if t.dtype != ref.dtype or t.device != ref.device:
        raise ValueError("%s must be a %s tensor on %s, got %s on %s" % (name, ref.dtype, ref.device, t.dtype, t.device))
    if width > 1 and t.stride(-1) != 1:
        raise ValueError("the %d elements of a row of %s must be contiguous (stride %d)" % (width, name, t.stride(-1)))
    return t


def column(t):
    """[...] -> [..., 1]: one value per row as check_rows takes it; what is no tensor is left for check_rows to refuse."""
    return t.unsqueeze(-1) if isinstance(t, torch.Tensor) else t


def records_of(g, F, what):
    if not isinstance(g, torch.Tensor) or g.dim() not in (3, 4) or g.shape[-1] != F:
        raise ValueError("%s must be [W, T, Bm, %d] or [T, Bm, %d], got %s" % (what, F, F, tuple(getattr(g, 'shape', ()))))
    return g


def columns(layout, rec):
    """Full records [W, T, Bm, F] (or [T, Bm, F]) or compact records [W, T + 1, Bm, Fc] (or [T + 1, Bm, Fc]) of `layout`, whose
    tail row holds no action and is left out: obs and action sit at the same offsets in both."""
    Fc = getattr(layout, 'Fc', None)
    if isinstance(rec, torch.Tensor) and Fc is not None and rec.shape[-1] == Fc and rec.dim() in (3, 4):
        if rec.shape[-3] != layout.T + 1:
            raise ValueError("compact records must hold %d rows of time (the tail included), got %d" % (layout.T + 1, rec.shape[-3]))
        return rec[..., :layout.T, :, :]
    return records_of(rec, layout.F, 'records')


def launches(lead, strides):
    """The leading dimensions `lead` shared by several tensors with per-tensor `strides` -> [(offsets, n_outer, n_inner,
    [(stride_outer, stride_inner)])]: dimensions of size 1 dropped, neighbours that merge in every tensor merged, and what is
    still beyond two dimensions walked here, one launch per index."""
    dims = [(n, [s[j] for s in strides]) for j, n in enumerate(lead) if n != 1]
    merged = []
    for n, st in dims:
        if merged and all(a == n * b for a, b in zip(merged[-1][1], st)):
            merged[-1] = (merged[-1][0] * n, st)
        else:
            merged.append((n, st))
    out = []

    def walk(ds, offs):
        if len(ds) <= 2:
            ds = [(1, [0] * len(strides))] * (2 - len(ds)) + ds
            out.append((offs, ds[0][0], ds[1][0], list(zip(ds[0][1], ds[1][1]))))
            return
        for i in range(ds[0][0]):
            walk(ds[1:], [o + i * s for o, s in zip(offs, ds[0][1])])

    walk(merged, [0] * len(strides))
    return out


def one_launch(ts, names, lead, what=None):
    """The one launch of tensors that are gathered through idx or summed over: `what` ('a gradient', 'a product') cannot be
    split over launches."""
    found = launches(lead, [t.stride()[:-1] for t in ts])
    if len(found) != 1:
        raise ValueError("the leading dimensions %s of %s do not collapse to one (outer, inner) pair%s" % (
            tuple(lead), ', '.join(names), ": %s cannot be split over launches" % what if what else ""))
    return found[0]


def checked_idx(idx, x):
    """None, or flat row numbers: int64 [M >= 1], contiguous, on the device of x.  Their range is not looked at."""
    if idx is None:
        return None
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.dim() != 1 or idx.numel() < 1:
        raise ValueError("idx must be a one-dimensional int64 tensor of at least one row number")
    if idx.device != x.device or not idx.is_contiguous():
        raise ValueError("idx must be contiguous and on %s" % x.device)
    return idx


def n_rows(idx, launch):
    """The rows of a call: those idx names, or every row of the launch."""
    return idx.numel() if idx is not None else launch[1] * launch[2]


TARGET_ROWS = ('next_obs', 'reward', 'absorbing')


def target_rows(next_obs, reward, absorbing, lead, D, idx):
    """The row tensors of a TD target (TARGET_ROWS; a bool `absorbing` is converted to the dtype) -> (tensors, launch, idx, M)."""
    if isinstance(absorbing, torch.Tensor) and absorbing.dtype == torch.bool:
        absorbing = absorbing.to(next_obs.dtype)
    ts = [check_rows(next_obs, 'next_obs', lead, D, next_obs), check_rows(column(reward), 'reward', lead, 1, next_obs),
          check_rows(column(absorbing), 'absorbing', lead, 1, next_obs)]
    launch = one_launch(ts, TARGET_ROWS, lead)
    idx = checked_idx(idx, next_obs)
    return ts, launch, idx, n_rows(idx, launch)


def checked_blocks(n_blocks, max_blocks):
    """Whatever int() takes, in 0 .. max_blocks -> int."""
    if type(n_blocks) is int and 0 <= n_blocks <= max_blocks:
        return n_blocks
    try:
        n = int(n_blocks)
    except (TypeError, ValueError, OverflowError):
        n = -1
    if not 0 <= n <= max_blocks:
        raise ValueError("n_blocks must be 0 (the library chooses) or 1 .. %d, got %r" % (max_blocks, n_blocks))
    return n


def rows_out(t, name, M, width, x):
    """An output (or eps) of M rows of `width`: [M, width] (or [M] for width 1) with contiguous rows -> (tensor, row stride).
    None: a new one."""
    shape = (M, width) if width > 1 or (isinstance(t, torch.Tensor) and t.dim() == 2) else (M,)
    if t is None:
        t = torch.empty(shape, dtype=x.dtype, device=x.device)
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
        raise ValueError("%s must be a tensor of shape %s" % (name, shape))
    if t.dtype != x.dtype or t.device != x.device:
        raise ValueError("%s must be a %s tensor on %s" % (name, x.dtype, x.device))
    if t.dim() == 2 and width > 1 and t.stride(1) != 1:
        raise ValueError("the %d elements of a row of %s must be contiguous" % (width, name))
    return t, (t.stride(0) if M > 1 else width)


def optional_rows(a, into, x, M, specs):
    """For every (name, tensor, width) of `specs` whose tensor is given: rows_out, then a.<name> and a.<name>_stride; the
    (tensor, name) pairs join `into`, the list the overlap check reads."""
    for name, t, width in specs:
        if t is not None:
            t, stride = rows_out(t, name, M, width, x)
            setattr(a, name, t.data_ptr())
            setattr(a, name + '_stride', stride)
            into.append((t, name))


def bound(v, k, x, name):
    """A scalar, a sequence or a tensor -> [k] on the device of x in its dtype; a tensor already there is used as it is."""
    if isinstance(v, torch.Tensor) and v.device == x.device and v.dtype == x.dtype and tuple(v.shape) == (k,) and v.is_contiguous():
        return v
    t = torch.as_tensor(v, dtype=torch.float64).detach().reshape(-1)
    if t.numel() == 1:
        t = t.expand(k)
    if t.numel() != k:
        raise ValueError("%s: expected a scalar or %d values, got %d" % (name, k, t.numel()))
    return t.to(device=x.device, dtype=x.dtype).contiguous()


def extent(x):
    """[first byte, one past the last byte) of the memory a strided tensor touches."""
    lo = hi = 0
    for n, st in zip(x.shape, x.stride()):
        if n == 0:
            return x.data_ptr(), x.data_ptr()
        lo, hi = lo + min(0, (n - 1) * st), hi + max(0, (n - 1) * st)
    return x.data_ptr() + lo * x.element_size(), x.data_ptr() + (hi + 1) * x.element_size()


def overlap(a, b):
    (a0, a1), (b0, b1) = extent(a), extent(b)
    return a0 < b1 and b0 < a1


def inputs(ts, names, idx=None):
    """[(tensor, name)] of a call's row tensors and its idx, as no_overlap takes them."""
    return list(zip(ts, names)) + ([(idx, 'idx')] if idx is not None else [])


def buffers(out):
    """[(tensor, name)] of what a gradient call writes into its result."""
    return [(out.flat, 'out.flat'), (out.stats, 'out.stats'), (out.workspace, 'out.workspace')]


def no_overlap(outs, ins):
    """No output's extent meets that of an input or of another output; `outs` and `ins` are [(tensor, name)].  An object may
    stand in both lists (or twice among the outputs, a workspace two results share) and is not held against itself."""
    outs = [(t, name, extent(t)) for t, name in outs]
    rest = [(t, name, extent(t)) for t, name in ins] + outs
    for o, oname, (o0, o1) in outs:
        for t, name, (t0, t1) in rest:
            if t is not o and o0 < t1 and t0 < o1:
                raise ValueError("%s overlaps %s: the call does not work in place" % (oname, name))


# ---------------------------------------------------------------------- results
def carve(obj, flat, shapes):
    """Named views into one flat buffer: for every (name, shape) in order, obj.<name> = the next prod(shape) values of `flat`
    in that shape; a shape of None takes nothing and sets None."""
    o = 0
    for name, shape in shapes:
        if shape is None:
            setattr(obj, name, None)
            continue
        n = 1
        for s in shape:
            n *= s
        setattr(obj, name, flat[o:o + n].view(shape))
        o += n


def sized(L, need):
    """The bytes a library's workspace_size gave: 0 is its refusal, raised with the reason the library (binding `L`) keeps."""
    if need == 0:
        L.check(L.E_INVALID)
    return need


def reuse(outs, cls, key, need, describe):
    """The rule of `out=`: every result in `outs` (at least one) is a `cls` made by a call with the same `key`, and the workspace
    of the first holds the `need` bytes of this call.  `describe()` finishes "out must be the ..."."""
    if not outs or not all(isinstance(o, cls) and o.key == key for o in outs):
        raise ValueError("out must be the " + describe())
    have = outs[0].workspace.numel()
    if have < need:
        raise ValueError("out was made for fewer workgroups: its workspace holds %d bytes where this call needs %d" % (have, need))
    return outs


# ---------------------------------------------------------------------- argument structs
def network_struct(owner, shapes, struct_cls, device, dtype, keep='_keep'):
    """A ctypes struct with one pointer per tensor of owner.tensors: each moved to `device` in `dtype` -- a tensor already there
    is used as it is, so the call can be captured in a graph; the copies live in owner.<keep>, as long as the owner or until its
    next call -- and held to its shape in `shapes` = ((name, shape), ...) by name; None gives a null pointer."""
    device = torch.device(device)
    dev = {k: (None if v is None else torch.as_tensor(v).detach().to(device=device, dtype=dtype).contiguous())
           for k, v in owner.tensors.items()}
    setattr(owner, keep, dev)
    c = struct_cls()
    for name, shape in shapes:
        t = dev[name]
        if t is not None and tuple(t.shape) != shape:
            raise ValueError("%s has the shape %s where the critic needs %s" % (name, tuple(t.shape), shape))
        setattr(c, name, None if t is None else t.data_ptr())
    return c


def fill(a, x, n_blocks, launch, slots, ts, idx=None):
    """The head of an argument struct: device, dtype and n_blocks, the (outer, inner) pair of `launch`, a View per row tensor
    `ts` in the field `slots` names, and idx."""
    offs, a.n_outer, a.n_inner, strides = launch
    a.device, a.dtype, a.n_blocks = x.device.index, DTYPES[x.dtype], n_blocks
    size = x.element_size()
    for slot, t, off, (so, si) in zip(slots, ts, offs, strides):
        setattr(a, slot, View(t.data_ptr() + off * size, so, si))
    if idx is not None:
        a.idx, a.n_idx = idx.data_ptr(), idx.numel()


def run(a, fn, check, x, ws=None):
    """The tail of a call: the workspace, the current stream of x's device, and the checked call."""
    if ws is not None:
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    a.stream = stream(x.device.index)
    check(fn(a))


def critic_gradient(L, name, critics, dims, obs, action, target, idx, out, n_blocks, grads):
    """offgrad.critic_gradient and soft.soft_critic_gradient: the mean-squared TD error of one critic or a pair over the rows of
    obs [..., D] and action [..., k], target [M] per row of the call.  `L` is the binding of libatacom_<name>.so, `critics` a
    tuple the caller has checked, `dims` = (D, k); `grads` = (cls, key, sizes, make, struct, what) says what is written: the
    class of a result, its key without (dtype, device), the sizes atacom_<name>_workspace_size takes between the number of
    critics and the rows, make(n, bytes, key) -> n fresh results on one workspace, struct(critic, device, dtype) -> a critic's
    struct, `what` the words for a foreign `out`.  -> the tuple of results."""
    D, k = dims
    cls, key, sizes, make, struct, what = grads
    lead = rows_of(obs, 'obs')
    names = ('obs', 'action')
    ts = [check_rows(obs, 'obs', lead, D, obs), check_rows(action, 'action', lead, k, obs)]
    launch = one_launch(ts, names, lead)
    idx = checked_idx(idx, obs)
    M = n_rows(idx, launch)
    if not isinstance(target, torch.Tensor) or tuple(target.shape) != (M,):
        raise ValueError("target must be a tensor of shape (%d,): one value per row of the call" % M)
    if target.dtype != obs.dtype or target.device != obs.device:
        raise ValueError("target must be a %s tensor on %s" % (obs.dtype, obs.device))
    n_blocks = checked_blocks(n_blocks, L.MAX_BLOCKS)
    needs_gpu(obs, name)
    lib = L.load()
    need = sized(L, getattr(lib, 'atacom_%s_workspace_size' % name)(DTYPES[obs.dtype], len(critics), *sizes, M, n_blocks))
    key += (obs.dtype, obs.device)
    if out is None:
        outs = make(len(critics), need, key)
    else:
        outs = (out,) if isinstance(out, cls) else tuple(out)
        reuse(outs if len(outs) == len(critics) else (), cls, key, need, lambda: "%s in %s on %s" % (what, obs.dtype, obs.device))
    ws = outs[0].workspace
    bufs = [(ws, 'out.workspace')]
    for o, (flat, stats) in zip(outs, (('out[0].flat', 'out[0].stats'), ('out[1].flat', 'out[1].stats'))):
        bufs += [(o.flat, flat), (o.stats, stats)]
    no_overlap(bufs, inputs(ts, names, idx) + [(target, 'target')])
    a = L.new_args(L.CriticArgs)
    fill(a, obs, n_blocks, launch, names, ts, idx)
    a.n_critics = len(critics)
    for j, c in enumerate(critics):
        a.critics[j] = struct(c, obs.device, obs.dtype)
        a.grad[j], a.stats[j] = outs[j].flat.data_ptr(), outs[j].stats.data_ptr()
    a.target, a.target_stride = target.data_ptr(), (target.stride(0) if M > 1 else 1)
    run(a, getattr(lib, 'atacom_%s_critic_gradient' % name), L.check, obs, ws)
    return outs
