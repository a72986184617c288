"""The forward half of an off-policy update (DDPG, TD3) on the device -- the host side of libatacom_offpolicy.so
(include/atacom_offpolicy_hip.h states the arithmetic): a replay memory in the project's record format, the Q-value of the
reference's two-branch critic, the fused TD target  r + gamma (1 - absorbing) min_j Q'_j(s', clip(pi'(s') + clip(sigma eps)))
of a minibatch gathered through row numbers from the memory in place, and MushroomRL's soft target update, one launch each.
The critic and actor gradients are the other half, offgrad.py (libatacom_offgrad.so); ReplayMemory forwards to both.

Every call is enqueued on the current stream of the tensors' device and nothing synchronises.  With `out=` (and parameters
that already live on the device in the call's dtype) a call allocates nothing and can be captured in a graph.  Forward passes
only: nothing here is differentiable.  No numerics here, and no fall-back: a missing library is an error.
"""
import torch

from . import _lib_offpolicy as _lo
from ._rows import (DTYPES, TARGET_ROWS, bound, check_rows, checked_blocks, checked_idx, fill, inputs, n_rows, needs_gpu, network_struct,
                    no_overlap, one_launch, optional_rows, rows_of, rows_out, run, target_rows)
from .rollout import pack_fields, record_columns, record_fields

_KINDS = {'ddpg': _lo.DDPG, 'td3': _lo.TD3}


class QCritic:
    """Weights of the critic of the reference's DDPG and TD3 agents (examples/network.py: DDPGCriticNetwork,
    TD3CriticNetwork): q = W3 act(W2 act(W1 x1 + b1) + W2a (a / act_scale) + b2) + b3 with x1 the normalised observation
    (kind 'ddpg', W1 [64, D]) or [normalised observation | a / act_scale] (kind 'td3', W1 [64, D + k]); W2a [64, k] has no bias.
    `QCritic.from_module(net, obs_dim)` accepts any module with `_h1`, `_h2_s`, `_h2_a`, `_h3` and optionally
    `_action_scaling`, the attribute names of those two classes."""

    def __init__(self, W1, b1, W2, b2, W2a, W3, b3, kind, act_scale=None, obs_shift=None, obs_scale=None, activation='relu'):
        if kind not in _KINDS:
            raise ValueError("kind must be 'ddpg' or 'td3', got %r" % (kind,))
        self.tensors = dict(W1=W1, b1=b1, W2=W2, b2=b2, W2a=W2a, W3=W3, b3=b3, obs_shift=obs_shift, obs_scale=obs_scale,
                            act_scale=act_scale)
        self.kind = kind
        self.activation = {'relu': 0, 'tanh': 1}[activation]
        self.n_act = int(torch.as_tensor(W2a).shape[1])
        n1 = int(torch.as_tensor(W1).shape[1])
        self.n_obs = n1 - self.n_act if kind == 'td3' else n1
        if self.n_obs < 1:
            raise ValueError("a td3 critic's first layer takes the observation and the %d action elements, got %d inputs" % (self.n_act, n1))
        self._keep = None

    @classmethod
    def from_module(cls, net, obs_dim, obs_low=None, obs_high=None, activation='relu'):
        n1, k = net._h1.in_features, net._h2_a.in_features
        if n1 == obs_dim:
            kind = 'ddpg'
        elif n1 == obs_dim + k:
            kind = 'td3'
        else:
            raise ValueError("_h1 takes %d inputs where the observation has %d and the action %d elements" % (n1, obs_dim, k))
        shift = scale = None
        if obs_low is not None and obs_high is not None:          # MinMaxPreprocessor, as MlpPolicy.from_module forms it
            lo, hi = torch.as_tensor(obs_low, dtype=torch.float64), torch.as_tensor(obs_high, dtype=torch.float64)
            finite = torch.isfinite(lo) & torch.isfinite(hi)
            shift = torch.where(finite, (hi + lo) / 2, torch.zeros_like(lo))
            scale = torch.where(finite, 2.0 / (hi - lo).clamp_min(1e-12), torch.ones_like(lo))
        s = getattr(net, '_action_scaling', None)
        if s is not None:
            s = torch.as_tensor(s, dtype=torch.float64).detach().reshape(-1)
            s = (s.expand(k) if s.numel() == 1 else s).clone()
        if getattr(net._h2_a, 'bias', None) is not None:
            raise ValueError("_h2_a must be a Linear without bias")
        return cls(net._h1.weight.detach(), net._h1.bias.detach(), net._h2_s.weight.detach(), net._h2_s.bias.detach(),
                   net._h2_a.weight.detach(), net._h3.weight.detach(), net._h3.bias.detach(), kind=kind, act_scale=s,
                   obs_shift=shift, obs_scale=scale, activation=activation)

    def shapes(self):
        """((name, shape), ...) of the tensors, in the order of the library's struct."""
        D, k = self.n_obs, self.n_act
        return (('W1', (64, D + k if self.kind == 'td3' else D)), ('b1', (64,)), ('W2', (64, 64)), ('b2', (64,)), ('W2a', (64, k)),
                ('W3', (1, 64)), ('b3', (1,)), ('obs_shift', (D,)), ('obs_scale', (D,)), ('act_scale', (k,)))

    def as_struct_on(self, device, dtype):
        """The atacom_offpolicy_critic of this network on `device` in `dtype`.  Tensors that are already there are used as they
        are (no copy, so the call can be captured in a graph); the copies live as long as the critic or until the next call."""
        c = network_struct(self, self.shapes(), _lo.Critic, device, dtype)
        c.kind, c.n_obs, c.n_act, c.activation = _KINDS[self.kind], self.n_obs, self.n_act, self.activation
        return c


def q_values(critic, obs, action, *, idx=None, out=None, n_blocks=0):
    """Q(obs[row], action[row]) of a QCritic for obs [..., D] and action [..., k] sharing their leading dimensions (strided views
    with contiguous rows: the columns of a replay memory or of packed records, read in place) -> [M]: the rows idx[r] (flat row
    numbers, repeats allowed; the library does not guard one out of range), or every row in order without idx."""
    if not isinstance(critic, QCritic):
        raise ValueError("critic must be a QCritic")
    lead = rows_of(obs, 'obs')
    names = ('obs', 'action')
    ts = [check_rows(obs, 'obs', lead, critic.n_obs, obs), check_rows(action, 'action', lead, critic.n_act, obs)]
    launch = one_launch(ts, names, lead)
    idx = checked_idx(idx, obs)
    q, q_stride = rows_out(out, 'out', n_rows(idx, launch), 1, obs)
    no_overlap([(q, 'out')], inputs(ts, names))
    n_blocks = checked_blocks(n_blocks, _lo.MAX_BLOCKS)
    needs_gpu(obs, 'offpolicy')
    a = _lo.new_args(_lo.QArgs)
    fill(a, obs, n_blocks, launch, names, ts, idx)
    a.critic = critic.as_struct_on(obs.device, obs.dtype)
    a.q, a.q_stride = q.data_ptr(), q_stride
    run(a, _lo.load().atacom_offpolicy_q, _lo.check, obs)
    return q


def td_target(actor, critics, next_obs, reward, absorbing, gamma, *, eps=None, noise_std=0.0, noise_clip=0.0, low=None, high=None,
              idx=None, out=None, action_out=None, n_blocks=0):
    """The TD target of DDPG (one critic) or TD3 (a pair: the minimum of the two) in one launch, for next_obs [..., D], reward
    [...] and absorbing [...] (0.0 / 1.0 in the dtype; a bool tensor is converted) sharing their leading dimensions:

        a' = actor(next_obs)  (act_scale * tanh(.) for an actor of from_td3 / from_ddpg),   n = clamp(noise_std * eps, -+noise_clip)
        a'' = clamp(a' + n, low, high),   y = reward + gamma * ((1 - absorbing) * min_j Q_j(next_obs, a''))

    `actor` is an MlpPolicy (its exploration settings are not read), `critics` one QCritic or a pair, eps [M, k] standard normals
    of the caller (row r belongs to row r of the call, not to idx[r]; None: no noise), low / high the bounds of the action (both
    or neither).  -> y [M]; action_out [M, k], if given, receives a''."""
    lead = rows_of(next_obs, 'next_obs')
    critics = (critics,) if isinstance(critics, QCritic) else tuple(critics)
    if len(critics) not in (1, 2) or not all(isinstance(c, QCritic) for c in critics):
        raise ValueError("critics must be one QCritic or a pair of them")
    c0 = critics[0]
    if any((c.kind, c.n_obs, c.n_act) != (c0.kind, c0.n_obs, c0.n_act) for c in critics):
        raise ValueError("the two critics differ in kind, observation or action size")
    if (low is None) != (high is None):
        raise ValueError("low and high are given together or not at all")
    for name, v in (('noise_std', noise_std), ('noise_clip', noise_clip)):
        if not float(v) >= 0.0 or float(v) == float('inf'):
            raise ValueError("%s must be >= 0 and finite, got %r" % (name, v))
    if float(gamma) != float(gamma) or abs(float(gamma)) == float('inf'):
        raise ValueError("gamma must be finite, got %r" % (gamma,))
    D, k = c0.n_obs, c0.n_act
    ts, launch, idx, M = target_rows(next_obs, reward, absorbing, lead, D, idx)
    m = actor.as_struct_on(next_obs.device, next_obs.dtype)
    if (m.n_in, m.n_out) != (D, k):
        raise ValueError("the actor maps %d to %d where the critics take %d observation and %d action elements" % (m.n_in, m.n_out, D, k))
    a = _lo.new_args(_lo.TargetArgs)
    y, a.y_stride = rows_out(out, 'out', M, 1, next_obs)
    ins, outs = inputs(ts, TARGET_ROWS), [(y, 'out')]
    optional_rows(a, ins, next_obs, M, [('eps', eps, k)])
    optional_rows(a, outs, next_obs, M, [('action_out', action_out, k)])
    no_overlap(outs, ins)
    if low is not None:
        keep = [bound(low, k, next_obs, 'low'), bound(high, k, next_obs, 'high')]
        a.act_low, a.act_high = keep[0].data_ptr(), keep[1].data_ptr()
    n_blocks = checked_blocks(n_blocks, _lo.MAX_BLOCKS)
    needs_gpu(next_obs, 'offpolicy')
    fill(a, next_obs, n_blocks, launch, TARGET_ROWS, ts, idx)
    a.n_critics, a.actor = len(critics), m
    for j, c in enumerate(critics):
        a.critics[j] = c.as_struct_on(next_obs.device, next_obs.dtype)
    a.noise_std, a.noise_clip, a.gamma, a.y = float(noise_std), float(noise_clip), float(gamma), y.data_ptr()
    run(a, _lo.load().atacom_offpolicy_target, _lo.check, next_obs)
    return y


def _pair_tensors(obj):
    """(tensors in the library's order, n_in, n_out, n_act) of an MlpPolicy, a QCritic or a tuple of 6 or 7 tensors
    (W1, b1, W2, b2, W3, b3[, W2a])."""
    if isinstance(obj, QCritic):
        ts = [obj.tensors[k] for k in _lo.PARAMS]
    elif hasattr(obj, 'tensors'):
        ts = [obj.tensors[k] for k in _lo.PARAMS[:6]]
    else:
        ts = list(obj)
    if len(ts) not in (6, 7) or not all(isinstance(t, torch.Tensor) for t in ts):
        raise ValueError("a parameter set is an MlpPolicy, a QCritic or 6 or 7 tensors (W1, b1, W2, b2, W3, b3[, W2a])")
    n_in, n_out, n_act = ts[0].shape[1], ts[4].shape[0], (ts[6].shape[1] if len(ts) == 7 else 0)
    shapes = [(64, n_in), (64,), (64, 64), (64,), (n_out, 64), (n_out,), (64, n_act)]
    for t, s, name in zip(ts, shapes, _lo.PARAMS):
        if tuple(t.shape) != s:
            raise ValueError("%s has the shape %s where %s is expected" % (name, tuple(t.shape), s))
    return ts, n_in, n_out, n_act


def soft_update(targets, onlines, tau):
    """MushroomRL's _update_target, target = tau * online + (1 - tau) * target, for up to four (target, online) pairs in one
    launch: MlpPolicy / QCritic objects or tuples of tensors, whose tensors live on one GPU in one dtype and are contiguous.  The
    targets are updated in place; the online tensors are only read."""
    if isinstance(targets, QCritic) or hasattr(targets, 'tensors') or (len(targets) and isinstance(targets[0], torch.Tensor)):
        targets, onlines = [targets], [onlines]
    if len(targets) != len(onlines) or not 1 <= len(targets) <= _lo.MAX_PAIRS:
        raise ValueError("soft_update takes 1 to %d pairs, got %d targets and %d online sets" % (_lo.MAX_PAIRS, len(targets), len(onlines)))
    if not 0.0 <= float(tau) <= 1.0:
        raise ValueError("tau must be in [0, 1], got %r" % (tau,))
    a = _lo.new_args(_lo.SoftUpdateArgs)
    ref = None
    for j, (tg, on) in enumerate(zip(targets, onlines)):
        (tt, *shape_t), (ot, *shape_o) = _pair_tensors(tg), _pair_tensors(on)
        if shape_t != shape_o:
            raise ValueError("pair %d: the target and the online set differ in shape" % j)
        for t in tt + ot:
            ref = t if ref is None else ref
            if t.dtype not in DTYPES or t.dtype != ref.dtype or t.device != ref.device or not t.is_contiguous():
                raise ValueError("the tensors of a soft update are contiguous, on one device and all float32 or all float64")
        p = a.pairs[j]
        p.n_in, p.n_out, p.n_act = shape_t
        for i, (t, o) in enumerate(zip(tt, ot)):
            p.target[i], p.online[i] = t.data_ptr(), o.data_ptr()
    needs_gpu(ref, 'offpolicy')
    a.device, a.dtype, a.n_pairs, a.tau = ref.device.index, DTYPES[ref.dtype], len(targets), float(tau)
    run(a, _lo.load().atacom_offpolicy_soft_update, _lo.check, ref)


class ReplayMemory:
    """A ring of `capacity` transitions in the full record format [obs | action | reward | next_obs | absorbing | last]
    (rollout.record_fields; F = 2 D + k + 3) on the device: `storage` [capacity, F].  Row j = t B + b of a collection goes to
    slot (head + j) mod capacity; of a collection longer than the capacity only the last `capacity` rows are written, so no slot is
    written twice.  `head` and `size` are host integers that depend on shapes alone: nothing here synchronises.  Adding is torch
    indexing (a copy); the kernels read the storage's columns in place."""

    def __init__(self, capacity, obs_dim, n_null, dtype=torch.float32, device='cuda'):
        if int(capacity) < 1:
            raise ValueError("capacity must be >= 1")
        self.capacity, self.D, self.k = int(capacity), int(obs_dim), int(n_null)
        self.fields, self.F = record_fields(self.D, self.k)
        self.storage = torch.zeros((self.capacity, self.F), dtype=dtype, device=device)
        self.head, self.size = 0, 0

    def initialized(self, initial_size):
        return self.size >= int(initial_size)

    def _same_device(self, what, *tensors):
        for t in tensors:
            if isinstance(t, torch.Tensor) and t.device != self.storage.device:
                raise ValueError("%s live on %s, the memory's storage on %s: move them first" % (what, t.device, self.storage.device))

    def _write(self, rows):
        n, cap = rows.shape[0], self.capacity
        j0 = max(0, n - cap)
        start, m = (self.head + j0) % cap, n - j0
        first = min(m, cap - start)
        self.storage[start:start + first] = rows[j0:j0 + first]
        if m > first:
            self.storage[:m - first] = rows[j0 + first:]
        self.head, self.size = (self.head + n) % cap, min(self.size + n, cap)

    def add(self, layout, rec):
        """Full packed records [T, Bm, F] of one rank or gathered [W, T, Bm, F] of `layout` (a RecordLayout); the padding rows of
        ragged shards are skipped and the ranks' environments follow each other as in RecordLayout.time_major."""
        if not isinstance(rec, torch.Tensor) or rec.dim() not in (3, 4) or rec.shape[-1] != self.F or layout.F != self.F:
            raise ValueError("records must be [W, T, Bm, %d] or [T, Bm, %d]" % (self.F, self.F))
        self._same_device("the records", rec)
        rec = rec.unsqueeze(0) if rec.dim() == 3 else rec
        if rec.shape[0] != layout.world or rec.shape[2] < max(layout.sizes):
            raise ValueError("records %s do not fit the layout's %d ranks of up to %d environments" % (tuple(rec.shape), layout.world, layout.Bm))
        rows = torch.cat([rec[r, :, :layout.sizes[r]] for r in range(layout.world)], 1).reshape(-1, self.F)
        self._write(rows.to(self.storage.dtype))

    def add_compact(self, layout, records, ends=None, n_ends=None):
        """Compact records [T + 1, Bm, Fc] or [W, T + 1, Bm, Fc] of `layout` (a CompactRecordLayout) with their exception rows:
        next_obs is rebuilt the way CompactRecordLayout.unpack does it."""
        self._same_device("the compact records and their exception rows", records, ends)
        d = layout.unpack(records, ends, n_ends)
        full = torch.empty(tuple(d['reward'].shape) + (self.F,), dtype=records.dtype, device=records.device)
        pack_fields(full, self.fields, [d[name] for name in self.fields])
        self.add(layout, full)

    def add_fields(self, obs, action, reward, next_obs, absorbing, last):
        """Plain tensors: obs, next_obs [..., D], action [..., k], reward, absorbing, last [...] (flags of any dtype)."""
        self._same_device("the fields", obs, action, reward, next_obs, absorbing, last)
        lead = tuple(reward.shape)
        full = torch.empty(lead + (self.F,), dtype=self.storage.dtype, device=self.storage.device)
        pack_fields(full, self.fields, [obs, action, reward, next_obs, absorbing, last])
        self._write(full.reshape(-1, self.F))

    def sample(self, n, generator=None):
        """n int64 row numbers on the device, uniform over [0, size) with replacement (MushroomRL's ReplayMemory.get)."""
        if self.size < 1:
            raise ValueError("the memory is empty")
        return torch.randint(0, self.size, (int(n),), device=self.storage.device, generator=generator, dtype=torch.int64)

    def columns(self, idx=None):
        """The six fields for torch code, flags in the storage's dtype: views of the filled rows without idx, gathered copies
        with it."""
        return record_columns(self.storage[:self.size] if idx is None else self.storage[idx], self.fields)

    def q_values(self, critic, idx, **kw):
        """q_values on the obs and action columns of the storage, in place."""
        c = record_columns(self.storage, self.fields)
        return q_values(critic, c['obs'], c['action'], idx=idx, **kw)

    def td_target(self, actor, critics, idx, gamma, **kw):
        """td_target on the next_obs, reward and absorbing columns of the storage, in place."""
        c = record_columns(self.storage, self.fields)
        return td_target(actor, critics, c['next_obs'], c['reward'], c['absorbing'], gamma, idx=idx, **kw)

    def critic_gradient(self, critics, idx, target, **kw):
        """offgrad.critic_gradient on the obs and action columns of the storage, in place; target [M] is row r of the call."""
        from .offgrad import critic_gradient
        c = record_columns(self.storage, self.fields)
        return critic_gradient(critics, c['obs'], c['action'], target, idx=idx, **kw)

    def actor_gradient(self, actor, critic, idx, **kw):
        """offgrad.actor_gradient on the obs column of the storage, in place."""
        from .offgrad import actor_gradient
        c = record_columns(self.storage, self.fields)
        return actor_gradient(actor, critic, c['obs'], idx=idx, **kw)

    def soft_td_target(self, policy, critics, idx, gamma, log_alpha, eps, **kw):
        """soft.soft_td_target on the next_obs, reward and absorbing columns of the storage, in place."""
        from .soft import soft_td_target
        c = record_columns(self.storage, self.fields)
        return soft_td_target(policy, critics, c['next_obs'], c['reward'], c['absorbing'], gamma, log_alpha, eps, idx=idx, **kw)

    def soft_critic_gradient(self, critics, idx, target, **kw):
        """soft.soft_critic_gradient on the obs and action columns of the storage, in place; target [M] is row r of the call."""
        from .soft import soft_critic_gradient
        c = record_columns(self.storage, self.fields)
        return soft_critic_gradient(critics, c['obs'], c['action'], target, idx=idx, **kw)

    def soft_actor_gradient(self, policy, critics, idx, eps, log_alpha, target_entropy, **kw):
        """soft.soft_actor_gradient on the obs column of the storage, in place."""
        from .soft import soft_actor_gradient
        c = record_columns(self.storage, self.fields)
        return soft_actor_gradient(policy, critics, c['obs'], eps, log_alpha, target_entropy, idx=idx, **kw)
