"""Sharded on-policy rollout collection: one process per GPU, the env batch split into contiguous blocks,
NO collective while stepping (environments are independent), and ONE all-gather of the finished rollout
buffer per collection phase (RCCL over xGMI on the GPU box: `torch.distributed` backend "nccl"; the same code
runs on "gloo" for the CPU tests).

The reference has no distributed code at all; this is the data-parallel axis the
workload offers: BASELINE.json config 5 = 65536 IiwaAirHockey envs = 8 GPUs x 8192.

Data path of one collection (every pass over the data is listed; there are two):
  1. the rollout kernel writes the (state, action, reward, next_state, absorbing, last) tuples mushroom_rl.Core.learn
     hands to an on-policy agent as packed float records [T, B_shard, F] (atacom_rollout_packed, one launch);
  2. one `all_gather_into_tensor` of that buffer into [W, T, B_shard, F] -- which IS the final layout
     ("shard-major"): `unpack` returns views into it, `reshape(-1, F)` is the flat sample set a PPO / TRPO fit
     consumes, and the time axis of every environment stays strided-contiguous for GAE.
No size exchange (every rank's shard size is a pure function of (global_batch, world)), no packing copy, no
concatenation.  Ragged shards (global_batch not a multiple of the world size) are padded to the largest shard: block r
of the gathered buffer holds sizes[r] valid env rows followed by ZERO rows, so `reshape(-1, F)` of a ragged gather also
contains those padding records -- `RecordLayout.valid_mask()` selects the real ones, `time_major()` drops them.  For config 5: 120 x 8192 x 44 floats = 173 MB sent per rank, 1.38 GB received; xGMI is
point-to-point, so one large collective amortises the per-link setup far better than six small ones.
Constraint statistics are reduced with one MAX and one SUM all-reduce of two numbers each.

Compact format (RolloutCollector(record_format='compact'), opt-in): next_obs is the next record's obs except where an
auto-reset came between, so the kernel (atacom_rollout_compact) writes records [T + 1, Bm, D + k + 3] -- the full record
minus next_obs, plus a tail row holding the observation after the last step -- and appends one row [t, b, terminal obs] per
episode end before the last step.  The gather is then ONE all-gather of the W exception counts (this reads the count back:
one stream synchronisation per collection) and ONE all-gather of each rank's flat segment, records followed by max(count)
exception rows.  CompactRecordLayout.unpack rebuilds the dataset the full format returns, bit for bit; next_obs is
materialised (one copy of the obs slice), every other field stays a view.  For config 5: 121 x 8192 x 26 floats = 103 MB
plus 80 bytes per exception row sent per rank, instead of 173 MB.
"""
import torch
import torch.distributed as dist


def shard_bounds(global_batch, world_size, rank):
    """Contiguous block [lo, hi) of the global env index range owned by `rank` (remainder to the low ranks)."""
    base, rem = divmod(int(global_batch), int(world_size))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def record_fields(D, k):
    """(fields, F): where each field of the full packed record [obs | action | reward | next_obs | absorbing | last] sits --
    a slice or an index into the last axis, listed in record order -- and the record's length F = 2 D + k + 3.  Order and
    widths are the ABI of `Record<E>` (and, below, of `RecordCompact<E>`) in csrc/atacom_kernels.h: this is the one place
    the Python side spells them out."""
    o = D + k
    return {'obs': slice(0, D), 'action': slice(D, o), 'reward': o, 'next_obs': slice(o + 1, o + 1 + D),
            'absorbing': o + 1 + D, 'last': o + 2 + D}, 2 * D + k + 3


def compact_record_fields(D, k):
    """(fields, Fc, E) of the compact format: the record [obs | action | reward | absorbing | last] of Fc = D + k + 3 floats
    and the length E = D + 2 of an exception row [t, b, terminal obs]."""
    o = D + k
    return {'obs': slice(0, D), 'action': slice(D, o), 'reward': o, 'absorbing': o + 1, 'last': o + 2}, o + 3, D + 2


def unpack_fields(rec, fields):
    """Views (no copy) of `fields` into records [..., F]; the two flags as bool."""
    out = {name: rec[..., ix] for name, ix in fields.items()}
    out['absorbing'], out['last'] = out['absorbing'] > 0.5, out['last'] > 0.5
    return out


def record_columns(rec, fields):
    """Views (no copy) of `fields` into records [..., F] as they are stored: the two flags keep the records' dtype (0.0 / 1.0)
    and their stride, which is how the kernels of returns.py read them in place."""
    return {name: rec[..., ix] for name, ix in fields.items()}


def pack_fields(rec, fields, values):
    """Write `values` (one array per field, in record order; flags of any dtype) into the fields of rec [..., F]."""
    for ix, v in zip(fields.values(), values):
        rec[..., ix] = v.to(rec.dtype)


class RecordLayout:
    """The shard-major layout of a gathered collection, [W, T, Bm, F] with F = 2 D + k + 3 packed floats per (step, env):
    [obs | action | reward | next_obs | absorbing | last].  Pure index arithmetic -- usable without a process group
    (e.g. for a buffer that several engines of ONE process filled block by block)."""

    def __init__(self, sizes, obs_dim, n_null):
        self.sizes = [int(s) for s in sizes]
        self.world = len(self.sizes)
        self.Bm = max(self.sizes)
        self.D, self.k = int(obs_dim), int(n_null)
        self.fields, self.F = record_fields(self.D, self.k)

    def unpack(self, g):
        """Views (no copy) into records [..., F]."""
        return unpack_fields(g, self.fields)

    def time_major(self, data):
        """[W, T, Bm, ...] -> [T, B_global, ...] with rank r's envs in block shard_bounds(global_batch, W, r); the
        padding rows of ragged shards are dropped.  This one COPIES (a permute + concatenation)."""
        return {key: torch.cat([v[r, :, :self.sizes[r]] for r in range(self.world)], 1) for key, v in data.items()}

    def valid_mask(self, device=None):
        """bool [W, Bm]: True where block r, env row b is a real environment (False on the padding of ragged shards)."""
        idx = torch.arange(self.Bm, device=device)
        return idx[None, :] < torch.tensor(self.sizes, device=device)[:, None]


class CompactRecordLayout(RecordLayout):
    """The compact record format (BatchedAtacomEnv.rollout_compact, include/atacom_hip.h: atacom_rollout_compact) of a
    collection of T = n_steps steps: per rank, records [T + 1, Bm, Fc] with Fc = D + k + 3 --
    rows 0..T-1 [obs | action | reward | absorbing | last], row T the tail [obs after step T-1 | zeros] -- and a list of
    exception rows [t, b, terminal obs] (D + 2 floats) for the episode ends at t < T-1 of auto-resetting engines.
    `unpack` rebuilds exactly what RecordLayout.unpack returns for the full format.  time_major / valid_mask as there."""

    def __init__(self, sizes, obs_dim, n_null, n_steps):
        super().__init__(sizes, obs_dim, n_null)
        self.T = int(n_steps)
        self.compact_fields, self.Fc, self.E = compact_record_fields(self.D, self.k)   # E: floats per exception row
        self.record_numel = (self.T + 1) * self.Bm * self.Fc  # elements of one rank's records

    def unpack(self, records, ends=None, n_ends=None):
        """records [W, T + 1, Bm, Fc] (or [T + 1, Bm, Fc] for one rank), ends [W, M, D + 2] (or [M, D + 2]) of which the
        first n_ends[r] rows of block r are valid (None: all M) -> the dict of RecordLayout.unpack, [W, T, Bm, ...] (or
        [T, Bm, ...]).  Every field but next_obs is a view; next_obs is materialised: next_obs[t] = obs[t + 1],
        next_obs[T-1] = the tail, then each exception row overwrites its (t, b).  The order of the exception rows does not
        matter, and a superset of the necessary rows (any rows of last = 1) gives the same result."""
        one = records.dim() == 3
        if one:
            records = records.unsqueeze(0)
            ends = None if ends is None else ends.unsqueeze(0)
            n_ends = None if n_ends is None else [n_ends]
        T = self.T
        if records.dim() != 4 or records.shape[1] != T + 1 or records.shape[3] != self.Fc:
            raise ValueError("compact records must be [W, %d, Bm, %d], got %s" % (T + 1, self.Fc, tuple(records.shape)))
        body = records[:, :T]
        # obs of the next step; the tail row closes the last step
        nobs = records[:, 1:][..., self.compact_fields['obs']].clone()
        if ends is not None and ends.shape[1] > 0:
            W, M = ends.shape[0], ends.shape[1]
            if ends.shape[2] != self.E:
                raise ValueError("exception rows must hold %d floats, got %d" % (self.E, ends.shape[2]))
            counts = [M] * W if n_ends is None else [int(c) for c in n_ends]
            if len(counts) != W or any(c < 0 or c > M for c in counts):
                raise ValueError("n_ends %s does not fit exception blocks of %d rows for %d ranks" % (counts, M, W))
            live = torch.arange(M, device=ends.device)[None, :] < torch.tensor(counts, device=ends.device)[:, None]
            rows = ends[live]                                 # [N, D + 2], block by block
            rank = torch.arange(W, device=ends.device)[:, None].expand(W, M)[live]
            if rows.shape[0] > 0:
                t, b = rows[:, 0].long(), rows[:, 1].long()
                bad = (t < 0) | (t >= T) | (b < 0) | (b >= records.shape[2])
                if bool(bad.any()):
                    raise ValueError("an exception row names a (t, b) outside the [%d, %d] records" % (T, records.shape[2]))
                nobs[rank.to(nobs.device), t.to(nobs.device), b.to(nobs.device)] = rows[:, 2:].to(nobs.device)
        out = unpack_fields(body, self.compact_fields)
        out = {name: nobs if name == 'next_obs' else out[name] for name in self.fields}      # the full format's order
        return {key: v[0] for key, v in out.items()} if one else out


class CompactShard:
    """One rank's compact collection (RolloutCollector with record_format='compact'): `records` [T + 1, Bm, Fc] and `ends`
    [capacity, D + 2] are views into ONE flat buffer, records first, so that the records and the first rows of the exception
    list form a contiguous send segment; the first `n_ends` rows of `ends` are valid."""

    def __init__(self, flat, layout, capacity, n_ends=0):
        self.flat, self.layout, self.capacity, self.n_ends = flat, layout, int(capacity), int(n_ends)
        lay = layout
        self.records = flat[:lay.record_numel].view(lay.T + 1, lay.Bm, lay.Fc)
        self.ends = flat[lay.record_numel:lay.record_numel + self.capacity * lay.E].view(self.capacity, lay.E)


class CompactGather:
    """A gathered compact collection: `flat` [W, L] holds every rank's records followed by max(n_ends) exception rows (those
    past a rank's own count are zero); `n_ends` lists the valid rows per rank."""

    def __init__(self, flat, layout, n_ends):
        self.flat, self.layout, self.n_ends = flat, layout, list(n_ends)

    def unpack(self):
        lay, W = self.layout, self.flat.shape[0]
        M = max(self.n_ends) if self.n_ends else 0
        rec = self.flat[:, :lay.record_numel].view(W, lay.T + 1, lay.Bm, lay.Fc)
        ends = self.flat[:, lay.record_numel:lay.record_numel + M * lay.E].view(W, M, lay.E)
        return lay.unpack(rec, ends, self.n_ends)


class RolloutCollector:
    """Drive one local engine (a BatchedAtacomEnv, or anything with its surface) and assemble global rollouts.

    env          : local engine holding this rank's shard (env.batch envs)
    group        : torch.distributed process group (None = default group; no-op if dist is not initialised)
    global_batch : total number of envs over all ranks (default env.batch * world, i.e. equal shards); ragged
                   shards follow shard_bounds(global_batch, world, rank) and are padded to the largest shard
    record_format: 'full' (default) -- the packed records [T, Bm, 2 D + k + 3] all-gathered as they are; 'compact' -- records
                   without next_obs plus the exception rows of the episode ends (CompactRecordLayout): D fewer floats per
                   record sent, the same dataset returned.  Compact costs one stream synchronisation per collection (the
                   exception counts are exchanged before the records): when collect_async returns, the rollout kernel has
                   finished.
    """

    def __init__(self, env, group=None, global_batch=None, force_collective=False, record_format='full'):
        if record_format not in ('full', 'compact'):
            raise ValueError("record_format must be 'full' or 'compact', got %r" % (record_format,))
        self.record_format = record_format
        self.last_gather_bytes = 0                # payload one rank sent in the last gather (its send buffer)
        self.env = env
        self.group = group
        # force_collective: run the collectives even in a world of one rank (they are a copy through the backend then):
        # the way to exercise the RCCL transport -- buffer registration, the backend's stream, async work objects -- on a
        # single GPU.  Needs an initialised process group.
        self.force_collective = bool(force_collective)
        self.distributed = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if self.distributed else 1
        self.rank = dist.get_rank(group) if self.distributed else 0
        self.global_batch = int(global_batch) if global_batch is not None else env.batch * self.world
        self.sizes = []
        for r in range(self.world):
            lo, hi = shard_bounds(self.global_batch, self.world, r)
            self.sizes.append(hi - lo)
        if self.sizes[self.rank] != env.batch:
            raise ValueError("rank %d holds %d envs, shard_bounds(%d, %d) assigns it %d"
                             % (self.rank, env.batch, self.global_batch, self.world, self.sizes[self.rank]))
        self.Bm = max(self.sizes)                 # env-axis length of every rank's send buffer
        self.k = env.dims['null']
        self.D = env.obs_dim
        self.layout = RecordLayout(self.sizes, self.D, self.k)
        self.F = self.layout.F                    # obs, action, reward, next_obs, absorbing, last
        self.Fc = compact_record_fields(self.D, self.k)[1]   # the compact record: the same minus next_obs
        self._recv = None
        self._recv_flat = None
        self.mappings = self._agree_on_mappings()

    def _agree_on_mappings(self):
        """The kernel mappings (lanes per environment of step() and of the T-step kernels) sum in different orders, so
        ranks that hold equally sized shards must run the SAME mappings or a sharded collection is not reproducible
        against a single-process run of the same batch size per rank.  The library's policy is static (a pure function of
        the configuration, include/atacom_hip.h), so this can only fail when a rank was configured differently
        (lanes_per_env, ATACOM_CALIBRATE=1): checked ONCE here, at construction -- one all-gather of three integers,
        never in the data path -- and refused loudly.  Returns [(batch, step_lanes, rollout_lanes)] per rank."""
        mine = self._my_mappings()
        self._agreed = tuple(mine)
        if self.world == 1:
            return [tuple(mine)]
        dev = getattr(self.env, 'device', torch.device('cpu'))
        if dist.get_backend(self.group) == 'gloo':
            dev = torch.device('cpu')
        t = torch.tensor(mine, dtype=torch.int64, device=dev)
        allm = torch.empty((self.world * 3,), dtype=torch.int64, device=dev)     # the concatenated form every backend takes
        dist.all_gather_into_tensor(allm, t, group=self.group)
        rows = [tuple(int(v) for v in r) for r in allm.cpu().view(self.world, 3)]
        by_batch = {}
        for r, (b, sl, rl) in enumerate(rows):
            first = by_batch.setdefault(b, (r, sl, rl))
            if (sl, rl) != first[1:]:
                raise ValueError("ranks %d and %d hold shards of %d environments but run different kernel mappings "
                                 "(step %d / rollout %d lanes per environment against %d / %d): name lanes_per_env on "
                                 "every rank (and leave ATACOM_CALIBRATE unset) -- the bits depend on the mapping"
                                 % (first[0], r, b, first[1], first[2], sl, rl))
        return rows

    def _my_mappings(self):
        return [int(self.env.batch), int(getattr(self.env, 'lanes_per_env', 0)),
                int(getattr(self.env, 'rollout_lanes_per_env', 0))]

    def _check_mappings_unchanged(self):
        """A snapshot restore can make a handle ADOPT the image writer's kernel mappings (include/atacom_hip.h:
        atacom_snapshot_restore).  The agreement above was reached at construction: a rank whose mappings have changed since
        refuses to collect -- locally, no collective -- until a new collector is built (on every rank)."""
        now = tuple(self._my_mappings())
        if now != self._agreed:
            raise ValueError("this rank's kernel mappings changed after the collector was built (batch, step, rollout lanes "
                             "%s -> %s; a snapshot restore adopts the image's mappings): build a new RolloutCollector on every "
                             "rank" % (self._agreed, now))

    # ------------------------------------------------------------------ local collection
    def collect_local(self, n_steps, actions=None, policy=None, noise=None, out=None):
        """T = n_steps env steps of the local shard -> packed records [T, Bm, F] (record_format 'full') or a CompactShard
        (record_format 'compact'; `out` is then a flat contiguous buffer of at least compact_numel(T) elements).
        actions [T, B_local, k]  : pre-generated actions, ONE kernel launch;
        policy = MlpPolicy       : the actor network evaluated inside the rollout kernel, ONE launch (`noise` optional);
        policy = callable        : policy(obs) -> actions, one launch per step (host-driven loop)."""
        env = self.env
        self._check_mappings_unchanged()
        if self.record_format == 'compact':
            return self._collect_local_compact(n_steps, actions, policy, noise, out)
        fused = hasattr(env, 'rollout_packed')
        if fused and actions is not None:
            return env.rollout_packed(actions=actions, out=out, batch_stride=self.Bm)
        if fused and policy is not None and hasattr(policy, 'as_struct'):
            return env.rollout_packed(policy=policy, n_steps=n_steps, noise=noise, out=out, batch_stride=self.Bm)
        # engines without the packed kernel (the CPU test double) and host-side policies: pack here
        B = env.batch
        rollout = self._host_rollout(n_steps, actions, policy)
        obs = rollout[0]
        T = obs.shape[0]
        buf = torch.zeros((T, self.Bm, self.F), device=obs.device, dtype=obs.dtype) if out is None else out
        if out is not None and self.Bm > B:
            out[:, B:] = 0                         # a caller's buffer may hold anything: the padding rows are zero
        pack_fields(buf[:, :B], self.layout.fields, rollout)
        return buf

    def _host_rollout(self, n_steps, actions, policy):
        """The (obs, action, reward, next_obs, absorbing, last) arrays [T, B, ...] of an engine without the packed kernels
        or of a host-side policy."""
        env = self.env
        if actions is not None:
            o = env.rollout(actions)
            return o['obs'], o['action'], o['reward'], o['next_obs'], o['absorbing'], o['last']
        assert policy is not None
        obs_l, act_l, rew_l, nobs_l, ab_l, last_l = [], [], [], [], [], []
        o = env.reset()
        for _ in range(n_steps):
            a = policy(o)
            no, r, absorbing, info = env.step(a)
            obs_l.append(o); act_l.append(torch.as_tensor(a, dtype=no.dtype, device=no.device))
            rew_l.append(r); nobs_l.append(no); ab_l.append(absorbing); last_l.append(info['last'])
            o = no
            if bool(info['last'].any()):
                # mushroom_rl.Core resets finished episodes between steps; engines created with
                # auto_reset=True have already done it on the device, others get a masked reset
                if not getattr(env, 'cfg', None) or not env.cfg.auto_reset:
                    o = env.reset(mask=info['last'])
                else:
                    o = env.reset(mask=torch.zeros_like(info['last']))
        return (torch.stack(obs_l), torch.stack(act_l), torch.stack(rew_l), torch.stack(nobs_l), torch.stack(ab_l),
                torch.stack(last_l))

    def compact_layout(self, n_steps):
        return CompactRecordLayout(self.sizes, self.D, self.k, n_steps)

    def compact_numel(self, n_steps):
        """Elements of one rank's compact send buffer for T = n_steps: the records and the worst case of exception rows,
        (T - 1) Bm (only the rows used are sent)."""
        lay = self.compact_layout(n_steps)
        return lay.record_numel + max(lay.T - 1, 0) * self.Bm * lay.E

    def _collect_local_compact(self, n_steps, actions, policy, noise, out):
        env = self.env
        T = int(actions.shape[0]) if actions is not None else int(n_steps)
        lay = self.compact_layout(T)
        cap = max(T - 1, 0) * self.Bm           # >= every rank's count: the gather pads every rank to the largest one
        need = lay.record_numel + cap * lay.E
        fused = hasattr(env, 'rollout_compact') and (actions is not None or hasattr(policy, 'as_struct'))
        if out is not None:
            if out.dim() != 1 or out.numel() < need or not out.is_contiguous():
                raise ValueError("out must be a flat contiguous tensor of at least %d elements" % need)
            flat = out[:need]
        else:
            dt = getattr(env, 'dtype', None)
            dev = getattr(env, 'device', torch.device('cpu'))
            flat = torch.empty((need,), device=dev, dtype=dt) if (fused or dt is not None) else None
        if fused:
            sh = CompactShard(flat, lay, cap)
            _, _, n = env.rollout_compact(actions=actions, policy=None if actions is not None else policy, n_steps=T,
                                          noise=noise, out=(sh.records, sh.ends), batch_stride=self.Bm, ends_capacity=cap)
            sh.n_ends = n
            return sh
        # engines without the compact kernel and host-side policies: pack here, listing every last row before the final
        # step (a superset of the auto-resets; the reconstruction is the same for any superset)
        B = env.batch
        obs, act, rew, nobs, ab, last = self._host_rollout(T, actions, policy)
        if flat is None:
            flat = torch.empty((need,), device=obs.device, dtype=obs.dtype)
        sh = CompactShard(flat, lay, cap)
        rec = sh.records
        rec.zero_()
        pack_fields(rec[:T, :B], lay.compact_fields, (obs, act, rew, ab, last))
        rec[T, :B, lay.compact_fields['obs']] = nobs[T - 1]
        tb = torch.nonzero(last[:T - 1].to(torch.bool))           # [n, 2] = (t, b)
        n = int(tb.shape[0])
        if n:
            e = sh.ends[:n]
            e[:, 0] = tb[:, 0].to(obs.dtype)
            e[:, 1] = tb[:, 1].to(obs.dtype)
            e[:, 2:] = nobs[tb[:, 0], tb[:, 1]]
        sh.n_ends = n
        return sh

    # ------------------------------------------------------------------ the one collective
    def gather(self, buf, out=None, async_op=False):
        """All-gather the packed rollout: [T, Bm, F] on every rank -> [W, T, Bm, F] on every rank, rank r's shard in
        block r (its first sizes[r] env rows are valid).  One collective, written straight into the final buffer.
        Without `out` the result lives in a buffer the collector keeps and REUSES: the next gather overwrites it (an
        on-policy learner consumes a dataset before collecting the next one); pass `out` or clone to keep it.
        async_op=True returns (result, work): the collective runs on the backend's own stream (RCCL) while the caller
        goes on -- e.g. launches the next rollout -- and `work.wait()` orders the result before its first use.
        A CompactShard (record_format 'compact') is gathered by gather_compact."""
        if isinstance(buf, CompactShard):
            return self.gather_compact(buf, out=out, async_op=async_op)
        self.last_gather_bytes = buf.numel() * buf.element_size()
        if self.world == 1 and not (self.force_collective and self.distributed):
            if out is not None:
                out.view(buf.shape).copy_(buf)
                return (out, _Done()) if async_op else out
            return (buf.unsqueeze(0), _Done()) if async_op else buf.unsqueeze(0)
        T, Bm, F = buf.shape
        shape = (self.world, T, Bm, F)
        if out is not None and (tuple(out.shape) != shape or out.dtype != buf.dtype or not out.is_contiguous()):
            raise ValueError("out must be a contiguous %s tensor of dtype %s" % (shape, buf.dtype))
        if buf.is_cuda and dist.get_backend(self.group) == 'gloo':
            # gloo moves host memory: the control-flow check mode (several ranks sharing one GPU in the tests;
            # BENCH_DIST_BACKEND=gloo).  The production transport is RCCL, device to device, below.
            host = torch.empty(shape, dtype=buf.dtype)
            dist.all_gather_into_tensor(host.view(self.world * T, Bm, F), buf.cpu(), group=self.group)
            res = host.to(buf.device) if out is None else out.copy_(host)
            return (res, _Done()) if async_op else res
        if out is None:
            if self._recv is None or tuple(self._recv.shape) != shape or self._recv.dtype != buf.dtype \
                    or self._recv.device != buf.device:
                self._recv = torch.empty(shape, device=buf.device, dtype=buf.dtype)
            out = self._recv
        # output handed over as the concatenation along dim 0 (the form every backend accepts)
        work = dist.all_gather_into_tensor(out.view(self.world * T, Bm, F), buf, group=self.group, async_op=async_op)
        return (out, work) if async_op else out

    def gather_compact(self, sh, out=None, async_op=False):
        """All-gather a CompactShard: ONE all-gather of the W exception counts, then ONE all-gather of every rank's flat
        segment -- its records followed by max(n_ends) exception rows, those past its own count zeroed -- into [W, L].
        Returns a CompactGather (unpack() gives the dataset).  `out`: a flat contiguous tensor of at least W L elements
        (L = records + max(n_ends) rows; W * compact_numel(T) always suffices); without it the collector reuses a buffer of
        its own, as gather() does."""
        lay, n = sh.layout, sh.n_ends
        collective = not (self.world == 1 and not (self.force_collective and self.distributed))
        gloo = collective and dist.get_backend(self.group) == 'gloo'
        if collective:
            dev = torch.device('cpu') if gloo else sh.flat.device
            mine = torch.tensor([n], dtype=torch.int64, device=dev)
            allc = torch.empty((self.world,), dtype=torch.int64, device=dev)
            dist.all_gather_into_tensor(allc, mine, group=self.group)
            counts = [int(c) for c in allc.cpu()]
        else:
            counts = [n]
        M = max(counts)
        if M > sh.capacity:
            raise ValueError("a rank produced %d exception rows, more than this rank's buffer holds (%d)" % (M, sh.capacity))
        L = lay.record_numel + M * lay.E
        if M > n:
            sh.flat[lay.record_numel + n * lay.E:L].zero_()
        send = sh.flat[:L]
        self.last_gather_bytes = L * send.element_size()
        W = self.world
        if out is not None and (out.dim() != 1 or out.numel() < W * L or out.dtype != send.dtype or not out.is_contiguous()):
            raise ValueError("out must be a flat contiguous %s tensor of at least %d elements" % (send.dtype, W * L))
        if not collective:
            res = send.view(1, L) if out is None else out[:L].copy_(send).view(1, L)
            g = CompactGather(res, lay, counts)
            return (g, _Done()) if async_op else g
        if send.is_cuda and gloo:
            host = torch.empty((W * L,), dtype=send.dtype)
            dist.all_gather_into_tensor(host, send.cpu(), group=self.group)
            res = host.to(send.device) if out is None else out[:W * L].copy_(host)
            g = CompactGather(res.view(W, L), lay, counts)
            return (g, _Done()) if async_op else g
        if out is None:
            r = self._recv_flat
            if r is None or r.numel() < W * L or r.dtype != send.dtype or r.device != send.device:
                self._recv_flat = torch.empty((W * L,), device=send.device, dtype=send.dtype)
            out = self._recv_flat
        dst = out[:W * L]
        work = dist.all_gather_into_tensor(dst, send, group=self.group, async_op=async_op)
        g = CompactGather(dst.view(W, L), lay, counts)
        return (g, work) if async_op else g

    def unpack(self, g):
        """Views (no copy) into gathered records [W, T, Bm, F]: every entry is [W, T, Bm, ...].  A CompactGather unpacks
        to the same dict (next_obs materialised, CompactRecordLayout.unpack)."""
        if isinstance(g, CompactGather):
            return g.unpack()
        return self.layout.unpack(g)

    def time_major(self, data):
        """[W, T, Bm, ...] -> [T, B_global, ...] with rank r's envs in block shard_bounds(global_batch, W, r).
        This one COPIES (a permute + concatenation); it is for consumers that insist on a single env axis and for
        comparing against a single-process run -- the collection path itself never needs it."""
        return self.layout.time_major(data)

    def collect(self, n_steps, actions=None, policy=None, noise=None):
        """Local rollout + global all-gather.  Returns the unpacked global dataset, shard-major [W, T, Bm, ...]."""
        return self.unpack(self.gather(self.collect_local(n_steps, actions=actions, policy=policy, noise=noise)))

    def collect_async(self, n_steps, actions=None, policy=None, noise=None, out=None):
        """Like collect(), but the all-gather is left in flight: returns a PendingRollout whose .wait() gives the
        dataset.  Lets a learner overlap the collective (1.4 GB received per rank for config 5) with whatever it does
        next on the compute stream -- typically the first kernels of its update, or the next rollout into another
        buffer (pass a distinct `out` per buffer in flight)."""
        local = self.collect_local(n_steps, actions=actions, policy=policy, noise=noise)
        g, work = self.gather(local, out=out, async_op=True)
        return PendingRollout(self, g, work, local)

    # ------------------------------------------------------------------ constraint statistics
    def get_constraints_logs(self, n_logged):
        """Global (c_avg, c_max, c_dq_max): the reference's get_constraints_logs (atacom.py:207-216) over every env
        of every rank.  n_logged = number of (env, step) entries this rank logged since the last call."""
        c_avg, c_max, c_dq = self.env.get_constraints_logs()
        if self.world == 1 and not (self.force_collective and self.distributed):
            return c_avg, c_max, c_dq
        dev = getattr(self.env, 'device', torch.device('cpu'))
        if self.distributed and dist.get_backend(self.group) == 'gloo':
            dev = torch.device('cpu')
        mx = torch.tensor([c_max, c_dq], dtype=torch.float64, device=dev)
        sm = torch.tensor([c_avg * n_logged, float(n_logged)], dtype=torch.float64, device=dev)
        dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=self.group)
        dist.all_reduce(sm, op=dist.ReduceOp.SUM, group=self.group)
        return float(sm[0] / sm[1]), float(mx[0]), float(mx[1])


class _Done:
    def wait(self):
        return True


class PendingRollout:
    """A collection whose all-gather may still be running (RolloutCollector.collect_async)."""

    def __init__(self, collector, gathered, work, local):
        self._c, self._g, self._work, self._local = collector, gathered, work, local     # `local` is the send buffer:
                                                                                           # kept alive until the wait
    def wait(self):
        self._work.wait()
        self._local = None
        return self._c.unpack(self._g)


def to_mushroom_dataset(data):
    """Flatten a time-major rollout [T, B, ...] into MushroomRL's list-of-tuples dataset (s, a, r, s', absorbing,
    last), env by env (what Core.learn would have produced running the envs one after another)."""
    obs, act, rew = (data[k].cpu().numpy() for k in ('obs', 'action', 'reward'))
    nobs, ab, last = (data[k].cpu().numpy() for k in ('next_obs', 'absorbing', 'last'))
    T, B = rew.shape
    out = []
    for b in range(B):
        for t in range(T):
            out.append((obs[t, b], act[t, b], float(rew[t, b]), nobs[t, b], bool(ab[t, b]), bool(last[t, b]) or t == T - 1))
    return out
