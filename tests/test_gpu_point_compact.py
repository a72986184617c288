"""GPU tests of the collision-avoidance task collected in the compact record format (libatacom_point_compact.so,
k_point_rollout_compact) through BatchedPointReachEnv.rollout_compact, the C ABI and RolloutCollector.

Every bound is EQUALITY (torch.equal): the comparator is the full-format call of the same build, rollout_packed unpacked with
RecordLayout, on a twin environment of the same configuration, state and inputs.

Shapes.  B = 300 environments are two workgroups of 256, the second with one full wave and one of 44 live lanes (the matrix-core
path's shadow lanes and the masked stores); batch_stride = 320 pads the env axis.  T = 11 steps at horizon 4 with the episode
step counter staggered b % 4 before the rollout: episode ends fall on every t, T-1 included, and on a subset of the lanes of
every wave."""
import os
import sys

import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_point_policy import _pair            # noqa: E402  (the five agents' policies of the task)

DEV = 'cuda:0'
DT = {'f32': torch.float32, 'f64': torch.float64}
KEYS = ('obs', 'action', 'reward', 'next_obs', 'absorbing', 'last')
B, T, H, LD = 300, 11, 4, 320
SENTINEL = -777.0


def _envs(count, n, rw, dt, auto_reset=True, batch=B):
    """`count` environments of one configuration, reset, then staggered: environment b has taken b % 4 steps of its episode."""
    from rl_on_manifold_amd import BatchedPointReachEnv
    envs = [BatchedPointReachEnv(batch, n_objects=n, random_walk=rw, horizon=H, seed=6, auto_reset=auto_reset, device=DEV,
                                 dtype=DT[dt]) for _ in range(count)]
    envs[0].reset()
    st = envs[0].get_state()
    steps = (torch.arange(batch, device=DEV) % 4).to(st.dtype)
    st[:, -3] = steps                                  # [..., _time, steps taken, episodes started, centres set]
    st[:, -4] = steps * 0.01
    for e in envs:
        e.set_state(st)
    return envs


def _inputs(n, dt, supplied, seed=0, batch=B):
    g = torch.Generator(device=DEV).manual_seed(seed)
    acts = torch.rand((T, batch, 2), device=DEV, dtype=DT[dt], generator=g) * 2.4 - 1.2
    noise = torch.randn((T, batch, 2), device=DEV, dtype=DT[dt], generator=g)
    draws = (torch.rand((T, batch, n, 2), device=DEV, dtype=DT[dt], generator=g) * 2 - 1) if supplied else None
    return acts, noise, draws


def _unpack_full(env, full):
    from rl_on_manifold_amd import RecordLayout
    return RecordLayout([env.batch], env.obs_dim, 2).unpack(full)


def _unpack_compact(env, rec, ends, n):
    from rl_on_manifold_amd import CompactRecordLayout
    return CompactRecordLayout([env.batch], env.obs_dim, 2, T).unpack(rec, ends, n)


def _assert_compact_is_full(a, b, full, rec, ends, n):
    """full: env a's rollout_packed; (rec, ends, n): env b's rollout_compact.  Every key, the tail, the count, the state."""
    D = a.obs_dim
    assert rec.shape == (T + 1, LD, D + 5) and ends.shape == (n, D + 2)
    ref, got = _unpack_full(a, full), _unpack_compact(b, rec, ends, n)
    for key in KEYS:
        assert got[key].shape == ref[key].shape and got[key].dtype == ref[key].dtype, key
        assert torch.equal(got[key], ref[key]), key
    assert not rec[T, :, D:].any().item()                                  # the tail's five zeros, written by the kernel
    assert not rec[:, B:].any().item() and not full[:, B:].any().item()    # padding rows: zero in both formats
    assert ref['last'][T - 1, :B].any().item() and all(ref['last'][t, :B].any().item() for t in range(T))
    want = int(ref['last'][:T - 1, :B].sum()) if a.cfg.auto_reset else 0
    assert n == want, (n, want)
    assert torch.equal(a.get_state(), b.get_state())
    assert a.get_constraints_logs() == b.get_constraints_logs()
    return ref


# ---------------------------------------------------------------------------------------------------- 1. actions
@pytest.mark.parametrize('supplied', [False, True])
@pytest.mark.parametrize('mode', ['auto_reset', 'no_reset'])
@pytest.mark.parametrize('rw', [0, 1])
@pytest.mark.parametrize('n', [2, 4])
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_compact_unpacks_to_packed_with_actions(dt, n, rw, mode, supplied):
    a, b = _envs(2, n, bool(rw), dt, auto_reset=mode == 'auto_reset')
    acts, _, draws = _inputs(n, dt, supplied, seed=1)
    D = a.obs_dim
    out = None
    if supplied:                       # the caller's buffers, holding a sentinel: the padding rows are zeroed as in rollout_packed
        out = (torch.full((T + 1, LD, D + 5), SENTINEL, device=DEV, dtype=DT[dt]),
               torch.full(((T - 1) * B, D + 2), SENTINEL, device=DEV, dtype=DT[dt]))
    full = a.rollout_packed(actions=acts, draws=draws, batch_stride=LD,
                            out=None if out is None else torch.full((T, LD, 2 * D + 5), SENTINEL, device=DEV, dtype=DT[dt]))
    rec, ends, n_ends = b.rollout_compact(actions=acts, draws=draws, batch_stride=LD, out=out)
    _assert_compact_is_full(a, b, full, rec, ends, n_ends)
    if supplied:
        assert rec.data_ptr() == out[0].data_ptr()                       # the caller's buffers are the ones returned
        assert ends.untyped_storage().data_ptr() == out[1].untyped_storage().data_ptr()      # (an empty view has no pointer)
        assert not (rec[:, :B] == SENTINEL).any().item()                  # every record and the whole tail row written
        assert (out[1][n_ends:] == SENTINEL).all().item()                  # nothing past the rows counted
    if mode == 'auto_reset':
        assert n_ends == (ends[:, 0] < T - 1).sum().item() and n_ends >= 2 * B


# ---------------------------------------------------------------------------------------------------- 2. policy
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('kind,n', [('gauss', 4), ('sac', 4), ('td3', 4), ('ddpg', 4), ('gauss', 2), ('ddpg', 2)])
def test_compact_unpacks_to_packed_with_a_policy(kind, n, dt):
    a, b, c = _envs(3, n, True, dt)
    pa, _ = _pair(kind, n)
    pb, _ = _pair(kind, n)
    _, noise, draws = _inputs(n, dt, True, seed=2)
    full = a.rollout_packed(policy=pa, n_steps=T, noise=noise, draws=draws, batch_stride=LD)
    rec, ends, n_ends = b.rollout_compact(policy=pb, n_steps=T, noise=noise, draws=draws, batch_stride=LD)
    ref = _assert_compact_is_full(a, b, full, rec, ends, n_ends)
    assert torch.isfinite(ref['action']).all().item()
    if kind == 'ddpg':                                 # the Ornstein-Uhlenbeck state restarts at episode starts, in both
        assert torch.equal(pa.noise_state, pb.noise_state) and pb.noise_state.any().item()
    # the recorded actions ARE what the step received: replayed as pre-generated actions they give the same records
    got = _unpack_compact(b, rec, ends, n_ends)
    replay = _unpack_full(c, c.rollout_packed(actions=got['action'][:, :B].contiguous(), draws=draws, batch_stride=LD))
    for key in ('obs', 'reward', 'next_obs', 'last'):
        assert torch.equal(replay[key], got[key]), key
    assert torch.equal(c.get_state(), b.get_state())


def test_a_plain_callable_is_refused_as_in_rollout_packed():
    (env,) = _envs(1, 2, True, 'f32', batch=8)
    with pytest.raises(ValueError, match='MlpPolicy'):
        env.rollout_compact(policy=lambda o: o[:, :2], n_steps=2)
    with pytest.raises(ValueError, match='either actions or policy'):
        env.rollout_compact()
    with pytest.raises(ValueError, match='ends_capacity must be >= 0'):
        env.rollout_compact(actions=torch.zeros((2, 8, 2), device=DEV), ends_capacity=-1)
    with pytest.raises(ValueError, match=r'out\[0\] must be a contiguous \[3, 8, 17\]'):
        env.rollout_compact(actions=torch.zeros((2, 8, 2), device=DEV),
                            out=(torch.zeros((2, 8, 17), device=DEV), torch.zeros((8, 14), device=DEV)))
    with pytest.raises(ValueError, match=r'out\[1\] must be a contiguous \[>= 8, 14\]'):
        env.rollout_compact(actions=torch.zeros((2, 8, 2), device=DEV),
                            out=(torch.zeros((3, 8, 17), device=DEV), torch.zeros((8, 13), device=DEV)))


# ---------------------------------------------------------------------------------------------------- 3. overflow
def test_overflow_raises_and_writes_nothing_past_the_capacity():
    n = 4
    a, b = _envs(2, n, True, 'f32')
    acts, _, _ = _inputs(n, 'f32', False, seed=3)
    D = a.obs_dim
    full = a.rollout_packed(actions=acts, batch_stride=LD)
    rec = torch.full((T + 1, LD, D + 5), SENTINEL, device=DEV)
    ends = torch.full((50, D + 2), float('nan'), device=DEV)             # a larger buffer holding a sentinel
    count = int(_unpack_full(a, full)['last'][:T - 1, :B].sum())
    with pytest.raises(ValueError, match=r'(?s)%d episode-end rows, capacity 1\b.*larger ends_capacity' % count):
        b.rollout_compact(actions=acts, out=(rec, ends), batch_stride=LD, ends_capacity=1)
    torch.cuda.synchronize()
    assert torch.isfinite(ends[0]).all() and 0 <= float(ends[0, 0]) < T - 1 and 0 <= float(ends[0, 1]) < B   # one episode end
    assert torch.isnan(ends[1:]).all()                                   # nothing past the capacity
    # the records are complete all the same: every field that does not need the lost rows equals the reference run
    ref = _unpack_full(a, full)
    got = _unpack_compact(b, rec, ends[:1], 1)
    for key in ('obs', 'action', 'reward', 'absorbing', 'last'):
        assert torch.equal(got[key], ref[key]), key
    assert torch.equal(got['next_obs'][T - 1], ref['next_obs'][T - 1])   # the tail
    t0, b0 = int(ends[0, 0]), int(ends[0, 1])
    assert torch.equal(ends[0, 2:], ref['next_obs'][t0, b0]) and bool(ref['last'][t0, b0])
    assert torch.equal(a.get_state(), b.get_state())


# ---------------------------------------------------------------------------------------------------- 4. graph capture
def test_compact_rollout_is_capturable_in_a_graph():
    """No host synchronisation inside the C call: it can be captured in a HIP graph and replayed (the counter is reset by a
    memset node).  One stream, no parallel branches."""
    from rl_on_manifold_amd import _lib_point_compact
    n = 4
    a, b = _envs(2, n, True, 'f32')
    acts, _, draws = _inputs(n, 'f32', True, seed=4)
    D = a.obs_dim
    recs = torch.full((T + 1, LD, D + 5), SENTINEL, device=DEV)
    ends = torch.zeros(((T - 1) * B, D + 2), device=DEV)
    cnt = torch.full((1,), 12345, device=DEV, dtype=torch.int32)
    lib = _lib_point_compact.load()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        rc = lib.atacom_point_compact_rollout(b._h, T, acts.data_ptr(), None, None, draws.data_ptr(), recs.data_ptr(), LD,
                                              ends.data_ptr(), ends.shape[0], cnt.data_ptr(), s.cuda_stream)
    assert rc == 0, lib.atacom_point_compact_last_error().decode()
    graph.replay()
    torch.cuda.synchronize()
    count = int(cnt.item())
    rec_ref, ends_ref, n_ref = a.rollout_compact(actions=acts, draws=draws, batch_stride=LD)
    assert count == n_ref and n_ref > 0
    assert torch.equal(recs[:, :B], rec_ref[:, :B])
    assert (recs[:, B:] == SENTINEL).all().item()                        # the C call never writes the padding rows
    key = lambda e: e[torch.argsort(e[:, 0] * B + e[:, 1])]        # noqa: E731  (rows are appended in no fixed order)
    assert torch.equal(key(ends[:count]), key(ends_ref))
    assert torch.equal(a.get_state(), b.get_state())


# ---------------------------------------------------------------------------------------------------- 5. collector
@pytest.mark.parametrize('how', ['policy', 'actions', 'ragged'])
def test_compact_collector_takes_the_fused_path(how, monkeypatch):
    """RolloutCollector(record_format='compact') on this task: the dataset of the 'full' collector, from the environments'
    CURRENT state and without the host loop (before rollout_compact existed it reset the environments and stepped them one
    launch at a time)."""
    from rl_on_manifold_amd import RolloutCollector
    n = 4
    a, b = _envs(2, n, True, 'f32')
    pa, _ = _pair('gauss', n)
    pb, _ = _pair('gauss', n)
    acts, noise, _ = _inputs(n, 'f32', False, seed=5)
    host_calls = []
    real = RolloutCollector._host_rollout
    monkeypatch.setattr(RolloutCollector, '_host_rollout', lambda self, *x: host_calls.append(x) or real(self, *x))
    if how == 'ragged':
        # a shard narrower than the collective's stride: batch_stride > batch through collect_local(out=...).  No process
        # group here, so the collectors are given the shard table of rank 0 of a ragged world whose largest shard has LD envs
        cf, cc = (RolloutCollector(e, record_format=f) for e, f in ((a, 'full'), (b, 'compact')))
        for col in (cf, cc):
            col.sizes, col.Bm = [B, LD], LD
        full = cf.collect_local(T, actions=acts)
        sh = cc.collect_local(T, actions=acts, out=torch.full((cc.compact_numel(T),), SENTINEL, device=DEV))
        assert full.shape == (T, LD, a.record_dim) and sh.records.shape == (T + 1, LD, a.obs_dim + 5)
        ref = _unpack_full(a, full)
        got = _unpack_compact(b, sh.records, sh.ends, sh.n_ends)
        for key in KEYS:
            assert torch.equal(got[key], ref[key]), key
        assert not sh.records[:, B:].any().item()
    else:
        kw = dict(policy=pa, noise=noise) if how == 'policy' else dict(actions=acts)
        full = RolloutCollector(a).collect(T, **kw)
        kw = dict(policy=pb, noise=noise) if how == 'policy' else dict(actions=acts)
        comp = RolloutCollector(b, record_format='compact').collect(T, **kw)
        assert sorted(comp) == sorted(full)
        for key in full:
            assert comp[key].shape == full[key].shape and torch.equal(comp[key], full[key]), key
        assert full['last'][:T - 1].any().item()
    assert not host_calls
    assert torch.equal(a.get_state(), b.get_state())
