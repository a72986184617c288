"""Host-side logic that needs neither a GPU nor the library: sharding arithmetic, the packed-record layout and its views,
bench.py's helpers.  Property-based where the property is the specification."""
import os
import sys

import numpy as np
import torch
from hypothesis import given, settings, strategies as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from rl_on_manifold_amd.rollout import RolloutCollector, shard_bounds   # noqa: E402


@settings(max_examples=200, deadline=None)
@given(st.integers(1, 200000), st.integers(1, 64))
def test_shard_bounds_partition_the_batch(gb, world):
    spans = [shard_bounds(gb, world, r) for r in range(world)]
    assert spans[0][0] == 0 and spans[-1][1] == gb
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))             # contiguous, in rank order
    sizes = [hi - lo for lo, hi in spans]
    assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)   # remainder goes to the low ranks


class _Env:
    """The smallest engine surface the collector touches."""
    def __init__(self, B, D, k):
        self.batch, self.obs_dim, self.dims = B, D, {'null': k}
        self.device = torch.device('cpu')

    def rollout(self, actions):
        T, B, k = actions.shape
        g = torch.Generator().manual_seed(T * 1000 + B)
        return {'obs': torch.randn((T, B, self.obs_dim), generator=g, dtype=torch.float64),
                'next_obs': torch.randn((T, B, self.obs_dim), generator=g, dtype=torch.float64),
                'reward': torch.randn((T, B), generator=g, dtype=torch.float64),
                'absorbing': torch.rand((T, B), generator=g) < 0.1, 'last': torch.rand((T, B), generator=g) < 0.2,
                'action': torch.as_tensor(actions, dtype=torch.float64)}


@settings(max_examples=50, deadline=None)
@given(st.integers(1, 9), st.integers(1, 7), st.integers(1, 6), st.integers(1, 5))
def test_packed_records_round_trip(B, T, D, k):
    """collect_local packs (s, a, r, s', absorbing, last) into F = 2D + k + 3 floats; unpack / time_major give them back."""
    env = _Env(B, D, k)
    col = RolloutCollector(env)
    acts = torch.randn((T, B, k), dtype=torch.float64)
    ref = env.rollout(acts)
    buf = col.collect_local(T, actions=acts)
    assert buf.shape == (T, B, 2 * D + k + 3)
    data = col.time_major(col.unpack(col.gather(buf)))
    for key in ('obs', 'next_obs', 'reward', 'action'):
        assert torch.equal(data[key], ref[key]), key
    assert torch.equal(data['absorbing'], ref['absorbing']) and torch.equal(data['last'], ref['last'])
    flat = col.gather(buf).reshape(-1, col.F)                            # the flat sample set an on-policy fit consumes
    assert flat.shape[0] == T * B and flat.is_contiguous()


def test_collector_rejects_a_shard_of_the_wrong_size():
    import pytest
    with pytest.raises(ValueError):
        RolloutCollector(_Env(5, 4, 1), global_batch=7)                  # world 1: the single shard must hold all 7


def test_bench_helpers():
    import bench
    assert 1 <= bench.usable_cores() <= (os.cpu_count() or 1)
    for name, (M, N, K, nq, sub) in bench.SHAPES.items():
        assert N - M == K and bench.ALGO_BYTES[name] > 0
    rv, r = bench.roofline_objects('iiwa', 8192, 0.028)              # the binding roof (vector ALU) first, then the HBM view
    assert r['bound'] == 'hbm' and rv['bound'] == 'valu_f32'
    assert abs(r['achieved'] - 400 * 8192 / 0.028e-3 / 1e9) < 1e-6 and abs(r['frac'] - r['achieved'] / 8000.0) < 1e-12
    assert rv['unit'] == 'TFLOP/s' and 0.05 < rv['frac'] < 0.2
    rc, _ = bench.roofline_objects('iiwa', 8192, 0.028, chart='canonical')
    assert rc['algorithmic_flops_per_launch'] < rv['algorithmic_flops_per_launch'] / 3
    port = bench._free_port()
    assert 1024 < port < 65536


def test_bench_dump_outputs_types_and_cap(tmp_path, monkeypatch):
    """--dump-outputs: float arrays keep their type, flags become float32; above the cap every array keeps the same seeded
    rows, listed in sample_rows.npy, and the files stay within the cap."""
    import bench
    B = 1000
    rng = np.random.default_rng(3)
    arrays = {'obs': rng.normal(size=(B, 18)).astype(np.float32), 'reward': rng.normal(size=B),
              'absorbing': (rng.random(B) < 0.5).astype(np.uint8)}
    bench.dump_outputs(str(tmp_path / 'all'), arrays)
    got = {n: np.load(str(tmp_path / 'all' / (n + '.npy'))) for n in arrays}
    assert got['obs'].dtype == np.float32 and got['reward'].dtype == np.float64 and got['absorbing'].dtype == np.float32
    assert all(np.array_equal(got[n], arrays[n]) for n in arrays)
    assert not (tmp_path / 'all' / 'sample_rows.npy').exists()
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 20000)
    for run in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / run), arrays)
    files = sorted(os.listdir(str(tmp_path / 'a')))
    assert files == ['absorbing.npy', 'obs.npy', 'reward.npy', 'sample_rows.npy']
    rows = np.load(str(tmp_path / 'a' / 'sample_rows.npy'))
    assert rows.dtype == np.float64 and 0 < len(rows) < B and np.all(np.diff(rows) > 0)
    payload = 0
    for n in files:
        a, b = np.load(str(tmp_path / 'a' / n)), np.load(str(tmp_path / 'b' / n))
        assert np.array_equal(a, b) and len(a) == len(rows)
        payload += a.nbytes
        if n != 'sample_rows.npy':
            assert np.array_equal(a, arrays[n[:-4]][rows.astype(np.int64)].astype(a.dtype))
    assert payload <= 20000


# ------------------------------------------------------------------ the shared host layer of the device environments
def _same_view(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


class _Stub:
    """What the shared methods read, without a GPU or a library."""
    def __init__(self, B=3, D=4, k=2):
        self.batch, self.obs_dim, self.dims = B, D, {'null': k}
        self.device, self.dtype = torch.device('cpu'), torch.float64

    def _on_my_device(self, t):
        return t.device == self.device


@settings(max_examples=50, deadline=None)
@given(st.integers(1, 9), st.integers(1, 6), st.integers(0, 10 ** 6))
def test_record_layout_has_one_definition(D, k, seed):
    """The field slices of rollout.record_fields are the views RecordLayout.unpack and both engines' unpack_records return."""
    from rl_on_manifold_amd.rollout import RecordLayout, compact_record_fields, record_fields
    from rl_on_manifold_amd.engine import BatchedAtacomEnv
    from rl_on_manifold_amd.point import BatchedPointReachEnv
    fields, F = record_fields(D, k)
    _, Fc, E = compact_record_fields(D, k)
    assert F == 2 * D + k + 3 and Fc == D + k + 3 and E == D + 2
    rec = torch.rand((2, 3, F), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    stub = _Stub(3, D, k)
    got = (RecordLayout([3], D, k).unpack(rec), BatchedAtacomEnv.unpack_records(stub, rec),
           BatchedPointReachEnv.unpack_records(stub, rec))
    for name in ('obs', 'action', 'reward', 'next_obs'):
        assert all(_same_view(g[name], rec[..., fields[name]]) for g in got), name
    for name in ('absorbing', 'last'):
        assert all(g[name].dtype == torch.bool and torch.equal(g[name], rec[..., fields[name]] > 0.5) for g in got), name
    # the fields tile the record in the order [obs | action | reward | next_obs | absorbing | last]
    cover = torch.cat([torch.arange(F)[ix].reshape(-1) for ix in fields.values()])
    assert list(fields) == ['obs', 'action', 'reward', 'next_obs', 'absorbing', 'last'] and torch.equal(cover, torch.arange(F))


def test_compact_layout_rebuilds_a_hand_built_dataset():
    """T = 3, B = 2, D = 2, k = 1: records [T + 1, B, Fc = 6] and two exception rows against the dataset written out by hand."""
    from rl_on_manifold_amd.rollout import CompactRecordLayout
    T, B, D, k = 3, 2, 2, 1
    f64 = torch.float64
    #                        obs         action reward absorbing last
    rec = torch.tensor([[[1.0, 2.0, 0.1, 10.0, 0.0, 1.0], [3.0, 4.0, 0.2, 20.0, 1.0, 1.0]],          # t = 0: both envs end
                        [[5.0, 6.0, 0.3, 30.0, 0.0, 0.0], [7.0, 8.0, 0.4, 40.0, 0.0, 0.0]],          # t = 1
                        [[9.0, 10.0, 0.5, 50.0, 0.0, 0.0], [11.0, 12.0, 0.6, 60.0, 0.0, 1.0]],       # t = 2
                        [[13.0, 14.0, 0.0, 0.0, 0.0, 0.0], [15.0, 16.0, 0.0, 0.0, 0.0, 0.0]]], dtype=f64)   # the tail
    ends = torch.tensor([[0.0, 1.0, -3.0, -4.0], [0.0, 0.0, -1.0, -2.0]], dtype=f64)               # [t, b, terminal obs]
    lay = CompactRecordLayout([B], D, k, T)
    assert (lay.Fc, lay.E) == (6, 4) and rec.shape == (T + 1, B, lay.Fc)
    got = lay.unpack(rec, ends)
    want = {'obs': [[[1, 2], [3, 4]], [[5, 6], [7, 8]], [[9, 10], [11, 12]]],
            'action': [[[0.1], [0.2]], [[0.3], [0.4]], [[0.5], [0.6]]],
            'reward': [[10, 20], [30, 40], [50, 60]],
            'next_obs': [[[-1, -2], [-3, -4]], [[9, 10], [11, 12]], [[13, 14], [15, 16]]],
            'absorbing': [[False, True], [False, False], [False, False]],
            'last': [[True, True], [False, False], [False, True]]}
    assert list(got) == list(want)
    for name, v in want.items():
        w = torch.tensor(v, dtype=torch.bool if name in ('absorbing', 'last') else f64)
        assert got[name].dtype == w.dtype and torch.equal(got[name], w), name
    only_first = lay.unpack(rec, ends, n_ends=1)['next_obs']                  # the second row is past the count: not applied
    assert torch.equal(only_first[0], torch.tensor([[5.0, 6.0], [-3.0, -4.0]], dtype=f64))


def test_packed_output_buffer():
    """DeviceEnv._packed_out: empty when the env axis is not padded, zero padding rows otherwise (its own or the caller's
    buffer), and a caller's buffer of the wrong shape, dtype or strides is refused."""
    import pytest
    from rl_on_manifold_amd._device_env import DeviceEnv
    stub, seen = _Stub(B=3), []
    T, F = 4, 11
    real_empty, real_zeros = torch.empty, torch.zeros
    try:
        torch.empty = lambda *a, **kw: seen.append('empty') or real_empty(*a, **kw)
        torch.zeros = lambda *a, **kw: seen.append('zeros') or real_zeros(*a, **kw)
        own = DeviceEnv._packed_out(stub, T, 3, F, None)
        padded = DeviceEnv._packed_out(stub, T, 5, F, None)
    finally:
        torch.empty, torch.zeros = real_empty, real_zeros
    assert seen == ['empty', 'zeros']                                     # ld == B allocates without zeroing
    assert own.shape == (T, 3, F) and own.dtype == stub.dtype and own.is_contiguous()
    assert padded.shape == (T, 5, F) and bool((padded[:, 3:] == 0).all())
    mine = torch.full((T, 5, F), -777.0, dtype=torch.float64)
    assert DeviceEnv._packed_out(stub, T, 5, F, mine) is mine
    assert bool((mine[:, 3:] == 0).all()) and bool((mine[:, :3] == -777.0).all())
    for bad in (torch.zeros((T, 4, F), dtype=torch.float64), torch.zeros((T, 5, F), dtype=torch.float32),
                torch.zeros((T, 5, 2 * F), dtype=torch.float64)[..., ::2]):
        with pytest.raises(ValueError, match='must be a contiguous'):
            DeviceEnv._packed_out(stub, T, 5, F, bad)


def test_the_device_environments_share_one_host_layer():
    from rl_on_manifold_amd._device_env import DeviceEnv
    from rl_on_manifold_amd.engine import BatchedAtacomEnv
    from rl_on_manifold_amd.point import BatchedPointReachEnv
    for cls in (BatchedAtacomEnv, BatchedPointReachEnv):
        assert issubclass(cls, DeviceEnv)
        for name in ('_as_dev', '_check_io', '_stream', '_on_my_device', 'unpack_records', 'close', '__del__'):
            assert name not in vars(cls) and name in vars(DeviceEnv), (cls.__name__, name)
