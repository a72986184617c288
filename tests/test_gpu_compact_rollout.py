"""GPU tests of the compact record format (atacom_rollout_compact): two handles of the same configuration, initial states and
actions, one rolled out with rollout_packed and one with rollout_compact, unpack to IDENTICAL tensors on every key, padding rows
included -- on every task, dtype and lane mapping, with and without auto-reset, the in-kernel policy (shadow lanes), the noise
options and the rigid-body mode; the collector in compact form over RCCL (world 1) and gloo (two processes on one GPU); and
config 5 at full size (8 x 8192 x 120 iiwa shards)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
KEYS = ('obs', 'action', 'reward', 'next_obs', 'absorbing', 'last')
DTYPES = {'f32': torch.float32, 'f64': torch.float64}


def _env(name, B, dt='f32', **kw):
    from rl_on_manifold_amd import BatchedAtacomEnv
    return BatchedAtacomEnv(name, B, device=DEV, dtype=DTYPES[dt], **kw)


def _policy(D, k, dtype, seed=0):
    from rl_on_manifold_amd import MlpPolicy
    g = torch.Generator().manual_seed(seed)
    c = lambda x: x.to(dtype)      # noqa: E731
    return MlpPolicy(c(torch.randn(64, D, generator=g) * 0.2), c(torch.randn(64, generator=g) * 0.1),
                     c(torch.randn(64, 64, generator=g) * 0.1), c(torch.randn(64, generator=g) * 0.1),
                     c(torch.randn(k, 64, generator=g) * 0.1), c(torch.zeros(k)), std=c(torch.full((k,), 0.3)))


def _full_and_compact(make, T, stride, actions=None, policy=None, noise=None):
    """rollout_packed on one handle, rollout_compact on a twin: (full unpacked, compact unpacked, n_ends, full records)."""
    from rl_on_manifold_amd import RecordLayout, CompactRecordLayout
    a, b = make(), make()
    B, D, k = a.batch, a.obs_dim, a.dims['null']
    kw = dict(actions=actions) if actions is not None else dict(policy=policy, n_steps=T, noise=noise)
    full = a.rollout_packed(batch_stride=stride, **kw)
    rec, ends, n = b.rollout_compact(batch_stride=stride, **kw)
    assert rec.shape == (T + 1, stride, D + k + 3) and ends.shape == (n, D + 2)
    assert (rec[:, B:] == 0).all()
    ref = RecordLayout([B], D, k).unpack(full)
    got = CompactRecordLayout([B], D, k, T).unpack(rec, ends, n)
    for key in KEYS:
        assert got[key].shape == ref[key].shape and got[key].dtype == ref[key].dtype, key
        assert torch.equal(got[key], ref[key]), key
    # the kernel lists exactly the episode ends before the last step of an auto-resetting handle
    want = int(ref['last'][:T - 1].sum()) if a.cfg.auto_reset else 0
    assert n == want, (n, want)
    for e in (a, b):
        e.close()
    return ref, n


@pytest.mark.parametrize('mode', ['no_reset', 'auto_reset', 'random_init'])
@pytest.mark.parametrize('lanes', [1, 2, 4, 8])
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('name', ['circle', 'planar', 'iiwa'])
def test_compact_rollout_unpacks_to_the_packed_rollout(name, dt, lanes, mode):
    B, T = 133, 23
    kw = dict(lanes_per_env=lanes, horizon=7, auto_reset=mode != 'no_reset', random_init=mode == 'random_init', seed=5)
    k = _env(name, 1, dt).dims['null']
    g = torch.Generator(device=DEV).manual_seed(1)
    acts = (torch.rand((T, B, k), device=DEV, generator=g) * 2.4 - 1.2).to(DTYPES[dt])
    ref, n = _full_and_compact(lambda: _env(name, B, dt, **kw), T, B + 3, actions=acts)
    if mode != 'no_reset':
        assert n >= B                                        # horizon 7: episode ends before the last step are exception rows


@pytest.mark.mapping(kind='mlp')
@pytest.mark.parametrize('lanes', [1, 2, 4, 8])
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('name', ['planar', 'iiwa'])
def test_compact_policy_rollout_unpacks_to_the_packed_policy_rollout(name, dt, lanes):
    """The in-kernel policy at a batch that is not a multiple of 16: the matrix-core path's shadow lanes (past the batch, on
    environment B-1) must neither append a row nor write a tail."""
    B, T = 201, 19
    probe = _env(name, 1, dt)
    D, k = probe.obs_dim, probe.dims['null']
    pol = _policy(D, k, DTYPES[dt])
    g = torch.Generator(device=DEV).manual_seed(2)
    eps = torch.randn((T, B, k), device=DEV, generator=g).to(DTYPES[dt])
    ref, n = _full_and_compact(lambda: _env(name, B, dt, lanes_per_env=lanes, horizon=6, auto_reset=True), T, B + 5,
                               policy=pol, noise=eps)
    assert n >= 2 * B


@pytest.mark.parametrize('path', ['actions', 'policy'])
@pytest.mark.parametrize('opts', ['obs_noise', 'obs_delay', 'env_noise', 'all_noise', 'rigid_body', 'rigid_body_ff'])
def test_compact_rollout_with_noise_options_and_rigid_body(opts, path):
    kw = {'all_noise': dict(obs_noise=True, obs_delay=True, env_noise=True),
          'rigid_body': dict(dynamics_mode='rigid_body'), 'rigid_body_ff': dict(dynamics_mode='rigid_body_ff')}.get(
        opts, {opts: True})
    B, T = 150, 17
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        make = lambda: _env('iiwa', B, horizon=5, auto_reset=True, random_init=True, seed=3, **kw)     # noqa: E731
        make().close()
    g = torch.Generator(device=DEV).manual_seed(4)
    if path == 'actions':
        acts = torch.rand((T, B, 5), device=DEV, generator=g) * 2 - 1
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ref, n = _full_and_compact(make, T, B + 1, actions=acts)
    else:
        pol = _policy(18, 5, torch.float32)
        eps = torch.randn((T, B, 5), device=DEV, generator=g)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            ref, n = _full_and_compact(make, T, B + 1, policy=pol, noise=eps)
    assert n >= 2 * B


@pytest.mark.parametrize('case', ['f64_noise_policy', 'circle_policy', 'canonical_rigid_policy'])
def test_compact_rollout_refuses_what_the_packed_rollout_refuses(case):
    from rl_on_manifold_amd import AtacomError, _lib
    name, dt, kw = {'f64_noise_policy': ('iiwa', 'f64', dict(obs_noise=True)),
                    'circle_policy': ('circle', 'f32', {}),
                    'canonical_rigid_policy': ('iiwa', 'f32', dict(chart_mode='canonical', dynamics_mode='rigid_body_ff'))}[case]
    env = _env(name, 20, dt, auto_reset=True, **kw)
    D, k = env.obs_dim, env.dims['null']
    pol = _policy(D, k, DTYPES[dt])
    errs = []
    for call in (lambda: env.rollout_packed(policy=pol, n_steps=4),
                 lambda: env.rollout_compact(policy=pol, n_steps=4)):
        with pytest.raises(AtacomError) as ei:
            call()
        errs.append(str(ei.value))
    assert errs[0].replace('atacom_rollout_packed', 'X') == errs[1].replace('atacom_rollout_compact', 'X')
    # the codes are those of the packed call too (ATACOM_E_UNSUPPORTED), straight from the C ABI
    import ctypes as C
    net = pol.as_struct(env)
    recs = torch.empty((5, 20, D + k + 3), device=DEV, dtype=DTYPES[dt])
    ends = torch.empty((60, D + 2), device=DEV, dtype=DTYPES[dt])
    cnt = torch.zeros((1,), device=DEV, dtype=torch.int32)
    rc = env._lib.atacom_rollout_compact(env._h, 4, None, C.byref(net), None, recs.data_ptr(), 20, ends.data_ptr(), 60,
                                         cnt.data_ptr(), env._stream())
    assert rc == _lib.E_UNSUPPORTED
    # and the argument checks of the compact call
    for args in ((4, 19, 60), (4, 20, -1), (1 << 24, 20, 60), (4, 1 << 24, 60)):
        rc = env._lib.atacom_rollout_compact(env._h, args[0], None, C.byref(net), None, recs.data_ptr(), args[1],
                                             ends.data_ptr(), args[2], cnt.data_ptr(), env._stream())
        assert rc == _lib.E_INVALID, args
    rc = env._lib.atacom_rollout_compact(env._h, 4, None, C.byref(net), None, recs.data_ptr(), 20, ends.data_ptr(), 60,
                                         None, env._stream())
    assert rc == _lib.E_INVALID
    env.close()


def test_compact_rollout_overflow_raises_and_writes_nothing_past_the_capacity():
    B, T, cap = 64, 12, 1
    env = _env('planar', B, horizon=3, auto_reset=True)
    D, k = env.obs_dim, env.dims['null']
    acts = torch.zeros((T, B, k), device=DEV)
    rec = torch.empty((T + 1, B, D + k + 3), device=DEV)
    ends = torch.full((50, D + 2), float('nan'), device=DEV)            # a larger buffer holding a sentinel
    with pytest.raises(ValueError, match=r'(?s)\d+ episode-end rows, capacity 1.*snapshot'):
        env.rollout_compact(actions=acts, out=(rec, ends), ends_capacity=cap)
    torch.cuda.synchronize()
    assert torch.isfinite(ends[0]).all() and 0 <= float(ends[0, 0]) < T - 1     # the one row written: an episode end
    assert torch.isnan(ends[1:]).all()                                   # nothing past the capacity
    env.close()


def test_compact_rollout_is_capturable_in_a_graph():
    """No host synchronisation inside the C call: it can be captured in a HIP graph and replayed (the counter is reset by a
    memset node)."""
    import ctypes as C
    B, T = 96, 9
    make = lambda: _env('iiwa', B, horizon=4, auto_reset=True)     # noqa: E731
    a, b = make(), make()
    D, k = a.obs_dim, a.dims['null']
    acts = torch.rand((T, B, k), device=DEV, generator=torch.Generator(device=DEV).manual_seed(6)) * 2 - 1
    recs = torch.zeros((T + 1, B, D + k + 3), device=DEV)
    ends = torch.zeros(((T - 1) * B, D + 2), device=DEV)
    cnt = torch.full((1,), 12345, device=DEV, dtype=torch.int32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        rc = b._lib.atacom_rollout_compact(b._h, T, acts.data_ptr(), None, None, recs.data_ptr(), B, ends.data_ptr(),
                                           ends.shape[0], cnt.data_ptr(), s.cuda_stream)
    assert rc == 0
    graph.replay()
    torch.cuda.synchronize()
    n = int(cnt.item())
    rec_ref, ends_ref, n_ref = a.rollout_compact(actions=acts)
    assert n == n_ref and torch.equal(recs, rec_ref)
    key = lambda e: e[torch.argsort(e[:, 0] * B + e[:, 1])]        # noqa: E731  (rows are appended in no fixed order)
    assert torch.equal(key(ends[:n]), key(ends_ref))
    for e in (a, b):
        e.close()


def _rccl_compact_worker(port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    import torch.distributed as dist
    dev = torch.device(DEV)
    torch.cuda.set_device(dev)
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    try:
        from rl_on_manifold_amd.rollout import RolloutCollector
        B, T = 2048, 40
        ok = []
        for how in ('actions', 'policy', 'async'):
            res = {}
            for fmt in ('full', 'compact'):
                env = _env('iiwa', B, horizon=15, auto_reset=True, random_init=True, seed=8)
                g = torch.Generator(device=DEV).manual_seed(7)
                acts = torch.rand((T, B, 5), device=DEV, generator=g) * 2 - 1
                col = RolloutCollector(env, force_collective=True, record_format=fmt)
                if how == 'actions':
                    data = col.collect(T, actions=acts)
                elif how == 'policy':
                    data = col.collect(T, policy=_policy(18, 5, torch.float32), noise=acts)
                else:
                    data = col.collect_async(T, actions=acts).wait()
                res[fmt] = ({k_: v.clone() for k_, v in data.items()}, col.last_gather_bytes)
                env.close()
            ok.append(all(torch.equal(res['full'][0][k_], res['compact'][0][k_]) for k_ in KEYS))
            ok.append(res['compact'][1] < res['full'][1])
        q.put(ok)
    finally:
        dist.destroy_process_group()


def test_compact_collector_over_rccl_world_1():
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_compact_worker, args=(31800 + (os.getpid() % 1000), q))
    p.start()
    ok = q.get(timeout=600)
    p.join(timeout=120)
    assert p.exitcode == 0
    assert all(ok), ok


def _gloo_worker(rank, world, port, gb, T, fmt, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from rl_on_manifold_amd.rollout import RolloutCollector, shard_bounds
        lo, hi = shard_bounds(gb, world, rank)
        env = _env('planar', hi - lo, horizon=6, auto_reset=True)
        g = torch.Generator().manual_seed(9)
        acts = (torch.rand((T, gb, 3), generator=g) * 2 - 1)[:, lo:hi].to(DEV)
        col = RolloutCollector(env, global_batch=gb, record_format=fmt)
        data = col.time_major(col.collect(T, actions=acts))
        q.put((rank, fmt, {k_: v.cpu().numpy() for k_, v in data.items()}, col.last_gather_bytes))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_compact_collector_two_processes_sharing_the_gpu():
    """Two ranks (ragged shards 6 + 5) with their own HIP engines on one GPU over gloo: the compact collection equals the full
    one, and both equal a single-process run."""
    import torch.multiprocessing as mp
    from rl_on_manifold_amd.rollout import RolloutCollector
    gb, T, world = 11, 13, 2
    ctx = mp.get_context('spawn')
    results = {}
    for i, fmt in enumerate(('full', 'compact')):
        q = ctx.Queue()
        port = 32800 + (os.getpid() % 1000) + 7 * i
        procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, gb, T, fmt, q)) for r in range(world)]
        for p in procs:
            p.start()
        for _ in range(world):
            rank, f, data, nbytes = q.get(timeout=300)
            results[(f, rank)] = (data, nbytes)
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    env = _env('planar', gb, horizon=6, auto_reset=True)
    g = torch.Generator().manual_seed(9)
    acts = (torch.rand((T, gb, 3), generator=g) * 2 - 1).to(DEV)
    ref = RolloutCollector(env).time_major(RolloutCollector(env).collect(T, actions=acts))
    for rank in range(world):
        for key in KEYS:
            assert np.array_equal(results[('compact', rank)][0][key], results[('full', rank)][0][key]), (rank, key)
            assert np.array_equal(results[('compact', rank)][0][key], ref[key].cpu().numpy()), (rank, key)
        # shards padded to 6 envs: (T + 1) 6 (12 + 3 + 3) + max(n_ends) (12 + 2) floats
        last = ref['last'][:T - 1].cpu()
        m = max(int(last[:, :6].sum()), int(last[:, 6:].sum()))
        assert m > 0
        assert results[('compact', rank)][1] == ((T + 1) * 6 * 18 + m * 14) * 4
        assert results[('full', rank)][1] == T * 6 * 30 * 4


def test_config5_compact_rehearsal_eight_shards_on_one_gpu():
    """BASELINE config 5 in the compact format: every one of the 8 x 8192 x 120 iiwa shards, collected through a compact
    RolloutCollector, unpacks to exactly its full-format run, and a rank's payload is at most 110 MB (full: 173 MB)."""
    sys.path.insert(0, ROOT)
    import bench
    from rl_on_manifold_amd import RecordLayout
    from rl_on_manifold_amd.rollout import RolloutCollector
    W, B, T = 8, 8192, 120

    def shard(r):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(1234 + r)
        env, init, _ = bench.make_env('iiwa', B, torch.device(DEV), gen)
        return env, torch.rand((T, B, 5), device=DEV, generator=gen) * 2 - 1

    counts, sent = [], []
    for r in range(W):
        env, acts = shard(r)
        full = env.rollout_packed(actions=acts)
        ref = RecordLayout([B], env.obs_dim, 5).unpack(full)
        env.close()
        env, acts = shard(r)
        col = RolloutCollector(env, record_format='compact')
        g = col.gather(col.collect_local(T, actions=acts))
        got = col.unpack(g)
        for key in KEYS:
            assert torch.equal(got[key][0], ref[key]), (r, key)
        counts.append(g.n_ends[0])
        sent.append(col.last_gather_bytes)
        assert col.last_gather_bytes == ((T + 1) * B * 26 + g.n_ends[0] * 20) * 4
        assert g.n_ends[0] == int(ref['last'][:T - 1].sum())
        del full, ref, got, g
        env.close()
    print('config 5 compact: n_ends per shard %s; bytes sent per rank %s (full format: %d)'
          % (counts, sent, T * B * 44 * 4))
    assert max(sent) <= 110e6, sent
