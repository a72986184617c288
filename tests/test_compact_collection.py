"""The compact record format on the CPU: CompactRecordLayout.unpack rebuilds RecordLayout.unpack of the full format bit for
bit, and a RolloutCollector with record_format='compact' returns the dataset of the full format (gloo worlds of 2, 3 and 8
ranks over the float64 oracle engine), sending (T + 1) Bm (D + k + 3) + max(n_ends) (D + 2) floats per rank."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from rl_on_manifold_amd.rollout import (CompactRecordLayout, RecordLayout, RolloutCollector,   # noqa: E402
                                        shard_bounds)

KEYS = ('obs', 'action', 'reward', 'next_obs', 'absorbing', 'last')


def _synthetic(sizes, D, k, T, dtype, seed, end_at_last_step=True):
    """A full-format gather [W, T, Bm, F] whose next_obs repeats the next obs except at episode ends, and the compact form
    of the same data: records [W, T + 1, Bm, Fc] and the necessary exception rows per rank."""
    g = torch.Generator().manual_seed(seed)
    W, Bm = len(sizes), max(sizes)
    obs = torch.randn((W, T, Bm, D), generator=g, dtype=dtype)
    act = torch.randn((W, T, Bm, k), generator=g, dtype=dtype)
    rew = torch.randn((W, T, Bm), generator=g, dtype=dtype)
    last = torch.rand((W, T, Bm), generator=g) < 0.2
    if end_at_last_step:
        last[:, T - 1, 0] = True                         # an end at t = T-1: its terminal obs is the tail
    ab = last & (torch.rand((W, T, Bm), generator=g) < 0.5)
    term = torch.randn((W, T, Bm, D), generator=g, dtype=dtype)
    nobs = torch.empty_like(obs)
    nobs[:, :T - 1] = obs[:, 1:]
    nobs[:, T - 1] = term[:, T - 1]
    nobs[last] = term[last]
    valid = (torch.arange(Bm)[None, :] < torch.tensor(sizes)[:, None])[:, None, :].expand(W, T, Bm)
    for x in (obs, act, nobs, term):
        x[~valid] = 0
    rew[~valid] = 0
    last &= valid
    ab &= valid
    F = 2 * D + k + 3
    full = torch.zeros((W, T, Bm, F), dtype=dtype)
    full[..., :D], full[..., D:D + k], full[..., D + k] = obs, act, rew
    full[..., D + k + 1:2 * D + k + 1] = nobs
    full[..., 2 * D + k + 1], full[..., 2 * D + k + 2] = ab.to(dtype), last.to(dtype)
    Fc = D + k + 3
    rec = torch.zeros((W, T + 1, Bm, Fc), dtype=dtype)
    rec[:, :T, :, :D], rec[:, :T, :, D:D + k], rec[:, :T, :, D + k] = obs, act, rew
    rec[:, :T, :, D + k + 1], rec[:, :T, :, D + k + 2] = ab.to(dtype), last.to(dtype)
    rec[:, T, :, :D] = nobs[:, T - 1]
    ends = []
    for r in range(W):
        tb = torch.nonzero(last[r, :T - 1])
        e = torch.zeros((tb.shape[0], D + 2), dtype=dtype)
        e[:, 0], e[:, 1] = tb[:, 0].to(dtype), tb[:, 1].to(dtype)
        e[:, 2:] = nobs[r, tb[:, 0], tb[:, 1]]
        ends.append(e)
    return full, rec, ends, nobs


def _stack_ends(ends, D, pad_value=0.0, extra=0):
    M = max(e.shape[0] for e in ends) + extra
    out = torch.full((len(ends), M, D + 2), pad_value, dtype=ends[0].dtype)
    for r, e in enumerate(ends):
        out[r, :e.shape[0]] = e
    return out, [e.shape[0] for e in ends]


def _assert_same(a, b):
    for key in KEYS:
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, key
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('sizes', [[4], [3, 2, 2], [2, 2, 1, 1, 1, 1, 1, 1]])
def test_compact_unpack_equals_full_unpack(sizes, dtype):
    D, k, T = 5, 2, 7
    full, rec, ends, _ = _synthetic(sizes, D, k, T, dtype, seed=len(sizes))
    ref = RecordLayout(sizes, D, k).unpack(full)
    lay = CompactRecordLayout(sizes, D, k, T)
    assert lay.Fc == D + k + 3 and lay.record_numel == (T + 1) * max(sizes) * lay.Fc
    # rows past a rank's count hold garbage (NaN): they must not be read
    e, n = _stack_ends(ends, D, pad_value=float('nan'), extra=2)
    got = lay.unpack(rec, e, n)
    _assert_same(got, ref)
    # every field but next_obs is a view into the records
    for key in ('obs', 'action', 'reward'):
        assert got[key].data_ptr() >= rec.data_ptr() and got[key]._base is not None
    # time_major and valid_mask behave as in the full layout
    _assert_same(lay.time_major(got), RecordLayout(sizes, D, k).time_major(ref))
    assert torch.equal(lay.valid_mask(), RecordLayout(sizes, D, k).valid_mask())


def test_compact_unpack_end_at_the_last_step_comes_from_the_tail():
    D, k, T = 4, 1, 5
    full, rec, ends, nobs = _synthetic([3], D, k, T, torch.float64, seed=3)
    assert bool(full[0, T - 1, 0, 2 * D + k + 2] > 0.5)        # last at t = T-1 ...
    assert all(float(r[0]) < T - 1 for r in ends[0])           # ... and no exception row lists it
    got = CompactRecordLayout([3], D, k, T).unpack(rec[0], ends[0], ends[0].shape[0])     # the one-rank form
    assert torch.equal(got['next_obs'][T - 1], nobs[0, T - 1])
    _assert_same(got, RecordLayout([3], D, k).unpack(full[0]))


def test_compact_unpack_ignores_the_order_of_the_rows_and_accepts_a_superset():
    sizes, D, k, T = [3, 2, 2], 6, 3, 9
    full, rec, ends, nobs = _synthetic(sizes, D, k, T, torch.float32, seed=11)
    ref = RecordLayout(sizes, D, k).unpack(full)
    lay = CompactRecordLayout(sizes, D, k, T)
    g = torch.Generator().manual_seed(5)
    permuted = [e[torch.randperm(e.shape[0], generator=g)] for e in ends]
    e, n = _stack_ends(permuted, D)
    _assert_same(lay.unpack(rec, e, n), ref)
    # a superset: every row of a rank listed (whether or not an episode ended there), some twice
    sup = []
    for r, size in enumerate(sizes):
        tb = torch.cartesian_prod(torch.arange(T - 1), torch.arange(size))
        tb = torch.cat([tb, tb[::3]])
        rows = torch.zeros((tb.shape[0], D + 2), dtype=torch.float32)
        rows[:, 0], rows[:, 1] = tb[:, 0].float(), tb[:, 1].float()
        rows[:, 2:] = nobs[r, tb[:, 0], tb[:, 1]]
        sup.append(rows[torch.randperm(rows.shape[0], generator=g)])
    e, n = _stack_ends(sup, D)
    _assert_same(lay.unpack(rec, e, n), ref)


def test_compact_unpack_refuses_rows_outside_the_records():
    D, k, T = 4, 1, 5
    _, rec, ends, _ = _synthetic([2], D, k, T, torch.float64, seed=2)
    bad = torch.zeros((1, D + 2), dtype=torch.float64)
    bad[0, 0] = T
    with pytest.raises(ValueError, match='outside'):
        CompactRecordLayout([2], D, k, T).unpack(rec[0], bad, 1)


def test_record_format_is_validated():
    from oracle_engine import OracleEngine
    with pytest.raises(ValueError, match='record_format'):
        RolloutCollector(OracleEngine('circle', 2, horizon=4), record_format='small')


GLOBAL_B, T, NAME = 10, 10, 'planar'       # horizon 5: episodes end at t = 4 (an exception row) and t = 9 = T-1 (the tail)


def _actions():
    rng = np.random.default_rng(42)
    return rng.uniform(-1.2, 1.2, (T, GLOBAL_B, 3))


def _init_q():
    from oracle import robots
    rng = np.random.default_rng(7)
    return robots.PLANAR_INIT_Q + rng.normal(0, 0.05, (GLOBAL_B, 3))


def _policy(obs):
    return torch.tanh(3.0 * obs[:, 6:9] - obs[:, :3])           # deterministic in the observation


def _collect_both(lo, hi, how):
    """The same collection in both formats on fresh engines: (full dataset, compact dataset, collector, gathered)."""
    from oracle_engine import OracleEngine
    res = []
    for fmt in ('full', 'compact'):
        eng = OracleEngine(NAME, hi - lo, init_q=_init_q()[lo:hi], horizon=5)
        col = RolloutCollector(eng, global_batch=GLOBAL_B, record_format=fmt)
        if how == 'actions':
            g = col.gather(col.collect_local(T, actions=_actions()[:, lo:hi]))
            data = col.unpack(g)
        elif how == 'policy':
            g = col.gather(col.collect_local(T, policy=_policy))
            data = col.unpack(g)
        else:
            g = None
            data = col.collect_async(T, actions=_actions()[:, lo:hi]).wait()
        res.append((data, col, g))
    return res


def _compact_worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        lo, hi = shard_bounds(GLOBAL_B, world, rank)
        out = {}
        for how in ('actions', 'policy', 'async'):
            (full, fcol, _), (comp, ccol, g) = _collect_both(lo, hi, how)
            tf, tc = fcol.time_major(full), ccol.time_major(comp)
            same = all(torch.equal(full[k_], comp[k_]) and torch.equal(tf[k_], tc[k_]) for k_ in KEYS)
            shapes = all(full[k_].shape == comp[k_].shape and full[k_].dtype == comp[k_].dtype for k_ in KEYS)
            item = {'same': same and shapes, 'full_bytes': fcol.last_gather_bytes, 'bytes': ccol.last_gather_bytes,
                    'last': tf['last'].numpy(), 'Bm': ccol.Bm, 'D': ccol.D, 'k': ccol.k}
            if g is not None:
                item['n_ends'] = list(g.n_ends)
            out[how] = item
        q.put((rank, out))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3, 8])       # 8: config 5's shard count (ragged: 10 envs over 8 ranks)
def test_gloo_compact_collection_equals_full(world):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 2000) + world
    procs = [ctx.Process(target=_compact_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    sizes = [shard_bounds(GLOBAL_B, world, r)[1] - shard_bounds(GLOBAL_B, world, r)[0] for r in range(world)]
    for rank, out in results:
        for how, it in out.items():
            assert it['same'], (rank, how)
            Bm, D, k = it['Bm'], it['D'], it['k']
            # the exception counts: every last row before the final step of each rank's block (the host packer's superset)
            last = it['last']
            blocks = np.split(last[:T - 1], np.cumsum(sizes)[:-1], axis=1)
            counts = [int(b.sum()) for b in blocks]
            assert max(counts) > 0 and last[T - 1].all()            # ends inside the rollout and at its last step
            if 'n_ends' in it:
                assert it['n_ends'] == counts
            assert it['bytes'] == ((T + 1) * Bm * (D + k + 3) + max(counts) * (D + 2)) * 8
            assert it['full_bytes'] == T * Bm * (2 * D + k + 3) * 8


def test_compact_collection_without_a_process_group():
    """World of one, no collective: the compact dataset is the full one, and a short T = 1 collection (no exception rows
    possible) works too."""
    from oracle_engine import OracleEngine
    for n_steps in (T, 1):
        acts = _actions()[:n_steps]
        runs = {}
        for fmt in ('full', 'compact'):
            col = RolloutCollector(OracleEngine(NAME, GLOBAL_B, init_q=_init_q(), horizon=5), record_format=fmt)
            g = col.gather(col.collect_local(n_steps, actions=acts))
            runs[fmt] = (col.unpack(g), col.last_gather_bytes, g)
        _assert_same(runs['compact'][0], runs['full'][0])
        n = runs['compact'][2].n_ends[0]
        assert n == (GLOBAL_B if n_steps == T else 0)
        assert runs['compact'][1] == ((n_steps + 1) * GLOBAL_B * 18 + n * 14) * 8     # planar: D = 12, k = 3
