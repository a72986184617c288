"""GPU tests of libatacom_returns.so (rl_on_manifold_amd/returns.py): advantages and returns against the float64 oracle inside
its forward error bound on EVERY sample, the same data through four memory layouts and three flag types bit for bit, the
normalisation (statistics, reproducibility, application), the episode returns, real full and compact collections of two tasks,
a buffer filled block by block by three engines, and graph capture.  Shapes are the smallest at which the kernels can go wrong:
one step and one environment, sizes around the 64-lane block, more steps than two load-ahead buffers hold, ragged blocks."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import returns_oracle as ro                                  # noqa: E402
from returns_cases import GAMMA_LAM, PATTERNS, make_case, ragged_sizes      # noqa: E402

DEV = 'cuda:0'
DT = {'f32': torch.float32, 'f64': torch.float64}
NP = {'f32': np.float32, 'f64': np.float64}
STEPS, ENVS = (1, 2, 7, 33), (1, 63, 65, 257)


def _dev(x, dt):
    """A numpy array on the device: values in the call's dtype, flags as bool."""
    x = np.asarray(x)
    return torch.from_numpy(x.copy() if x.dtype == bool else x.astype(NP[dt])).to(DEV)


def _rounded(c, dt):
    """The case as the kernel receives it: values rounded to its dtype (the float64 reference gets these)."""
    return {k: (x if x.dtype == bool else x.astype(NP[dt])) for k, x in c.items()}


def _assert_inside(got, want, bound, what):
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), (what, 'worst |error| / bound %.3f on %d of %d samples' % (worst, int((err > bound).sum()), err.size))
    return worst


@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('dt', ['f64', 'f32'])
def test_gae_is_inside_the_bound_on_every_sample(dt, pattern, W):
    from rl_on_manifold_amd import compute_gae
    worst = 0.0
    for T in STEPS:
        for B in ENVS:
            c = _rounded(make_case(T, B, pattern, seed=11, W=W), dt)
            d = {k: _dev(x, dt) for k, x in c.items()}
            sizes = ragged_sizes(W, B) if W > 1 else None
            for gamma, lam in GAMMA_LAM:
                ret, adv = compute_gae(d['reward'], d['absorbing'], d['last'], d['v'], d['v_next'], gamma, lam, sizes=sizes)
                assert ret.shape == d['reward'].shape and ret.dtype == DT[dt] and ret.is_contiguous()
                want_ret, want_adv = ro.gae(gamma=gamma, lam=lam, **c)
                b_ret, b_adv = ro.gae_bound(gamma=gamma, lam=lam, eps=ro.EPS[dt], **c)
                what = (dt, pattern, W, T, B, gamma, lam)
                worst = max(worst, _assert_inside(adv, want_adv, b_adv, what + ('adv',)),
                            _assert_inside(ret, want_ret, b_ret, what + ('ret',)))
            # without a critic: lam = 1 is the discounted return-to-go
            ret, adv = compute_gae(d['reward'], d['absorbing'], d['last'], None, None, 0.99, 1.0)
            want_ret, want_adv = ro.gae(c['reward'], c['absorbing'], c['last'], None, None, 0.99, 1.0)
            b_ret, b_adv = ro.gae_bound(c['reward'], c['absorbing'], c['last'], None, None, 0.99, 1.0, ro.EPS[dt])
            _assert_inside(adv, want_adv, b_adv, (dt, pattern, W, T, B, 'v = None'))
            assert torch.equal(ret, adv)
    print('%s %s W %d: worst |error| / bound %.3f' % (dt, pattern, W, worst))


def test_plain_two_dimensional_arrays_and_caller_outputs():
    from rl_on_manifold_amd import compute_gae
    c = _rounded(make_case(33, 65, 'consecutive_ends', seed=12), 'f32')
    d = {k: _dev(x[0], 'f32') for k, x in c.items()}
    ret, adv = compute_gae(d['reward'], d['absorbing'], d['last'], d['v'], d['v_next'], 0.99, 0.95)
    assert ret.shape == (33, 65)
    out = (torch.full((33, 65), float('nan'), device=DEV), torch.full((33, 65), float('nan'), device=DEV))
    got = compute_gae(d['reward'], d['absorbing'], d['last'], d['v'], d['v_next'], 0.99, 0.95, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    assert torch.equal(out[0], ret) and torch.equal(out[1], adv)
    ret3, adv3 = compute_gae(*(d[k][None] for k in ('reward', 'absorbing', 'last', 'v', 'v_next')), 0.99, 0.95)
    assert torch.equal(ret3[0], ret) and torch.equal(adv3[0], adv)
    with pytest.raises(ValueError, match='contiguous'):
        compute_gae(d['reward'], d['absorbing'], d['last'], d['v'], d['v_next'], 0.99, 0.95, out=(out[0], out[1].t()))
    for bad in ((out[0], out[0]), (d['v'], out[1]), (out[0], d['reward']), (out[0], d['v_next'])):
        with pytest.raises(ValueError, match='overlap'):
            compute_gae(d['reward'], d['absorbing'], d['last'], d['v'], d['v_next'], 0.99, 0.95, out=bad)
    with pytest.raises(ValueError, match='must be a torch.float32'):
        compute_gae(d['reward'], d['absorbing'], d['last'], d['v'].double(), d['v_next'].double(), 0.99, 0.95)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_four_layouts_and_three_flag_types_give_the_same_bits(dt):
    """Contiguous arrays, the columns of full records, the columns of compact records (v a view of [W, T + 1, Bm]) and tensors
    with a non-unit environment stride; flags as bool, uint8 and in the value dtype."""
    from rl_on_manifold_amd import compute_gae, compute_J
    from rl_on_manifold_amd.rollout import compact_record_fields, record_columns, record_fields
    D, k = 3, 2
    for T, B, W in ((1, 1, 1), (7, 65, 3), (33, 63, 3), (2, 257, 1)):
        c = _rounded(make_case(T, B, 'consecutive_ends', seed=13, W=W), dt)
        d = {k_: _dev(x, dt) for k_, x in c.items()}
        sizes = ragged_sizes(W, B)
        names = ('reward', 'absorbing', 'last', 'v', 'v_next')
        ref = compute_gae(*(d[n] for n in names), 0.99, 0.95, sizes=sizes)
        ref_j = compute_J(d['reward'], d['last'], 0.99, sizes=sizes)
        flags = lambda cast: dict(d, absorbing=cast(d['absorbing']), last=cast(d['last']))      # noqa: E731
        variants = {'uint8 flags': flags(lambda f: f.to(torch.uint8)), 'value flags': flags(lambda f: f.to(DT[dt]))}
        # full records [W, T, B, F]
        fields, F = record_fields(D, k)
        g = torch.randn((W, T, B, F), device=DEV, dtype=DT[dt])
        for n in ('reward', 'absorbing', 'last'):
            g[..., fields[n]] = d[n].to(DT[dt])
        variants['full records'] = dict(record_columns(g, {n: fields[n] for n in ('reward', 'absorbing', 'last')}), v=d['v'],
                                        v_next=d['v_next'])
        # compact records [W, T + 1, B, Fc], v as the first T rows of [W, T + 1, B]
        cf, Fc, _ = compact_record_fields(D, k)
        rec = torch.randn((W, T + 1, B, Fc), device=DEV, dtype=DT[dt])
        for n in ('reward', 'absorbing', 'last'):
            rec[:, :T, :, cf[n]] = d[n].to(DT[dt])
        v_tail = torch.cat([d['v'], torch.randn((W, 1, B), device=DEV, dtype=DT[dt])], 1)
        variants['compact records'] = dict(record_columns(rec[:, :T], {n: cf[n] for n in ('reward', 'absorbing', 'last')}),
                                           v=v_tail[:, :T], v_next=d['v_next'])
        # a non-unit environment stride: every second column of [W, T, 2 B], and the environment axis outermost
        def strided(x):
            wide = torch.zeros((W, T, 2 * B), device=DEV, dtype=x.dtype)
            wide[..., ::2] = x
            return wide[..., ::2]
        variants['every second column'] = {n: strided(d[n]) for n in names}
        variants['environment-major storage'] = {n: d[n].permute(0, 2, 1).contiguous().permute(0, 2, 1) for n in names}
        for name, x in variants.items():
            got = compute_gae(*(x[n] for n in names), 0.99, 0.95, sizes=sizes)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (dt, T, B, W, name)
            got_j = compute_J(x['reward'], x['last'], 0.99, sizes=sizes)
            assert torch.equal(got_j[0], ref_j[0]) and torch.equal(got_j[1], ref_j[1]), (dt, T, B, W, name)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_normalisation(dt):
    from rl_on_manifold_amd import compute_gae, normalize_advantages
    names = ('reward', 'absorbing', 'last', 'v', 'v_next')
    for T, B, W in ((33, 65, 3), (7, 257, 3), (1, 63, 1), (2, 1, 3)):
        c = _rounded(make_case(T, B, 'consecutive_ends', seed=14, W=W), dt)
        d = {k: _dev(x, dt) for k, x in c.items()}
        sizes = ragged_sizes(W, B)
        if B == 1:
            sizes = [1] * W
        raw_ret, raw = compute_gae(*(d[n] for n in names), 0.99, 0.95, sizes=sizes)
        ret, adv, stats = compute_gae(*(d[n] for n in names), 0.99, 0.95, sizes=sizes, normalize=True)
        ret2, adv2, stats2 = compute_gae(*(d[n] for n in names), 0.99, 0.95, sizes=sizes, normalize=True)
        assert torch.equal(ret, raw_ret) and torch.equal(ret2, raw_ret)
        assert stats.dtype == torch.float64 and stats.shape == (3,)
        assert torch.equal(stats, stats2) and torch.equal(adv, adv2)                # the same bits on two runs
        alone = raw.clone()
        assert torch.equal(normalize_advantages(alone, sizes=sizes), stats) and torch.equal(alone, adv)
        # the statistics against float64 numpy over the real rows
        a = raw.cpu().numpy().astype(np.float64)
        real = ro.valid_rows(a.shape, sizes)
        _, want = ro.normalize(a, sizes)
        d_mean, d_std = ro.stats_bound(a, sizes)
        count, mean, std = stats.cpu().numpy()
        assert count == want[0] == T * sum(sizes)
        assert abs(mean - want[1]) <= d_mean, (dt, T, B, W, mean - want[1], d_mean)
        assert abs(std - want[2]) <= d_std, (dt, T, B, W, std - want[2], d_std)
        # the application, recomputed from the statistics as they are returned: inside the issue's 2 eps |adv - mean| / (std + 1e-8),
        # and -- the kernel does the subtraction and the division in double and rounds once -- the same bits
        expect = (a - mean) / (std + 1e-8)
        got = adv.cpu().numpy().astype(np.float64)
        assert np.array_equal(got[~real], a[~real])                                  # padding rows are left as they are
        assert (np.abs(got - expect)[real] <= 2 * ro.EPS[dt] * np.abs(expect)[real]).all(), (dt, T, B, W)
        assert np.array_equal(adv.cpu().numpy()[real], expect.astype(NP[dt])[real]), (dt, T, B, W)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_episode_returns(dt):
    """compute_J against the oracle, with trailing unfinished episodes and padding rows; gamma = 1 gives R."""
    from rl_on_manifold_amd import compute_J, episode_returns
    u = 2.0 ** -53
    for T, B, W in ((33, 65, 3), (7, 257, 1), (1, 1, 1), (2, 63, 3)):
        for pattern in ('consecutive_ends', 'no_last', 'last_everywhere'):
            c = _rounded(make_case(T, B, pattern, seed=15, W=W), dt)
            r, last = _dev(c['reward'], dt), _dev(c['last'], dt)
            sizes = ragged_sizes(W, B) if W > 1 else None
            for gamma in (0.99, 1.0, 0.0):
                got = episode_returns(r, last, gamma, sizes=sizes).cpu().numpy()
                want, js = ro.episode_sums(c['reward'], c['last'], gamma, sizes)
                bounds = []
                for w in range(W):
                    n = B if sizes is None else sizes[w]
                    bounds += ro.episodes_in_dtype(c['reward'][w][:, :n], c['last'][w][:, :n], gamma, NP[dt])[1] if n else []
                bounds = np.asarray(bounds)
                assert got[1] == want[1] == len(js)
                assert abs(got[0] - want[0]) <= bounds.sum() + u * len(js) * np.abs(js).sum(), (dt, T, B, W, pattern, gamma)
                assert abs(got[2] - want[2]) <= (2 * np.abs(js) * bounds + bounds ** 2).sum() + u * (len(js) + 2) * (js * js).sum()
                mean, n_ep = compute_J(r, last, gamma, sizes=sizes)
                assert float(n_ep) == want[1] and float(mean) == got[0] / got[1]
    r = torch.tensor([[1.0], [2.0], [4.0], [3.0], [8.0], [16.0], [5.0]], device=DEV, dtype=DT[dt])
    last = torch.tensor([[0], [0], [1], [0], [1], [0], [0]], device=DEV, dtype=torch.bool)
    assert episode_returns(r, last, 0.5).tolist() == [28.5, 3.0, 9.0 + 49.0 + 18.5 ** 2]
    assert episode_returns(r, last).tolist() == [39.0, 3.0, 49.0 + 121.0 + 441.0]


def _critic(obs):
    return 0.5 * obs[..., 0] + obs[..., 1]            # elementwise: its bits do not depend on the batch shape


def _twin_collections(make, T, k, seed, stride=None):
    """The same seed collected once as full packed records and once compact -> (full, (records, ends, n), D)."""
    a, b = make(), make()
    a.reset()
    st = a.get_state()
    a.set_state(st)
    b.set_state(st)
    acts = torch.rand((T, a.batch, k), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * 2 - 1
    full = a.rollout_packed(actions=acts, batch_stride=stride)
    rec, ends, n = b.rollout_compact(actions=acts, batch_stride=stride)
    D = a.obs_dim
    for e in (a, b):
        e.close()
    return full, (rec, ends.clone(), n), D


@pytest.mark.parametrize('task', ['point_reach', 'circle'])
def test_full_and_compact_collections_of_a_real_task_agree_bit_for_bit(task):
    from rl_on_manifold_amd import (BatchedAtacomEnv, BatchedPointReachEnv, CompactRecordLayout, RecordLayout, compute_gae,
                                    compute_J, gae_from_compact, gae_from_records)
    B, T, gamma, lam = 96, 12, 0.99, 0.95
    if task == 'point_reach':
        make, k = (lambda: BatchedPointReachEnv(B, n_objects=2, horizon=5, auto_reset=True, seed=3, device=DEV)), 2
    else:
        make, k = (lambda: BatchedAtacomEnv('circle', B, horizon=5, auto_reset=True, device=DEV)), None
    if k is None:
        probe = make()
        k = probe.dims['null']
        probe.close()
    full, (rec, ends, n), D = _twin_collections(make, T, k, seed=16)
    lay, clay = RecordLayout([B], D, k), CompactRecordLayout([B], D, k, T)
    dfull, dcomp = lay.unpack(full), clay.unpack(rec, ends, n)
    assert int(dfull['last'].sum()) >= 2 * B and n >= B                     # horizon 5: two ends per environment, one exception row
    # from the records in place
    v, vn = _critic(full[..., lay.fields['obs']]), _critic(full[..., lay.fields['next_obs']])
    a = gae_from_records(lay, full, v, vn, gamma, lam)
    v_c, v_e = _critic(rec[..., clay.compact_fields['obs']]), _critic(ends[:, 2:])
    assert v_c.shape == (T + 1, B) and v_e.shape == (n,)
    b = gae_from_compact(clay, rec, ends, n, v_c, v_e, gamma, lam)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # from the unpacked dicts
    for d in (dfull, dcomp):
        c = compute_gae(d['reward'], d['absorbing'], d['last'], _critic(d['obs']), _critic(d['next_obs']), gamma, lam)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    # ... and inside the oracle's bound
    args = [x.cpu().numpy().astype(np.float64) for x in (dfull['reward'], dfull['absorbing'], dfull['last'], v, vn)]
    want_ret, want_adv = ro.gae(*args, gamma, lam)
    b_ret, b_adv = ro.gae_bound(*args, gamma, lam, ro.EPS['f32'])
    _assert_inside(a[1], want_adv, b_adv, (task, 'adv'))
    _assert_inside(a[0], want_ret, b_ret, (task, 'ret'))
    # normalised, and the episode returns, across the three
    na, nb = gae_from_records(lay, full, v, vn, gamma, lam, normalize=True), gae_from_compact(clay, rec, ends, n, v_c, v_e, gamma, lam,
                                                                                                normalize=True)
    assert all(torch.equal(x, y) for x, y in zip(na, nb))
    for g_ in (gamma, 1.0):
        j = [compute_J(full[..., lay.fields['reward']], full[..., lay.fields['last']], g_),
             compute_J(rec[:T, :, clay.compact_fields['reward']], rec[:T, :, clay.compact_fields['last']], g_),
             compute_J(dfull['reward'], dfull['last'], g_), compute_J(dcomp['reward'], dcomp['last'], g_)]
        assert all(torch.equal(x[0], j[0][0]) and torch.equal(x[1], j[0][1]) for x in j[1:])
        want, js = ro.episode_sums(args[0][None], args[2][None], g_)
        assert float(j[0][1]) == want[1]
        assert abs(float(j[0][0]) - want[0] / want[1]) <= 2.0 ** -24 * (T + 2) * np.abs(args[0]).sum() / want[1]


def test_a_buffer_filled_block_by_block_by_three_engines():
    """[3, T, Bm, F] and [3, T + 1, Bm, Fc] with ragged blocks [5, 4, 4], each block written by an engine of its own."""
    from rl_on_manifold_amd import BatchedAtacomEnv, CompactRecordLayout, RecordLayout, gae_from_compact, gae_from_records
    sizes, T, gamma, lam = [5, 4, 4], 9, 0.99, 0.95
    Bm, W = max(sizes), len(sizes)
    probe = BatchedAtacomEnv('planar', 1, device=DEV)
    D, k = probe.obs_dim, probe.dims['null']
    probe.close()
    lay, clay = RecordLayout(sizes, D, k), CompactRecordLayout(sizes, D, k, T)
    g = torch.zeros((W, T, Bm, lay.F), device=DEV)
    rec = torch.zeros((W, T + 1, Bm, clay.Fc), device=DEV)
    cap = (T - 1) * Bm
    ends = torch.zeros((W, cap, clay.E), device=DEV)
    counts = []
    for r, size in enumerate(sizes):
        acts = torch.rand((T, size, k), device=DEV, generator=torch.Generator(device=DEV).manual_seed(20 + r)) * 2 - 1
        a = BatchedAtacomEnv('planar', size, horizon=4, auto_reset=True, device=DEV)
        b = BatchedAtacomEnv('planar', size, horizon=4, auto_reset=True, device=DEV)
        a.rollout_packed(actions=acts, out=g[r], batch_stride=Bm)
        counts.append(b.rollout_compact(actions=acts, out=(rec[r], ends[r]), batch_stride=Bm, ends_capacity=cap)[2])
        a.close()
        b.close()
    d = lay.unpack(g)
    v, vn = _critic(d['obs']), _critic(d['next_obs'])
    x = gae_from_records(lay, g, v, vn, gamma, lam, normalize=True)
    y = gae_from_compact(clay, rec, ends, counts, _critic(rec[..., clay.compact_fields['obs']]), _critic(ends[..., 2:]), gamma, lam,
                         normalize=True)
    assert all(torch.equal(p, q) for p, q in zip(x, y))
    args = [t.cpu().numpy().astype(np.float64) for t in (d['reward'], d['absorbing'], d['last'], v, vn)]
    want_ret, want_adv = ro.gae(*args, gamma, lam)
    b_ret, _ = ro.gae_bound(*args, gamma, lam, ro.EPS['f32'])
    _assert_inside(x[0], want_ret, b_ret, 'ret')
    count, mean, std = x[2].tolist()
    assert count == T * sum(sizes)
    real = ro.valid_rows(want_adv.shape, sizes)
    assert abs(mean - want_adv[real].mean()) <= 1e-5 * np.abs(want_adv[real]).mean() and abs(std - want_adv[real].std()) <= 1e-5 * std
    assert (x[1].cpu().numpy()[~real] == 0).all()                               # padding rows: zero records in, zeros out


def test_graph_capture_and_replay():
    """compute_gae(..., normalize=True, out=...) captured once on one stream, replayed twice with new inputs: each replay gives the
    bits of the eager call."""
    from rl_on_manifold_amd import compute_gae
    T, B, W = 33, 65, 3
    sizes = ragged_sizes(W, B)
    names = ('reward', 'absorbing', 'last', 'v', 'v_next')
    cases = [{k: _dev(x, 'f32') for k, x in make_case(T, B, 'consecutive_ends', seed=30 + i, W=W).items()} for i in range(3)]
    static = {k: x.clone() for k, x in cases[0].items()}
    out = (torch.zeros((W, T, B), device=DEV), torch.zeros((W, T, B), device=DEV))
    compute_gae(*(static[n] for n in names), 0.99, 0.95, sizes=sizes, normalize=True, out=out)      # warm: the sizes are uploaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, _, stats = compute_gae(*(static[n] for n in names), 0.99, 0.95, sizes=sizes, normalize=True, out=out)
    for c in cases[1:]:
        for n in names:
            static[n].copy_(c[n])
        graph.replay()
        torch.cuda.synchronize()
        ret, adv, st = compute_gae(*(c[n] for n in names), 0.99, 0.95, sizes=sizes, normalize=True)
        assert torch.equal(out[0], ret) and torch.equal(out[1], adv) and torch.equal(stats, st)
