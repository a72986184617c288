"""GPU tests of libatacom_evaluate.so (rl_on_manifold_amd/evaluate.py): the network's output and the fused log-probability against
the float64 oracle, float32 inside its forward error bound on EVERY sample and float64 to 1e-12 of the output's scale; row counts
around the 16-row block and the 64-row tile, one and several tiles per workgroup; every CH = ceil(n_in / 4) path that differs;
columns of padded records read in place with NaN in the padding and poison around the outputs; mean and logp in one pass; real
full and compact collections through values_from_* into the advantage kernels; the collector kernel's own mean; graph capture.
Shapes are the smallest at which the kernels can go wrong."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluate_oracle as eo                                  # noqa: E402
import returns_oracle as ro                                   # noqa: E402

DEV = 'cuda:0'
DT = {'f32': torch.float32, 'f64': torch.float64}
NP = {'f32': np.float32, 'f64': np.float64}
_cache = {}


def _case(dt, case, seed=7):
    """(policy on the device, x, action, the oracle's (logp, e_logp, scale_logp, y, e_y), scale_y), computed once per case."""
    key = (dt, case, seed)
    if key not in _cache:
        from rl_on_manifold_amd import MlpPolicy
        net, x, action, std = eo.case_data(seed, *case, dtype=NP[dt])
        t = lambda a: None if a is None else torch.from_numpy(a).to(DEV)          # noqa: E731
        pol = MlpPolicy(*(t(net[k]) for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')), std=t(std), obs_shift=t(net['obs_shift']),
                        obs_scale=t(net['obs_scale']), activation=net['activation'])
        want = eo.log_prob(net, x, action, std)
        z = (action.astype(np.float64) - want[3]) / std
        assert np.abs(z).max() > 5.0 and np.abs(z).min() < 1e-3 or x.shape[0] < 8, 'the case must span z from 0 to about 6'
        _cache[key] = (pol, t(x), t(action), want, eo.forward(net, x)[2])
    return _cache[key]


def _inside(dt, got, want, e32, scale, what):
    """float32: |error| <= the oracle's bound; float64: <= 1e-12 scale + 1e-14.  -> the worst |error| / bound."""
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    bound = e32 if dt == 'f32' else 1e-12 * scale + 1e-14
    err = np.abs(got - want)
    worst = float((err / bound).max())
    print('%s %s: worst |error| / bound %.4f, worst |error| %.3g' % (what, dt, worst, err.max()))
    assert (err <= bound).all(), (what, dt, 'worst |error| / bound %.3f on %d of %d samples' % (worst, int((err > bound).sum()), err.size))
    return worst


def _check(dt, case, n_blocks=0):
    from rl_on_manifold_amd import evaluate_rows
    pol, x, action, (lp, e_lp, s_lp, y, e_y), s_y = _case(dt, case)
    got_y, got_lp = torch.full_like(action, float('nan')), torch.full((x.shape[0],), float('nan'), dtype=DT[dt], device=DEV)
    evaluate_rows(pol, x, action, y=got_y, logp=got_lp, n_blocks=n_blocks)
    _inside(dt, got_y, y, e_y, s_y, (case, n_blocks, 'y'))
    _inside(dt, got_lp, lp, e_lp, s_lp, (case, n_blocks, 'logp'))
    return got_y, got_lp


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('rows,n_blocks', eo.ROW_CASES)
def test_row_counts_and_grids(dt, rows, n_blocks):
    """1 .. 600 rows: a lone row, a part-filled 16-block, a tail wave, 200 rows walked by one and by two workgroups, and 600 by
    one, whose wavefronts walk two and three tiles."""
    case = eo.SHAPE_CASES[3][:4] + (rows,)
    got = _check(dt, case, n_blocks)
    if n_blocks:                                  # the result of a row does not depend on the grid
        auto = _check(dt, case, 0)
        assert torch.equal(got[0], auto[0]) and torch.equal(got[1], auto[1])


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('case', eo.SHAPE_CASES, ids=str)
def test_network_shapes(dt, case):
    """n_in 4 .. 32 (CH = 1, widths that are no multiple of 4, the maximum), n_out 1 .. 8, both activations, with and without the
    observation normalisation; z = (action - mean) / std from 0 to 6 at std from 1e-2 to 2."""
    from rl_on_manifold_amd import evaluate_mlp, gaussian_log_prob
    y, lp = _check(dt, case)
    pol, x, action = _case(dt, case)[:3]
    assert torch.equal(evaluate_mlp(pol, x), y) and torch.equal(gaussian_log_prob(pol, x, action), lp)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_mean_and_logp_of_one_call_are_those_of_two(dt):
    from rl_on_manifold_amd import evaluate_mlp, gaussian_log_prob
    case = eo.SHAPE_CASES[2]
    pol, x, action = _case(dt, case)[:3]
    mean = torch.empty_like(action)
    lp = gaussian_log_prob(pol, x, action, mean_out=mean)
    assert torch.equal(mean, evaluate_mlp(pol, x)) and torch.equal(lp, gaussian_log_prob(pol, x, action))
    out = torch.empty_like(mean)
    assert evaluate_mlp(pol, x, out=out) is out and torch.equal(out, mean)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_columns_of_padded_records_are_read_in_place_and_nothing_else_is_written(dt):
    """x and action as columns of [T = 3, batch_stride = 8 > B = 5, F] records whose padding rows and other columns hold NaN; y
    and logp into padded, poisoned buffers: the bits of the contiguous call, and not a byte outside the output views changes."""
    from rl_on_manifold_amd import evaluate_rows
    T, B, stride, n_in, n_out = 3, 5, 8, 18, 5
    case = (n_in, n_out, 'relu', False, T * B)
    pol, x, action = _case(dt, case)[:3]
    y0 = torch.empty((T * B, n_out), dtype=DT[dt], device=DEV)
    lp0 = torch.empty((T * B,), dtype=DT[dt], device=DEV)
    evaluate_rows(pol, x, action, y=y0, logp=lp0)
    F = n_in + n_out + 3
    rec = torch.full((T, stride, F), float('nan'), dtype=DT[dt], device=DEV)
    rec[:, :B, :n_in], rec[:, :B, n_in:n_in + n_out] = x.view(T, B, n_in), action.view(T, B, n_out)
    poison = 12345.0
    ybuf = torch.full((T, stride, n_out + 3), poison, dtype=DT[dt], device=DEV)
    lbuf = torch.full((T, stride, 2), poison, dtype=DT[dt], device=DEV)
    yv, lv = ybuf[:, :B, 1:1 + n_out], lbuf[:, :B, 1]
    evaluate_rows(pol, rec[:, :B, :n_in], rec[:, :B, n_in:n_in + n_out], y=yv, logp=lv)
    assert torch.equal(yv.reshape(T * B, n_out), y0) and torch.equal(lv.reshape(T * B), lp0)
    keep_y, keep_l = torch.ones_like(ybuf, dtype=torch.bool), torch.ones_like(lbuf, dtype=torch.bool)
    keep_y[:, :B, 1:1 + n_out], keep_l[:, :B, 1] = False, False
    assert bool((ybuf[keep_y] == poison).all()) and bool((lbuf[keep_l] == poison).all())
    # the inputs are inputs
    assert bool(torch.isnan(rec[:, B:]).all()) and torch.equal(rec[:, :B, :n_in].reshape(T * B, n_in), x)
    # a leading dimension that does not merge is walked: [2, T, B] views of two separate record buffers' worth of rows
    two = torch.full((2, T + 1, stride, F), float('nan'), dtype=DT[dt], device=DEV)
    two[:, :T] = rec
    y2 = torch.empty((2, T, B, n_out), dtype=DT[dt], device=DEV)
    evaluate_rows(pol, two[:, :T, :B, :n_in], y=y2)
    assert torch.equal(y2[0].reshape(T * B, n_out), y0) and torch.equal(y2[1], y2[0])


def _twin_collections(make, T, k, seed):
    """The same seed collected once as full packed records and once compact -> (full, (records, ends, n), D)."""
    a, b = make(), make()
    a.reset()
    st = a.get_state()
    a.set_state(st)
    b.set_state(st)
    acts = torch.rand((T, a.batch, k), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * 2 - 1
    full = a.rollout_packed(actions=acts)
    rec, ends, n = b.rollout_compact(actions=acts)
    D = a.obs_dim
    for e in (a, b):
        e.close()
    return full, (rec, ends.clone(), n), D


def test_values_of_full_and_compact_collections_feed_the_advantages_with_the_same_bits():
    """B = 32, T = 6, horizon 4 with auto-reset: every environment ends an episode at t = 3 < T - 1.  values_from_compact ->
    gae_from_compact and values_from_records -> gae_from_records give the same bits, inside the float32 bounds of the float64
    chain oracle critic -> oracle recurrence; the log-probability of the recorded actions reads both formats alike."""
    from rl_on_manifold_amd import (BatchedAtacomEnv, CompactRecordLayout, MlpPolicy, RecordLayout, gae_from_compact, gae_from_records,
                                    log_prob_from_records, values_from_compact, values_from_records)
    B, T, gamma, lam = 32, 6, 0.99, 0.95
    make = lambda: BatchedAtacomEnv('circle', B, horizon=4, auto_reset=True, device=DEV)      # noqa: E731
    probe = make()
    k = probe.dims['null']
    probe.close()
    full, (rec, ends, n), D = _twin_collections(make, T, k, seed=5)
    lay, clay = RecordLayout([B], D, k), CompactRecordLayout([B], D, k, T)
    d = lay.unpack(full)
    assert n >= B and bool(d['last'][:T - 1].any())
    rng = np.random.default_rng(11)
    cnet, anet = eo.random_net(rng, D, 1, 'tanh'), eo.random_net(rng, D, k, 'relu')
    std = np.full(k, 0.5, np.float32)
    t = lambda a: None if a is None else torch.from_numpy(a).to(DEV)          # noqa: E731
    mk = lambda net, s: MlpPolicy(*(t(net[q]) for q in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')), std=t(s), obs_shift=t(net['obs_shift']),      # noqa: E731
                                  obs_scale=t(net['obs_scale']), activation=net['activation'])
    critic, actor = mk(cnet, None), mk(anet, std)
    v, vn = values_from_records(lay, full, critic)
    v_c, v_e = values_from_compact(clay, rec, ends, n, critic)
    assert v.shape == vn.shape == (T, B) and v_c.shape == (T + 1, B) and v_e.shape == (n,)
    assert torch.equal(v_c[:T], v)
    a = gae_from_records(lay, full, v, vn, gamma, lam)
    b = gae_from_compact(clay, rec, ends, n, v_c, v_e, gamma, lam)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the float64 chain and its bound: the recurrence is linear in v and v_next, so their bounds travel through it, and the
    # recurrence's own rounding (returns_oracle.gae_bound) is added
    f64 = lambda x: x.cpu().numpy().astype(np.float64)                           # noqa: E731
    obs, nobs = f64(d['obs']).reshape(T * B, D), f64(d['next_obs']).reshape(T * B, D)
    (wv, ev, _), (wvn, evn, _) = eo.forward(cnet, obs), eo.forward(cnet, nobs)
    wv, ev, wvn, evn = (x.reshape(T, B) for x in (wv, ev, wvn, evn))
    _inside('f32', v, wv, ev, None, 'v')
    _inside('f32', vn, wvn, evn, None, 'v_next')
    r, ab, la = f64(d['reward']), f64(d['absorbing']), f64(d['last'])
    want_ret, want_adv = ro.gae(r, ab, la, wv, wvn, gamma, lam)
    b_ret, b_adv = ro.gae_bound(r, ab, la, wv, wvn, gamma, lam, ro.EPS['f32'])
    e_adv, carry = np.zeros((T, B)), np.zeros(B)
    for s in reversed(range(T)):
        carry = gamma * np.where(ab[s] > 0.5, 0.0, evn[s]) + ev[s] + gamma * lam * np.where(la[s] > 0.5, 0.0, carry)
        e_adv[s] = carry
    _inside('f32', a[1], want_adv, 1.001 * (b_adv + e_adv), None, 'adv')
    _inside('f32', a[0], want_ret, 1.001 * (b_ret + e_adv + ev), None, 'ret')
    # the log-probability of the recorded actions, from both formats
    lp = log_prob_from_records(lay, full, actor)
    assert lp.shape == (T, B) and torch.equal(lp, log_prob_from_records(clay, rec, actor))
    want = eo.log_prob(anet, obs, f64(d['action']).reshape(T * B, k), std)
    _inside('f32', lp.reshape(-1), want[0], want[1], None, 'logp')


def test_the_collector_kernels_own_mean():
    """On a zero-noise rollout_policy the recorded action is the collector kernel's mean of the recorded observation;
    evaluate_mlp agrees with it inside the bound (each is inside the oracle's bound, so they differ by at most two)."""
    from rl_on_manifold_amd import BatchedAtacomEnv, MlpPolicy, evaluate_mlp
    B, T = 64, 2
    env = BatchedAtacomEnv('planar', B, device=DEV, random_init=True, seed=2)
    D, k = env.obs_dim, env.dims['null']
    net = eo.random_net(np.random.default_rng(3), D, k, 'relu')
    t = lambda a: torch.from_numpy(a).to(DEV)          # noqa: E731
    pol = MlpPolicy(*(t(net[q]) for q in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')), std=None, obs_shift=t(net['obs_shift']),
                    obs_scale=t(net['obs_scale']))
    env.reset()
    d = env.rollout_policy(pol, T, noise=None)
    mean = evaluate_mlp(pol, d['obs'])
    env.close()
    y, e, _ = eo.forward(net, d['obs'].cpu().numpy().reshape(T * B, D))
    _inside('f32', mean.reshape(T * B, k), y, e, None, 'evaluate_mlp')
    _inside('f32', d['action'].reshape(T * B, k), y, e, None, 'the collector')
    diff = (mean - d['action']).abs().reshape(T * B, k).cpu().numpy()
    print('evaluate_mlp vs the collector kernel: bit-equal %s, worst difference %.3g' % (bool((diff == 0).all()), diff.max()))
    assert (diff <= 2 * e).all()


def test_graph_capture_and_replay():
    """evaluate_rows with both outputs given captures (it allocates nothing) and every replay gives the bits of the eager call."""
    from rl_on_manifold_amd import evaluate_rows
    case = eo.SHAPE_CASES[0][:4] + (200,)
    pol, x, action = _case('f32', case)[:3]
    sx, sa = x.clone(), action.clone()
    y, lp = torch.zeros_like(action), torch.zeros((x.shape[0],), device=DEV)
    evaluate_rows(pol, sx, sa, y=y, logp=lp)               # warm: the library is loaded
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        evaluate_rows(pol, sx, sa, y=y, logp=lp)
    for shift in (0.25, -0.5):
        sx.copy_(x + shift)
        sa.copy_(action - shift)
        y.zero_()
        lp.zero_()
        graph.replay()
        torch.cuda.synchronize()
        ey, elp = torch.empty_like(y), torch.empty_like(lp)
        evaluate_rows(pol, x + shift, action - shift, y=ey, logp=elp)
        assert torch.equal(y, ey) and torch.equal(lp, elp)
