"""GPU tests of libatacom_fit.so (rl_on_manifold_amd/fit.py): the gradients of the value loss and of PPO's clipped surrogate
against the float64 oracle of tests/fit_oracle.py, float32 inside its bound on EVERY element and float64 to 1e-12 of the
element's scale; row counts around the 16-row block and the 64-row tile, one and several tiles per wavefront; every
CH = ceil(n_in / 4) path that differs; gathering through idx; columns of padded full and compact records read in place with NaN
in the padding and poison around every output; repeated calls, other grids, reuse of the outputs, graph capture, and three Adam
steps through Gradients.to_module against torch's autograd.  Shapes are the smallest at which the kernels can go wrong."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_oracle as fo                                       # noqa: E402

DEV = 'cuda:0'
DT = {'f32': torch.float32, 'f64': torch.float64}
NP = {'f32': np.float32, 'f64': np.float64}
_cache = {}
_spec = {(c[1],) + tuple(c[2:]): c for c in fo.CASES}         # (head, n_in, n_out, activation, normalise, rows) -> its seed


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(dt, spec):
    """(policy on the device, the case's tensors on the device, the case with its oracle), made once per case and dtype."""
    key = (dt, spec)
    if key not in _cache:
        from rl_on_manifold_amd import MlpPolicy
        c = fo.case(*spec, dtype=NP[dt])
        net = c['net']
        pol = MlpPolicy(*(_t(net[k]) for k in fo.NAMES), std=_t(c['std']), obs_shift=_t(net['obs_shift']),
                        obs_scale=_t(net['obs_scale']), activation=net['activation'])
        _cache[key] = (pol, {k: _t(c[k]) for k in ('x', 'action', 'weight', 'logp_old')}, c)
    return _cache[key]


def _call(dt, spec, **kw):
    from rl_on_manifold_amd import fit
    pol, t, c = _case(dt, spec)
    if spec[1] == fo.VALUE:
        return fit.value_gradient(pol, t['x'], t['weight'], **kw)
    return fit.policy_gradient(pol, t['x'], t['action'], t['weight'], t['logp_old'], clip=c['clip'], **kw)


def _inside(dt, g, want, what):
    """float32: |error| <= the oracle's bound on every element; float64: <= 1e-12 scale + 1e-14.  The oracle's float32 bound is
    a worst case over three layers and is wide (torch's own float32 autograd uses a thousandth of it, tests/test_fit_oracle.py),
    so float32 is ALSO held to what separates rounding from a mistake of layout or sign: the latter moves the gradient by its
    own norm, the former by about 1e-6 of it (up to 1e-4 through rho at std = 1e-2); the relative error of the whole vector in
    the 2-norm stays below 1e-2.  -> the worst |error| / bound."""
    worst = 0.0
    for name, got, ref, e32, scale in (('grad', g.flat, want['flat'], want['bound'], want['scale']),
                                       ('stats', g.stats, want['stats'], want['stats_bound'], want['stats_scale'])):
        got = got.cpu().numpy().astype(np.float64)
        assert got.shape == ref.shape and np.isfinite(got).all(), (what, name)
        bound = e32 if dt == 'f32' else 1e-12 * scale + 1e-14
        err = np.abs(got - ref)
        live = bound > 0
        w = float((err[live] / bound[live]).max()) if live.any() else 0.0
        print('%s %s %s: worst |error| / bound %.4g, worst |error| %.3g' % (what, dt, name, w, err.max()))
        assert (err <= bound).all(), (what, dt, name, 'worst |error| / bound %.3g on %d of %d' % (w, int((err > bound).sum()), err.size))
        if name == 'grad':
            assert np.linalg.norm(got - ref) <= 1e-2 * np.linalg.norm(ref), (what, dt, np.linalg.norm(got - ref) / np.linalg.norm(ref))
        worst = max(worst, w)
    return worst


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('head', [fo.VALUE, fo.PPO_CLIP], ids=['value', 'ppo'])
@pytest.mark.parametrize('rows,n_blocks', fo.ROW_CASES)
def test_row_counts_and_grids(dt, head, rows, n_blocks):
    """1 .. 600 rows: a lone row, a part-filled 16-block, a tail wave, 200 rows walked by one and by two workgroups, and 600 by
    one, whose float32 wavefronts walk two and three tiles.  A repeated call gives the same bits; another grid agrees inside the
    bound (both do, with the oracle)."""
    spec = _spec[(head,) + fo.ROW_SHAPE[head] + (rows,)]
    g = _call(dt, spec, n_blocks=n_blocks)
    _inside(dt, g, _case(dt, spec)[2]['want'], (spec, n_blocks))
    again = _call(dt, spec, n_blocks=n_blocks)
    assert torch.equal(again.flat, g.flat) and torch.equal(again.stats, g.stats)
    if n_blocks:
        _inside(dt, _call(dt, spec, n_blocks=0), _case(dt, spec)[2]['want'], (spec, 0))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('spec', [c for c in fo.CASES if c[0] < 300], ids=str)
def test_network_shapes(dt, spec):
    """n_in 4 .. 32 (CH = 1, widths that are no multiple of 4, the maximum, one and two input tiles of dW1), n_out 1 .. 8, both
    activations, with and without the observation normalisation, 65 rows; the value head at (4, 1) and (25, 1)."""
    g = _call(dt, spec)
    _inside(dt, g, _case(dt, spec)[2]['want'], spec)
    assert (g.log_std is None) == (spec[1] == fo.VALUE)
    assert g.W1.shape == (64, spec[2]) and g.W3.shape == (spec[3], 64) and g.W1.data_ptr() == g.flat.data_ptr()


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('head', [fo.VALUE, fo.PPO_CLIP], ids=['value', 'ppo'])
def test_idx_gathers_in_the_row_loads(dt, head):
    """70 of 200 rows, shuffled, with repeats: the oracle on the gathered rows, and inside the bound the call on gathered
    contiguous copies; idx = arange gives the bits of idx = None."""
    from rl_on_manifold_amd import fit
    spec = _spec[(head,) + fo.ROW_SHAPE[head] + (200,)]
    pol, t, c = _case(dt, spec)
    rng = np.random.default_rng(5)
    pick = rng.permutation(200)[:64]
    pick = np.concatenate([pick, pick[:6]])[rng.permutation(70)].astype(np.int64)
    want = fo.oracle(c, head, pick)
    assert want['kinks'] == 0
    idx = _t(pick)
    g = _call(dt, spec, idx=idx)
    _inside(dt, g, want, (spec, 'idx'))
    copies = {k: (None if v is None else v[idx].contiguous()) for k, v in t.items()}
    if head == fo.VALUE:
        h = fit.value_gradient(pol, copies['x'], copies['weight'])
    else:
        h = fit.policy_gradient(pol, copies['x'], copies['action'], copies['weight'], copies['logp_old'], clip=c['clip'])
    _inside(dt, h, want, (spec, 'gathered copies'))
    fit.check_idx(idx, 200)
    with pytest.raises(ValueError, match='row numbers'):
        fit.check_idx(idx + 150, 200)
    every = _call(dt, spec, idx=torch.arange(200, device=DEV))
    plain = _call(dt, spec)
    assert torch.equal(every.flat, plain.flat) and torch.equal(every.stats, plain.stats)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('compact', [False, True], ids=['full', 'compact'])
def test_columns_of_padded_records_are_read_in_place_and_nothing_else_is_written(dt, compact):
    """obs and action as columns of [T = 3, batch_stride = 8 > B = 5, F] records whose padding rows, other columns and (compact)
    tail row hold NaN; gradients, statistics and workspace inside poisoned buffers: the bits of the contiguous call, and not a
    byte outside the outputs and the declared workspace changes."""
    from rl_on_manifold_amd import MlpPolicy, fit
    from rl_on_manifold_amd.rollout import CompactRecordLayout, RecordLayout
    T, B, stride, n_in, n_out = 3, 5, 8, 18, 5
    lay = CompactRecordLayout([B], n_in, n_out, T) if compact else RecordLayout([B], n_in, n_out)
    width = lay.Fc if compact else lay.F
    poison = 12345.0
    for head, spec in ((fo.PPO_CLIP, (401, fo.PPO_CLIP, n_in, n_out, 'relu', False, T * B)), (fo.VALUE, (402, fo.VALUE, n_in, 1, 'tanh', True, T * B))):
        pol, t, c = _case(dt, spec)
        ref = _call(dt, spec)
        _inside(dt, ref, c['want'], spec)
        rec = torch.full((T + compact, stride, width), float('nan'), dtype=DT[dt], device=DEV)
        rec[:T, :B, lay.fields['obs']] = t['x'].view(T, B, n_in)
        if head == fo.PPO_CLIP:
            rec[:T, :B, lay.fields['action']] = t['action'].view(T, B, n_out)
        view = rec[:, :B]
        out = _call(dt, spec)                                            # a Gradients whose buffers are moved into poison
        n, need = out.flat.numel(), out.workspace.numel()
        big = torch.full((n + 64,), poison, dtype=DT[dt], device=DEV)
        sbuf = torch.full((4 + 16,), poison, dtype=DT[dt], device=DEV)
        wbuf = torch.full((need + 512,), 0x5a, dtype=torch.uint8, device=DEV)
        out.flat, out.stats, out.workspace = big[32:32 + n], sbuf[8:12], wbuf[256:256 + need]
        w2 = t['weight'].view(T, B)
        if head == fo.VALUE:
            got = fit.value_gradient_from_records(lay, view, w2, pol, out=out)
        else:
            got = fit.policy_gradient_from_records(lay, view, w2, t['logp_old'].view(T, B), pol, clip=c['clip'], out=out)
        assert got is out and torch.equal(out.flat, ref.flat) and torch.equal(out.stats, ref.stats)
        assert bool((big[:32] == poison).all()) and bool((big[32 + n:] == poison).all())
        assert bool((sbuf[:8] == poison).all()) and bool((sbuf[12:] == poison).all())
        assert bool((wbuf[:256] == 0x5a).all()) and bool((wbuf[256 + need:] == 0x5a).all())
        assert bool(torch.isnan(rec[:, B:]).all()) and (not compact or bool(torch.isnan(rec[T]).all()))      # inputs are inputs
        assert torch.equal(rec[:T, :B, lay.fields['obs']].reshape(T * B, n_in), t['x'])
        # idx numbers the flat [T * B] rows of the view
        idx = torch.tensor([14, 0, 7, 7, 3], device=DEV)
        if head == fo.VALUE:
            a, b = fit.value_gradient_from_records(lay, view, w2, pol, idx=idx), fit.value_gradient(pol, t['x'], t['weight'], idx=idx)
        else:
            a = fit.policy_gradient_from_records(lay, view, w2, t['logp_old'].view(T, B), pol, clip=c['clip'], idx=idx)
            b = fit.policy_gradient(pol, t['x'], t['action'], t['weight'], t['logp_old'], clip=c['clip'], idx=idx)
        assert torch.equal(a.flat, b.flat) and torch.equal(a.stats, b.stats)
    # leading dimensions that do not collapse to one (outer, inner) pair are refused: a gradient cannot be split over launches
    two = torch.zeros((2, T + 1, stride, lay.F if not compact else lay.Fc), dtype=DT[dt], device=DEV)
    crit = _case(dt, (402, fo.VALUE, n_in, 1, 'tanh', True, T * B))[0]
    with pytest.raises(ValueError, match='do not collapse'):
        fit.value_gradient(crit, two[:, :T, :B, :n_in], torch.zeros((2, T, B), dtype=DT[dt], device=DEV))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('head', [fo.VALUE, fo.PPO_CLIP], ids=['value', 'ppo'])
def test_out_is_reused_without_allocation_and_a_graph_sees_new_weights(dt, head):
    """out=: the second call allocates nothing; a captured graph replayed after an in-place change of the weights gives the bits
    of a fresh call."""
    spec = _spec[(head,) + fo.ROW_SHAPE[head] + (65,)]
    pol = _case(dt, spec)[0]
    out = _call(dt, spec)
    first = out.flat.clone()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    assert _call(dt, spec, out=out) is out
    assert torch.cuda.memory_allocated() == before
    assert torch.equal(out.flat, first)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _call(dt, spec, out=out)                                         # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _call(dt, spec, out=out)
    keep = {k: pol.tensors[k].clone() for k in ('W2', 'b3')}
    try:
        pol.tensors['W2'].mul_(0.5)
        pol.tensors['b3'].add_(0.25)
        out.flat.zero_()
        graph.replay()
        torch.cuda.synchronize()
        fresh = _call(dt, spec)
        assert torch.equal(out.flat, fresh.flat) and torch.equal(out.stats, fresh.stats)
        assert not torch.equal(out.flat, first)
    finally:
        for k, v in keep.items():
            pol.tensors[k].copy_(v)


def test_three_adam_steps_through_to_module_are_those_of_autograd():
    """A toy problem in float64: an actor 6 -> 2 with log std and a critic 6 -> 1, 130 rows in minibatches of 64 with a tail of
    2, three Adam steps.  The library's gradients, handed over by Gradients.to_module, against torch's autograd of the
    example's expressions: the parameters stay equal to 1e-10."""
    import math
    import torch.nn as nn
    from rl_on_manifold_amd import MlpPolicy, fit

    class Net(nn.Module):
        def __init__(self, n_in, n_out):
            super().__init__()
            self._h1, self._h2, self._h3 = nn.Linear(n_in, 64), nn.Linear(64, 64), nn.Linear(64, n_out)

        def forward(self, x):
            return self._h3(torch.tanh(self._h2(torch.tanh(self._h1(x)))))

    torch.manual_seed(3)
    R, n_in, k, clip, dt = 130, 6, 2, 0.2, torch.float64
    obs, act = torch.randn(R, n_in, dtype=dt, device=DEV), torch.randn(R, k, dtype=dt, device=DEV) * 0.3
    adv, ret = torch.randn(R, dtype=dt, device=DEV), torch.randn(R, dtype=dt, device=DEV)
    worlds = []
    for _ in range(2):
        torch.manual_seed(11)
        actor, critic = Net(n_in, k).to(DEV, dt), Net(n_in, 1).to(DEV, dt)
        log_std = torch.full((k,), -0.7, dtype=dt, device=DEV, requires_grad=True)
        worlds.append((actor, critic, log_std, torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()) + [log_std], lr=1e-2)))
    (a0, c0, ls0, opt0), (a1, c1, ls1, opt1) = worlds
    with torch.no_grad():
        mu = a0(obs)
        logp_old = (-0.5 * ((act - mu) / ls0.exp()) ** 2 - ls0).sum(-1) - 0.5 * k * math.log(2 * math.pi) + 0.3 * torch.randn(R, dtype=dt, device=DEV)
    std = ls1.detach().exp()
    pol, cri = MlpPolicy.from_module(a1, std=std, activation='tanh'), MlpPolicy.from_module(c1, activation='tanh')
    gp = gc = None
    perm = torch.randperm(R, device=DEV)
    for i in range(0, R, 64):
        idx = perm[i:i + 64]
        mu = a0(obs[idx])
        logp = (-0.5 * ((act[idx] - mu) / ls0.exp()) ** 2 - ls0).sum(-1) - 0.5 * k * math.log(2 * math.pi)
        ratio = (logp - logp_old[idx]).exp()
        pl = -torch.min(ratio * adv[idx], ratio.clamp(1 - clip, 1 + clip) * adv[idx]).mean()
        vl = (c0(obs[idx]).squeeze(-1) - ret[idx]).pow(2).mean()
        opt0.zero_grad()
        (pl + vl).backward()
        opt0.step()
        gp = fit.policy_gradient(pol, obs, act, adv, logp_old, clip=clip, idx=idx, out=gp).to_module(a1, ls1)
        gc = fit.value_gradient(cri, obs, ret, idx=idx, out=gc).to_module(c1)
        assert abs(gp.stats[0].item() - pl.item()) < 1e-10 and abs(gc.loss.item() - vl.item()) < 1e-10
        opt1.step()
        std.copy_(ls1.detach().exp())                 # the policy's std follows log_std, in place
    for p0, p1 in zip(list(a0.parameters()) + list(c0.parameters()) + [ls0], list(a1.parameters()) + list(c1.parameters()) + [ls1]):
        assert float((p0 - p1).detach().abs().max()) <= 1e-10
