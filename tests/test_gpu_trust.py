"""GPU tests of libatacom_trust.so and rl_on_manifold_amd/trust.py: the Fisher-vector product against the float64 oracle of
tests/trust_oracle.py, float32 inside its bound on EVERY element and to 1e-2 of the vector's norm, float64 to 1e-12 of the
element's scale; row counts around the 16-row block and the 64-row tile, one and several tiles per wavefront; every
CH = ceil(n_in / 4) path that differs; gathering through idx; the obs column of padded full and compact records read in place
with NaN in the padding and poison around the outputs; the damping and the log-std block exactly as the header orders them;
the conjugate-gradient solve against the oracle's with conditioning-aware allowances, its device-side stop and its graph; the
TRPO step's line search on three cases built on the CPU; and three iterations of the example's loop.  Shapes are the smallest
at which the kernels can go wrong."""
import os
import sys

import numpy as np
import pytest
import torch

from rl_on_manifold_amd import MlpPolicy, trust

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_oracle as fo                                       # noqa: E402
import trust_oracle as to                                     # noqa: E402

DEV = 'cuda:0'
DT = {'f32': torch.float32, 'f64': torch.float64}
NP = {'f32': np.float32, 'f64': np.float64}
_cache = {}
_spec = {tuple(c[1:]): c for c in to.CASES}                   # (n_in, n_out, activation, normalise, rows) -> its case
ROWS200 = _spec[to.ROW_SHAPE + (200,)]


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _policy(net, std):
    return MlpPolicy(*(_t(net[k]) for k in fo.NAMES), std=_t(std), obs_shift=_t(net['obs_shift']), obs_scale=_t(net['obs_scale']),
                     activation=net['activation'])


def _case(dt, spec):
    """(policy on the device, the case's tensors on the device, the case with its oracle), made once per case and dtype."""
    key = (dt, spec)
    if key not in _cache:
        c = to.case(*spec, dtype=NP[dt])
        _cache[key] = (_policy(c['net'], c['std']), {k: _t(c[k]) for k in ('x', 'v', 'g', 'rhs')}, c)
    return _cache[key]


def _call(dt, spec, **kw):
    pol, t, c = _case(dt, spec)
    kw.setdefault('damping', c['damping'])
    return trust.fisher_vector_product(pol, t['x'], t['v'], **kw)


def _inside(dt, got, want, what):
    """float32: |error| <= the oracle's bound on every element AND ||error|| <= 1e-2 ||ref|| (the rule of tests/test_gpu_fit.py:
    rounding moves the vector by about 1e-6 of its norm, a mistake of layout or sign by its own norm); float64: <= 1e-12 scale
    + 1e-14.  -> the worst |error| / bound."""
    ref = want['flat']
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    bound = want['bound'] if dt == 'f32' else 1e-12 * want['scale'] + 1e-14
    err = np.abs(got - ref)
    w = float((err / bound).max())
    print('%s %s: worst |error| / bound %.4g, ||error|| / ||ref|| %.3g' % (what, dt, w, np.linalg.norm(got - ref) / np.linalg.norm(ref)))
    assert (err <= bound).all(), (what, dt, 'worst |error| / bound %.3g on %d of %d' % (w, int((err > bound).sum()), err.size))
    if dt == 'f32':
        assert np.linalg.norm(got - ref) <= 1e-2 * np.linalg.norm(ref), (what, np.linalg.norm(got - ref) / np.linalg.norm(ref))
    return w


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('rows,n_blocks', to.ROW_CASES)
def test_row_counts_and_grids(dt, rows, n_blocks):
    """1 .. 600 rows: a lone row, a part-filled 16-block, a tail wave, 200 rows walked by one and by two workgroups, and 600 by
    one, whose float32 wavefronts walk two and three tiles.  A repeated call gives the same bits; another grid agrees inside the
    bound (both do, with the oracle)."""
    spec = _spec[to.ROW_SHAPE + (rows,)]
    want = _case(dt, spec)[2]['want']
    got = _call(dt, spec, n_blocks=n_blocks)
    _inside(dt, got, want, (spec, n_blocks))
    assert torch.equal(_call(dt, spec, n_blocks=n_blocks), got)
    if n_blocks:
        _inside(dt, _call(dt, spec, n_blocks=0), want, (spec, 0))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('spec', [c for c in to.CASES if c[0] < 600], ids=str)
def test_network_shapes(dt, spec):
    """n_in 4 .. 32 (CH = 1, widths that are no multiple of 4, the maximum, one and two input tiles of dW1), n_out 1 .. 8, both
    activations, with and without the observation normalisation, 65 rows."""
    got = _call(dt, spec)
    _inside(dt, got, _case(dt, spec)[2]['want'], spec)
    assert got.shape == (to.size(spec[1], spec[2]),)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_idx_gathers_in_the_row_loads(dt):
    """70 of 200 rows, shuffled, with repeats: the oracle on the gathered rows, and inside the bound the call on gathered
    contiguous copies; idx = arange gives the bits of idx = None."""
    pol, t, c = _case(dt, ROWS200)
    rng = np.random.default_rng(5)
    pick = rng.permutation(200)[:64]
    pick = np.concatenate([pick, pick[:6]])[rng.permutation(70)].astype(np.int64)
    want = to.fvp(c['net'], c['std'], c['x'], c['v'], c['damping'], idx=pick)
    assert want['kinks'] == 0
    idx = _t(pick)
    _inside(dt, _call(dt, ROWS200, idx=idx), want, 'idx')
    _inside(dt, trust.fisher_vector_product(pol, t['x'][idx].contiguous(), t['v'], damping=c['damping']), want, 'gathered copies')
    assert torch.equal(_call(dt, ROWS200, idx=torch.arange(200, device=DEV)), _call(dt, ROWS200))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('compact', [False, True], ids=['full', 'compact'])
def test_the_obs_column_of_padded_records_is_read_in_place_and_nothing_else_is_written(dt, compact):
    """obs as a column of [T = 3, batch_stride = 8 > B = 5, F] records whose padding rows, other columns and (compact) tail row
    hold NaN; the product and the workspace inside poisoned buffers: the bits of the contiguous call, and not a byte outside the
    output and the declared workspace changes."""
    from rl_on_manifold_amd.rollout import CompactRecordLayout, RecordLayout
    T, B, stride, n_in, n_out = 3, 5, 8, 18, 5
    lay = CompactRecordLayout([B], n_in, n_out, T) if compact else RecordLayout([B], n_in, n_out)
    width = lay.Fc if compact else lay.F
    spec = (690, n_in, n_out, 'relu', False, T * B)
    pol, t, c = _case(dt, spec)
    ref = _call(dt, spec)
    _inside(dt, ref, c['want'], spec)
    rec = torch.full((T + compact, stride, width), float('nan'), dtype=DT[dt], device=DEV)
    rec[:T, :B, lay.fields['obs']] = t['x'].view(T, B, n_in)
    view = rec[:, :B]
    out = trust.FisherProduct.like(pol, t['x'])
    n, need = out.flat.numel(), out.workspace.numel()
    poison = 12345.0
    big = torch.full((n + 64,), poison, dtype=DT[dt], device=DEV)
    wbuf = torch.full((need + 512,), 0x5a, dtype=torch.uint8, device=DEV)
    out.flat, out.workspace = big[32:32 + n], wbuf[256:256 + need]
    got = trust.fisher_vector_product_from_records(lay, view, t['v'], pol, damping=c['damping'], out=out)
    assert got.data_ptr() == out.flat.data_ptr() and torch.equal(got, ref)
    assert bool((big[:32] == poison).all()) and bool((big[32 + n:] == poison).all())
    assert bool((wbuf[:256] == 0x5a).all()) and bool((wbuf[256 + need:] == 0x5a).all())
    assert bool(torch.isnan(rec[:, B:]).all()) and (not compact or bool(torch.isnan(rec[T]).all()))      # inputs are inputs
    assert torch.equal(rec[:T, :B, lay.fields['obs']].reshape(T * B, n_in), t['x'])
    # idx numbers the flat [T * B] rows of the view
    idx = torch.tensor([14, 0, 7, 7, 3], device=DEV)
    a = trust.fisher_vector_product_from_records(lay, view, t['v'], pol, damping=c['damping'], idx=idx)
    assert torch.equal(a, trust.fisher_vector_product(pol, t['x'], t['v'], damping=c['damping'], idx=idx))
    # with out= the call allocates nothing
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    trust.fisher_vector_product_from_records(lay, view, t['v'], pol, damping=c['damping'], out=out)
    assert torch.cuda.memory_allocated() == before


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_the_damping_and_the_log_std_block_enter_exactly(dt):
    """out = (F v) + (d v) with d rounded once to the dtype and every operation rounded on its own: from the call without
    damping, numpy in the dtype reproduces the call with damping bit for bit, so fvp(d) - fvp(0) is d v to the one rounding of
    the sum; the log-std block is (2 v) + (d v)."""
    pol, t, c = _case(dt, ROWS200)
    n_out, T = c['n_out'], NP[dt]
    v = c['v']
    plain = _call(dt, ROWS200, damping=0.0).cpu().numpy()
    assert plain.dtype == T and np.array_equal(plain[-n_out:], T(2) * v[-n_out:])
    for d in (1e-2, 0.37):
        got = _call(dt, ROWS200, damping=d).cpu().numpy()
        dv = T(d) * v
        assert dv.dtype == T and np.array_equal(got, plain + dv)
        assert np.array_equal(got[-n_out:], T(2) * v[-n_out:] + dv[-n_out:])


def _cg_ref(dt):
    """The oracle's solve of the (18, 5) case of 200 rows in `dt`, its allowances, and the tolerance that stops it after three
    iterations; computed once, on the CPU, from the reference alone."""
    if ('cg', dt) not in _cache:
        c = _case(dt, ROWS200)[2]
        ref = to.cg_reference(c)
        tol3 = float(np.sqrt(ref['hist'][2] * min(ref['hist'][:2])))
        three = to.cg_reference(c, tol=tol3)
        assert ref['n'] == 10 and three['n'] == 3
        _cache[('cg', dt)] = (ref, three, tol3)
    return _cache[('cg', dt)]


def _cg_inside(dt, x, ref, what):
    """|x - x_oracle| <= 1e-8 ||x||inf + 4 r on every element: r the oracle loop's own response to perturbations of its products
    of 1e-12, elementwise (float64), or r32, the size of the deviation of a numpy float32 run of the loop on the float32-rounded
    oracle product (float32; trust_oracle.cg_reference says why it is one number)."""
    r = ref['r'] if dt == 'f64' else np.full_like(ref['x'], ref['r32'])
    got = x.cpu().numpy().astype(np.float64)
    err, allow = np.abs(got - ref['x']), 1e-8 * np.abs(ref['x']).max() + 4.0 * r
    print('%s %s: worst |error| / allowance %.4g, ||error||inf / ||x||inf %.3g, allowance / ||x||inf max %.3g median %.3g' % (
        what, dt, (err / allow).max(), err.max() / np.abs(ref['x']).max(), allow.max() / np.abs(ref['x']).max(),
        np.median(allow) / np.abs(ref['x']).max()))
    assert np.isfinite(got).all() and (err <= allow).all(), (what, dt, int((err > allow).sum()), err.size)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_natural_gradient_is_the_oracles_and_its_stop_freezes_the_state(dt):
    """Ten iterations against the oracle's ten; with the tolerance at which the oracle stops after three, the device's ten
    iterations give the three-iteration x: the flag freezes x, r and p."""
    ref, three, tol3 = _cg_ref(dt)
    pol, t, c = _case(dt, ROWS200)
    work = trust.CgWork.like(pol, t['x'])
    x = trust.natural_gradient(pol, t['x'], t['rhs'], iters=10, damping=c['damping'], residual_tol=1e-10, work=work)
    assert x.data_ptr() == work.x.data_ptr()
    _cg_inside(dt, x, ref, 'ten iterations')
    assert not bool(work.done)
    x3 = trust.natural_gradient(pol, t['x'], t['rhs'], iters=10, damping=c['damping'], residual_tol=tol3, work=work).clone()
    _cg_inside(dt, x3, three, 'stopped after three')
    assert bool(work.done)
    only3 = trust.natural_gradient(pol, t['x'], t['rhs'], iters=3, damping=c['damping'], residual_tol=tol3, work=work)
    assert torch.equal(only3, x3)                            # seven frozen iterations changed no bit


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_natural_gradient_is_captured_and_replayed_with_a_changed_g(dt):
    """With work= the solve allocates nothing and is one linear chain: captured once, replayed twice with g changed in place,
    each replay has the bits of the eager call."""
    pol, t, c = _case(dt, ROWS200)
    work = trust.CgWork.like(pol, t['x'])
    g = t['rhs'].clone()
    kw = dict(iters=10, damping=c['damping'], residual_tol=1e-10, work=work)
    trust.natural_gradient(pol, t['x'], g, **kw)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    eager = trust.natural_gradient(pol, t['x'], g, **kw)
    assert torch.cuda.memory_allocated() == before
    eager = eager.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        trust.natural_gradient(pol, t['x'], g, **kw)         # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        trust.natural_gradient(pol, t['x'], g, **kw)
    work.x.zero_()
    graph.replay()
    assert torch.equal(work.x, eager)
    for other in (t['g'], 0.5 * t['rhs'] + t['v']):
        g.copy_(other)
        graph.replay()
        replayed = work.x.clone()
        assert torch.equal(replayed, trust.natural_gradient(pol, t['x'], other.clone(), **kw)) and not torch.equal(replayed, eager)


def _trpo_setup(dt, name):
    from rl_on_manifold_amd.rollout import RecordLayout
    c = to.trpo_case(name, dtype=NP[dt])
    n_in, n_out, rows = c['n_in'], c['n_out'], c['x'].shape[0]
    log_std = _t(c['log_std'])
    pol = _policy(c['net'], np.exp(c['log_std'].astype(np.float64)).astype(NP[dt]))
    lay = RecordLayout([rows], n_in, n_out)
    rec = torch.zeros((1, rows, lay.F), dtype=DT[dt], device=DEV)
    rec[0, :, lay.fields['obs']] = _t(c['x'])
    rec[0, :, lay.fields['action']] = _t(c['action'])
    return c, pol, log_std, lay, rec, _t(c['adv']).view(1, rows), _t(c['logp_old']).view(1, rows)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('name', sorted(to.TRPO_CASES))
def test_trpo_step_takes_the_oracles_branches(dt, name):
    """(a) accepted at once, (b) after 2 to 4 halvings, (c) nothing accepted: the same `halvings` and `accepted` as the oracle;
    the final parameters within the natural-gradient rule scaled by 2^-j / sqrt(shs / max_kl); in (c) every parameter tensor and
    std bit-equal to before."""
    c, pol, log_std, lay, rec, adv, lpo = _trpo_setup(dt, name)
    w = c['want']
    names = fo.NAMES + ('std',)
    before = {k: pol.tensors[k].clone() for k in names}
    ls_before = log_std.clone()
    res = trust.trpo_step(lay, rec, adv, lpo, pol, log_std, max_kl=c['max_kl'], ent_coeff=c['ent_coeff'], line_search=c['line_search'])
    print(name, dt, res, 'oracle', {k: w[k] for k in ('loss_old', 'loss_new', 'kl', 'halvings', 'accepted', 'cg_residual')})
    assert res['accepted'] == w['accepted'] and res['halvings'] == w['halvings']
    assert set(res) == {'loss_old', 'loss_new', 'kl', 'halvings', 'accepted', 'cg_residual'}
    if not w['accepted']:
        assert name == 'c'
        for k in names:
            assert torch.equal(pol.tensors[k], before[k]), k
        assert torch.equal(log_std, ls_before)
        assert res['loss_new'] == res['loss_old'] and res['kl'] == 0.0
        return
    assert np.isfinite(res['kl']) and res['kl'] <= 1.5 * c['max_kl'] and res['loss_new'] >= res['loss_old']
    # theta = theta_old + full 2^-j, full = x / sqrt(shs / max_kl): the natural-gradient rule carried to the full step
    # (trust_oracle.step_allowance, from the reference alone), scaled by 2^-j, plus the rounding of the sum
    got = np.concatenate([pol.tensors[n].cpu().numpy().reshape(-1) for n in fo.NAMES] + [log_std.cpu().numpy()]).astype(np.float64)
    u = 2.0 ** -24 if dt == 'f32' else 2.0 ** -53
    allow = 0.5 ** w['halvings'] * to.step_allowance(c, w, dt == 'f32') + 2.0 * u * np.abs(w['theta'])
    err = np.abs(got - w['theta'])
    print('%s %s: worst |theta error| / allowance %.4g, worst |theta error| %.3g, ||step||inf %.3g' % (
        name, dt, (err / allow).max(), err.max(), np.abs(w['theta'] - w['theta_old']).max()))
    assert (err <= allow).all(), (name, dt, int((err > allow).sum()), err.size)
    assert torch.equal(pol.tensors['std'], log_std.exp())


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_ent_coeff_shifts_the_log_std_part_of_g_by_exactly_that(dt, monkeypatch):
    """The reference's ent_coeff = 5e-5: the g that trpo_step hands to natural_gradient differs between ent_coeff = 0 and 5e-5
    by exactly one addition of 5e-5 to each log-std entry, and in nothing else."""
    seen = []
    real = trust.natural_gradient

    def spy(policy, obs, g, **kw):
        seen.append(g.clone())
        return real(policy, obs, g, **kw)
    monkeypatch.setattr(trust, 'natural_gradient', spy)
    for ent in (0.0, to.ENT_COEFF):
        c, pol, log_std, lay, rec, adv, lpo = _trpo_setup(dt, 'a')
        trust.trpo_step(lay, rec, adv, lpo, pol, log_std, max_kl=c['max_kl'], ent_coeff=ent, line_search=1)
    n_out = c['n_out']
    g0, g1 = seen
    assert torch.equal(g0[:-n_out], g1[:-n_out])
    assert torch.equal(g1[-n_out:], g0[-n_out:] + to.ENT_COEFF) and not torch.equal(g1[-n_out:], g0[-n_out:])
    want = c['want']['g']
    scale = np.abs(want).max()
    assert np.abs(g1.cpu().numpy().astype(np.float64) - want).max() <= (1e-3 if dt == 'f32' else 1e-10) * scale


def test_three_iterations_of_the_example():
    """examples/trpo_air_hockey.py on `planar`, B = 256, T = 16, three iterations: every printed kl is finite and, whenever the
    step was accepted, at most 1.5 max_kl."""
    import importlib.util
    import io
    import re
    from contextlib import redirect_stdout
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'trpo_air_hockey.py')
    spec = importlib.util.spec_from_file_location('trpo_air_hockey', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    buf = io.StringIO()
    with redirect_stdout(buf):
        mod.main(['--env', 'planar', '--batch', '256', '--horizon', '16', '--iters', '3'])
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith('iter')]
    print(buf.getvalue())
    assert len(lines) == 3
    for ln in lines:
        m = re.search(r'kl (\S+)\s+halvings (\d+)\s+accepted (\d)', ln)
        assert m, ln
        kl = float(m.group(1))
        assert np.isfinite(kl) and (m.group(3) == '0' or kl <= 1.5 * mod.MAX_KL)
