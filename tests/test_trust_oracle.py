"""CPU-only checks of tests/trust_oracle.py, what the GPU tests of libatacom_trust.so are measured against: the Fisher-vector
product equals torch's float64 double backward through torch.distributions.kl_divergence on every case, it is symmetric and
positive semi-definite, torch's own FLOAT32 double backward stays inside the float32 bound on every element of every GPU case,
three deliberate mistakes fail the bound and the norm rule, the conjugate-gradient loop equals a dense solve, and the three
line-search cases have the margins they claim.  No library is called -- but the package is imported, because these are the
tests of rl_on_manifold_amd.trust."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_oracle as fo                                       # noqa: E402
import trust_oracle as to                                     # noqa: E402
from rl_on_manifold_amd import trust                          # noqa: E402,F401  (the module under test must exist)

_cases = {}


def _case(spec):
    if spec not in _cases:
        _cases[spec] = to.case(*spec)
    return _cases[spec]


def torch_fvp(c, dt, damping, v=None, exact_std=False):
    """MushroomRL's TRPO._fisher_vector_product_t on the case's rows: two torch.autograd.grad calls through
    kl_divergence(old, new).mean(), then + damping v.  The new distribution's scale is exp(log_std) with log_std = log(std);
    `exact_std` writes it std * exp(s) at s = 0 instead -- the same derivatives with respect to s as to log_std, and a scale
    that IS the case's std, where log and exp in float32 would evaluate another policy, a few units of roundoff away."""
    net = c['net']
    t = lambda a: None if a is None else torch.tensor(np.asarray(a, dtype=np.float64), dtype=dt)          # noqa: E731
    P = [t(net[k]).requires_grad_() for k in fo.NAMES]
    std = t(c['std'])
    if exact_std:
        ls = torch.zeros_like(std).requires_grad_()
        scale = lambda: std * ls.exp()                        # noqa: E731
    else:
        ls = std.log().requires_grad_()
        scale = lambda: ls.exp()                              # noqa: E731
    x, sh, sc = t(c['x']), t(net['obs_shift']), t(net['obs_scale'])
    xn = x if sh is None else (x - sh) * sc
    f = torch.relu if net['activation'] == 'relu' else torch.tanh
    mu = f(f(xn @ P[0].T + P[1]) @ P[2].T + P[3]) @ P[4].T + P[5]
    MVN = torch.distributions.MultivariateNormal
    kl = torch.distributions.kl_divergence(MVN(mu.detach(), scale_tril=torch.diag(scale().detach())),
                                           MVN(mu, scale_tril=torch.diag(scale()))).mean()
    params = P + [ls]
    flat = torch.cat([g.reshape(-1) for g in torch.autograd.grad(kl, params, create_graph=True)])
    v = t(c['v'] if v is None else v)
    hv = torch.autograd.grad((flat * v).sum(), params)
    return (torch.cat([h.reshape(-1) for h in hv]) + damping * v).numpy().astype(np.float64)


@pytest.mark.parametrize('spec', to.CASES, ids=str)
def test_the_oracle_is_torchs_float64_double_backward(spec):
    """Every element, the log-std block (2 v_ls) and the damping included, to 1e-12 of the element's scale."""
    c = _case(spec)
    w = c['want']
    assert w['kinks'] == 0
    n_out = spec[2]
    got = torch_fvp(c, torch.float64, to.DAMPING)
    assert got.shape == w['flat'].shape == (to.size(spec[1], n_out),)
    assert (np.abs(got - w['flat']) <= 1e-12 * w['scale'] + 1e-14).all()
    ls = c['v'][-n_out:].astype(np.float64)
    assert np.array_equal(w['flat'][-n_out:], 2.0 * ls + to.DAMPING * ls)
    plain = to.fvp(c['net'], c['std'], c['x'], c['v'], 0.0)['flat']
    assert np.allclose(w['flat'] - plain, to.DAMPING * c['v'].astype(np.float64), rtol=0, atol=1e-12 * np.abs(w['scale']).max())


@pytest.mark.parametrize('spec', to.CASES[::3], ids=str)
def test_the_product_is_symmetric_and_positive_semidefinite(spec):
    c = _case(spec)
    u, v = c['g'].astype(np.float64), c['v'].astype(np.float64)
    Fu, Fv = (to.fvp(c['net'], c['std'], c['x'], d, 0.0) for d in (u, v))
    tol = 1e-12 * (np.abs(u) @ Fv['scale'] + np.abs(v) @ Fu['scale']) + 1e-14
    assert abs(u @ Fv['flat'] - v @ Fu['flat']) <= tol
    assert v @ Fv['flat'] >= -tol and u @ Fu['flat'] >= -tol


@pytest.mark.parametrize('spec', to.CASES, ids=str)
def test_torchs_float32_double_backward_is_inside_the_float32_bound(spec):
    """The bound is checked against a reference, not against the device: torch's CPU evaluation of the same double backward in
    float32, every element of every case of tests/test_gpu_trust.py."""
    c = _case(spec)
    w = c['want']
    got = torch_fvp(c, torch.float32, to.DAMPING, exact_std=True)
    ratio = np.abs(got - w['flat']) / w['bound']
    print('%s: worst |error| / bound %.3g, ||error|| / ||ref|| %.3g' % (spec, ratio.max(), np.linalg.norm(got - w['flat']) / np.linalg.norm(w['flat'])))
    assert (w['bound'] > 0).all() and (ratio <= 1.0).all()
    assert np.linalg.norm(got - w['flat']) <= 1e-2 * np.linalg.norm(w['flat'])


@pytest.mark.parametrize('mistake', to.MISTAKES)
@pytest.mark.parametrize('spec', [to.CASES[3], to.CASES[5], to.CASES[-2]], ids=str)
def test_a_deliberate_mistake_fails_the_bound_and_the_norm_rule(spec, mistake):
    c = _case(spec)
    w = c['want']
    wrong = to.fvp(c['net'], c['std'], c['x'], c['v'], to.DAMPING, mistake=mistake)['flat']
    assert (np.abs(wrong - w['flat']) > w['bound']).any()
    assert np.linalg.norm(wrong - w['flat']) > 1e-2 * np.linalg.norm(w['flat'])


def test_cg_equals_a_dense_solve():
    """(4, 1): F assembled column by column from the oracle, (F + damping I) x = g solved densely; the loop, allowed P
    iterations, reaches it to 1e-8 ||x|| (it stops long before: F has rank <= 65 rows x 1 output + 1)."""
    spec = to.CASES[0]
    c = _case(spec)
    n = to.size(4, 1)
    F = np.empty((n, n))
    e = np.zeros(n)
    for i in range(n):
        e[i] = 1.0
        F[:, i] = to.fvp(c['net'], c['std'], c['x'], e, 0.0)['flat']
        e[i] = 0.0
    assert np.abs(F - F.T).max() <= 1e-12 * np.abs(F).max()
    g = c['g'].astype(np.float64)
    A = F + to.DAMPING * np.eye(n)
    dense = np.linalg.solve(A, g)
    x, r2, its, _ = to.cg(lambda p: A @ p, g, iters=n, tol=1e-30 * (g @ g))
    print('cg stopped after %d of %d iterations, residual^2 %.3g' % (its, n, r2))
    assert np.linalg.norm(x - dense) <= 1e-8 * np.linalg.norm(dense)
    # ten iterations, the reference's n_epochs_cg, are a partial solve: the loop's early stop is not what ends them
    assert to.cg(lambda p: A @ p, g, iters=10, tol=1e-10)[2] == 10


def test_the_cg_reference_of_the_gpu_tests():
    """The (18, 5) case of 200 rows: the residual falls over the first three iterations, so a tolerance between the second and
    the third stops the loop after exactly three; the allowances are finite and the float32 one is the larger."""
    c = _case(next(s for s in to.CASES if s[-1] == 200))
    ref = to.cg_reference(c)
    h = ref['hist']
    assert ref['n'] == 10 and h[2] < h[1] and h[2] < h[0]
    tol3 = float(np.sqrt(h[2] * min(h[0], h[1])))
    three = to.cg_reference(c, tol=tol3)
    assert three['n'] == 3 and not np.array_equal(three['x'], ref['x'])
    assert np.isfinite(ref['r']).all() and np.isfinite(ref['r32']) and ref['r32'] > ref['r'].max()
    print('r32 / ||x||inf: ten iterations %.3g, three %.3g' % (ref['r32'] / np.abs(ref['x']).max(), three['r32'] / np.abs(three['x']).max()))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('name', sorted(to.TRPO_CASES))
def test_the_line_search_cases_have_the_margins_they_claim(name, dtype):
    """(a) accepted at j = 0, (b) after 2 to 4 halvings, (c) nothing accepted in two tries -- and at every candidate tried both
    kl - 1.5 max_kl and the improvement are at least 100 x their float32 forward bounds away from 0, so that a float32 device
    takes the same branches."""
    c = to.trpo_case(name, dtype)
    w = c['want']
    for j, (dkl, e_kl, improve, e_imp) in enumerate(w['candidates']):
        print('%s j = %d: kl - 1.5 max_kl %+.4g (bound %.3g), improve %+.4g (bound %.3g)' % (name, j, dkl, e_kl, improve, e_imp))
        assert abs(dkl) >= 100.0 * e_kl and abs(improve) >= 100.0 * e_imp
    if name == 'a':
        assert w['accepted'] and w['halvings'] == 0
    elif name == 'b':
        assert w['accepted'] and 2 <= w['halvings'] <= 4
        assert any(dkl > 0 or imp < 0 for dkl, _, imp, _ in w['candidates'][:-1])
    else:
        assert not w['accepted'] and w['halvings'] == c['line_search'] == 2 and len(w['candidates']) == 2
        assert np.array_equal(w['theta'], w['theta_old'])
    assert abs(w['g'][-c['n_out']:] - to.trpo(dict(c), max_kl=c['max_kl'], ent_coeff=0.0, line_search=1)['g'][-c['n_out']:] - to.ENT_COEFF).max() < 1e-15
