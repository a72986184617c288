"""CPU-only checks of tests/fit_oracle.py, the float64 restatement libatacom_fit.so is held to: it equals torch's float64
autograd of the two expressions of examples/ppo_air_hockey.py, torch's own FLOAT32 autograd lies inside its float32 bound on
every element of every case of the GPU suite -- the bound is validated against the reference implementation before a GPU sees
it -- and no row of any case sits at a kink."""
import math

import numpy as np
import pytest

import fit_oracle as fo

torch = pytest.importorskip('torch')


def torch_gradient(c, head, dtype, idx=None):
    """autograd of the example's expression -> (flat gradient in the library's order, stats[:3]) as float64 numpy.  d / d log std
    is taken at std_eff = std * exp(eta), eta = 0: exp(0) = 1 and std * 1 are exact, so float32 sees the case's own std."""
    net = c['net']
    t = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)     # noqa: E731
    P = {k: t(net[k]).requires_grad_() for k in fo.NAMES}
    x = t(c['x'])
    if net['obs_shift'] is not None:
        x = (x - t(net['obs_shift'])) * t(net['obs_scale'])
    act = torch.relu if net['activation'] == 'relu' else torch.tanh
    sel = (lambda a: a) if idx is None else (lambda a: a[torch.as_tensor(idx)])
    h = act(act(sel(x) @ P['W1'].T + P['b1']) @ P['W2'].T + P['b2']) @ P['W3'].T + P['b3']
    leaves = [P[k] for k in fo.NAMES]
    if head == fo.VALUE:
        loss = (h.squeeze(-1) - sel(t(c['weight']))).pow(2).mean()
        stats = [loss.item(), 0.0, 0.0]
    else:
        eta = torch.zeros(len(c['std']), dtype=dtype, requires_grad=True)
        std = t(c['std']) * eta.exp()
        k = len(c['std'])
        logp = (-0.5 * ((sel(t(c['action'])) - h) / std) ** 2 - std.log()).sum(-1) - 0.5 * k * math.log(2.0 * math.pi)
        ratio = (logp - sel(t(c['logp_old']))).exp()
        adv, clip = sel(t(c['weight'])), c['clip']
        loss = -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean()
        inactive = ((adv > 0) & (ratio > 1 + clip)) | ((adv < 0) & (ratio < 1 - clip))
        stats = [loss.item(), inactive.double().mean().item(), (sel(t(c['logp_old'])) - logp).mean().item()]
        leaves.append(eta)
    grads = torch.autograd.grad(loss, leaves)
    return np.concatenate([g.double().numpy().reshape(-1) for g in grads]), np.array(stats)


CASES = fo.CASES
_ids = ['%s-%d-%d-%s-%s-%d' % ('value' if c[1] == fo.VALUE else 'ppo', c[2], c[3], c[4], 'norm' if c[5] else 'raw', c[6]) for c in CASES]


@pytest.mark.parametrize('spec', CASES, ids=_ids)
def test_the_oracle_is_torch_float64_autograd(spec):
    seed, head = spec[:2]
    c = fo.case(*spec, dtype=np.float64)
    rows = spec[-1]
    rng = np.random.default_rng(seed)
    for idx in (None, rng.integers(0, rows, max(1, rows + 5))):                         # more picks than rows: repeats
        want = fo.oracle(c, head, idx)
        got, stats = torch_gradient(c, head, torch.float64, idx)
        assert got.shape == want['flat'].shape
        err = np.abs(got - want['flat'])
        assert (err <= 1e-12 * want['scale'] + 1e-14).all(), (err / (want['scale'] + 1e-300)).max()
        assert (np.abs(stats - want['stats'][:3]) <= 1e-12 * want['stats_scale'][:3] + 1e-14).all()


@pytest.mark.parametrize('spec', CASES, ids=_ids)
def test_torch_float32_autograd_lies_inside_the_float32_bound(spec):
    head = spec[1]
    c = fo.case(*spec)
    want = c['want']
    got, stats = torch_gradient(c, head, torch.float32)
    live = want['bound'] > 0                                  # a unit that no row activates has gradient 0 and bound 0
    worst = (np.abs(got - want['flat'])[live] / want['bound'][live]).max() if live.any() else 0.0
    print('worst |error| / bound %.3f' % worst)
    assert (np.abs(got - want['flat']) <= want['bound']).all(), worst
    assert (np.abs(stats - want['stats'][:3]) <= want['stats_bound'][:3] + 1e-300).all()


@pytest.mark.parametrize('spec', CASES, ids=_ids)
def test_no_row_of_any_case_sits_at_a_kink(spec):
    """Zero exclusions: relu pre-activations clear of 0 and ratios clear of 1 +- clip by more than their forward bounds; a PPO
    batch of 64 rows or more holds inactive rows on each side and active rows of both signs (fit_oracle.case asserts it)."""
    c = fo.case(*spec)
    assert c['want']['kinks'] == 0
    assert np.isfinite(c['want']['bound']).all() and np.isfinite(c['want']['flat']).all()
