"""CPU-only checks of tests/evaluate_oracle.py, the float64 restatement libatacom_evaluate.so is held to: it IS torch.nn's
network and torch.distributions' Gaussian (pinned, to 1e-12), and its float32 bound is one that torch's own float32 arithmetic
keeps on every sample of the cases the GPU tests run -- a bound the reference arithmetic itself broke would prove nothing."""
import numpy as np
import pytest

import evaluate_oracle as eo

torch = pytest.importorskip('torch')


def _module(net, dtype):
    """The torch.nn restatement: Linear - act - Linear - act - Linear on the normalised input."""
    lins = []
    for Wk, bk in (('W1', 'b1'), ('W2', 'b2'), ('W3', 'b3')):
        W = torch.as_tensor(np.asarray(net[Wk])).to(dtype)
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).to(dtype)
        with torch.no_grad():
            lin.weight.copy_(W)
            lin.bias.copy_(torch.as_tensor(np.asarray(net[bk])).to(dtype))
        lins.append(lin)
    act = torch.nn.ReLU() if net['activation'] == 'relu' else torch.nn.Tanh()
    seq = torch.nn.Sequential(lins[0], act, lins[1], act, lins[2])
    shift = 0.0 if net['obs_shift'] is None else torch.as_tensor(net['obs_shift']).to(dtype)
    scale = 1.0 if net['obs_scale'] is None else torch.as_tensor(net['obs_scale']).to(dtype)
    return lambda x: seq((x.to(dtype) - shift) * scale)


def _torch_results(case, dtype):
    net, x, action, std = eo.case_data(7, *case)
    with torch.no_grad():
        y = _module(net, dtype)(torch.as_tensor(x))
        s = torch.as_tensor(std).to(dtype)
        lp = torch.distributions.MultivariateNormal(y, torch.diag(s * s)).log_prob(torch.as_tensor(action).to(dtype))
    return (net, x, action, std), y.numpy().astype(np.float64), lp.numpy().astype(np.float64)


@pytest.mark.parametrize('case', eo.SHAPE_CASES, ids=str)
def test_the_oracle_is_torch_in_float64(case):
    (net, x, action, std), y_t, lp_t = _torch_results(case, torch.float64)
    lp, _, _, y, _ = eo.log_prob(net, x, action, std)
    assert np.abs(y - y_t).max() <= 1e-12 * max(1.0, np.abs(y_t).max())
    assert np.abs(lp - lp_t).max() <= 1e-12 * max(1.0, np.abs(lp_t).max())


@pytest.mark.parametrize('case', eo.SHAPE_CASES + [eo.SHAPE_CASES[3][:4] + (r,) for r in sorted({r for r, _ in eo.ROW_CASES})], ids=str)
def test_torch_float32_keeps_the_float32_bound_on_every_sample(case):
    (net, x, action, std), y_t, lp_t = _torch_results(case, torch.float32)
    lp, e_lp, _, y, e_y = eo.log_prob(net, x, action, std)
    worst_y, worst_lp = (np.abs(y_t - y) / e_y).max(), (np.abs(lp_t - lp) / e_lp).max()
    print('%s: torch float32 uses %.3f of the bound on the mean, %.3f on logp' % (case, worst_y, worst_lp))
    assert (np.abs(y_t - y) <= e_y).all() and (np.abs(lp_t - lp) <= e_lp).all()


def test_the_bound_grows_with_what_it_should():
    """Larger output weights raise the bound in proportion; a zero network has the bias's rounding alone."""
    rng = np.random.default_rng(0)
    net = eo.random_net(rng, 8, 2, 'relu', normalise=False)
    x = rng.normal(0, 1, (5, 8)).astype(np.float32)
    _, e0, _ = eo.forward(net, x)
    _, e1, _ = eo.forward(dict(net, W3=net['W3'] * 4), x)
    assert (e1 > 2 * e0).all() and (e1 <= 4 * e0).all()
    zero = {k: np.zeros_like(v) if isinstance(v, np.ndarray) else v for k, v in net.items()}
    zero['b3'] = np.ones(2, np.float32)
    y, e, _ = eo.forward(zero, x)
    assert np.array_equal(y, np.ones((5, 2))) and np.allclose(e, eo.SAFETY * eo.gamma(65), rtol=1e-12)
