"""CPU-only checks of tests/soft_oracle.py, the float64 restatement that the GPU tests of libatacom_soft.so compare against:
it equals torch modules, torch.distributions.Normal(...).rsample / log_prob and float64 autograd (the target, both losses'
gradients and the alpha gradient) to 1e-12 of scale; its cases keep log sigma where torch's own (u - m) / s holds those digits
and the bound on logp small on every row; the saturation case is finite and inside the per-sample allowance; and six deliberately
wrong restatements fall outside the float32 bound."""
import numpy as np
import pytest
import torch

import soft_oracle as so

CASES = [(11, 18, 5, 'relu', True, True, 65, 0), (12, 12, 3, 'tanh', False, False, 65, 0), (13, 18, 5, 'relu', True, True, 200, 48),
         (14, 4, 1, 'tanh', True, True, 17, 0)]


def _t(a):
    return None if a is None else torch.tensor(np.asarray(a, dtype=np.float64))


def _net(d):
    p = {k: _t(d[k]).requires_grad_(True) for k in so.PARAMS}
    return p, _t(d.get('obs_shift')), _t(d.get('obs_scale')), (torch.relu if d.get('activation', 'relu') == 'relu' else torch.tanh)


def _mlp(net, x):
    p, shift, scale, act = net
    return _mlp_in(net, (x - (0.0 if shift is None else shift)) * (1.0 if scale is None else scale))


def _mlp_in(net, h):
    p, _, _, act = net
    h = act(h @ p['W1'].T + p['b1'])
    h = act(h @ p['W2'].T + p['b2'])
    return h @ p['W3'].T + p['b3']


def _critic(net, x, a):
    _, shift, scale, _ = net
    xn = (x - (0.0 if shift is None else shift)) * (1.0 if scale is None else scale)
    return _mlp_in(net, torch.cat([xn, a], 1))[:, 0]


def _sample(c, mu, sigma, x, eps, monkeypatch):
    """MushroomRL's SACPolicy.compute_action_and_log_prob_t through torch.distributions, the draw replaced by the case's eps."""
    monkeypatch.setattr(torch.distributions.normal, '_standard_normal', lambda shape, dtype, device: eps)
    m, lr = _mlp(mu, x), _mlp(sigma, x)
    l = torch.clamp(lr, c['policy']['log_std_min'], c['policy']['log_std_max'])
    dist = torch.distributions.Normal(m, l.exp())
    u = dist.rsample()
    t = torch.tanh(u)
    k = eps.shape[1]
    a = t * _t(so._vec(c['act_scale'], k)) + _t(so._vec(c['act_shift'], k, 0.0))
    logp = dist.log_prob(u).sum(1) - torch.log(1.0 - t.pow(2) + 1e-6).sum(1)
    return a, logp, l


def _flat(net):
    return np.concatenate([net[0][k].grad.numpy().reshape(-1) for k in so.PARAMS])


def _close(got, want, scale, what):
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(-1) - np.asarray(want).reshape(-1))
    allow = 1e-12 * np.asarray(scale).reshape(-1) + 1e-14
    assert (err <= allow).all(), (what, float((err / allow).max()))


@pytest.mark.parametrize('seed,D,k,act,norm,with_act,rows,n_idx', CASES)
def test_the_restatement_equals_torch_distributions_and_float64_autograd(seed, D, k, act, norm, with_act, rows, n_idx, monkeypatch):
    c = so.case(seed, D, k, act, norm, with_act, rows, np.float64, n_idx)
    idx = c['idx']
    g = (lambda a: _t(a) if idx is None else _t(a)[torch.tensor(idx)])
    x, eps = g(c['obs']), _t(c['eps'])
    al = torch.tensor(c['log_alpha'], dtype=torch.float64, requires_grad=True)
    # ---- the target, with the target critics
    mu, sigma = _net(c['policy']['mu']), _net(c['policy']['sigma'])
    tq = [_net(cr) for cr in c['targets']]
    with torch.no_grad():
        a, logp, l = _sample(c, mu, sigma, x, eps, monkeypatch)
        assert so.LOG_STD_RANGE[0] <= float(l.min()) and float(l.max()) <= so.LOG_STD_RANGE[1]
        qmin = torch.minimum(_critic(tq[0], x, a), _critic(tq[1], x, a))
        y = g(c['reward']) + c['gamma'] * (1.0 - g(c['absorbing'])) * (qmin - al.exp() * logp)
    w = c['want_target']
    _close(y.numpy(), w['y'].v, w['y'].s, 'y')
    _close(a.numpy(), w['a'].v, w['a'].s, 'a')
    _close(logp.numpy(), w['logp'].v, w['logp'].s, 'logp')
    # ---- the critics' gradients
    for j, cr in enumerate(c['critics']):
        net = _net(cr)
        loss = ((_critic(net, x, g(c['action'])) - _t(c['target'])) ** 2).mean()
        loss.backward()
        wc = c['want_critic'][j]
        _close(_flat(net), wc['flat'], wc['scale'], 'critic %d' % j)
        _close(loss.item(), wc['stats'][0], wc['stats_scale'][0], 'critic loss')
    # ---- the actor's gradients and the alpha gradient
    cq = [_net(cr) for cr in c['critics']]
    a, logp, _ = _sample(c, mu, sigma, x, eps, monkeypatch)
    q1, q2 = _critic(cq[0], x, a), _critic(cq[1], x, a)
    assert float((q1 - q2).detach().abs().min()) > 0.0                              # no case has a tie
    loss = (al.exp().detach() * logp - torch.minimum(q1, q2)).mean()
    loss.backward()
    wa = c['want_actor']
    _close(_flat(mu), wa['mu']['flat'], wa['mu']['scale'], 'mu')
    _close(_flat(sigma), wa['sigma']['flat'], wa['sigma']['scale'], 'sigma')
    _close(loss.item(), wa['stats'][0], wa['stats_scale'][0], 'actor loss')
    _close(logp.mean().item(), wa['stats'][1], wa['stats_scale'][1], 'mean logp')
    aloss = -(al * (logp + c['target_entropy']).detach()).mean()
    aloss.backward()
    _close(al.grad.item(), wa['stats'][2], wa['stats_scale'][2], 'alpha gradient')
    # rows beyond both clamp bounds are present (and Mu still receives du there)
    if rows >= 64:
        lr, pol = wa['lr'].v, c['policy']
        assert (lr < pol['log_std_min']).any() and (lr > pol['log_std_max']).any() and wa['open'].any() and wa['stats'][3] > 0.0


def test_the_saturation_case_is_finite_and_inside_the_per_sample_allowance(monkeypatch):
    c = so.case(21, 18, 5, 'tanh', True, True, 65, np.float64, 0, True)
    w = c['want_target']
    assert float(np.abs(w['u'].v).max()) > 5.0                              # it saturates
    x, eps = _t(c['obs']), _t(c['eps'])
    mu, sigma = _net(c['policy']['mu']), _net(c['policy']['sigma'])
    with torch.no_grad():
        a, logp, _ = _sample(c, mu, sigma, x, eps, monkeypatch)
    sat = so.sample(c['policy'], c['obs'], c['eps'], c['act_scale'], c['act_shift'])['sat'].sum(1)
    ok, worst = so.inside_v(logp.numpy(), w['logp'], np.float64, extra=sat)
    assert ok and np.isfinite(w['logp'].v).all() and np.isfinite(w['logp'].e).all(), worst
    for part in ('mu', 'sigma'):
        assert np.isfinite(c['want_actor'][part]['flat']).all() and np.isfinite(c['want_actor'][part]['bound']).all()


WRONG_ACTOR = ('no_alpha', 'no_gate', 'larger', 'no_1e6', 'no_scale')


def _policy_for(c, wrong):
    """The case's policy -- for the omitted 1e-6, with one element of mu pushed to u >= 20, where tanh(u) is exactly 1 in either
    precision and w exactly 0: there the 1e-6 is all that keeps log(w + 1e-6) and 2 t w / (w + 1e-6) finite.  (Below saturation the
    omission moves w by 1e-6, three times the 3e-7 that the float32 tanh is allowed: no float32 bound can tell them apart.)"""
    pol = c['policy']
    if wrong != 'no_1e6':
        return pol
    mu = dict(pol['mu'])
    mu['b3'] = mu['b3'].copy()
    mu['b3'][0] += 40.0
    return dict(pol, mu=mu)


@pytest.mark.parametrize('wrong', WRONG_ACTOR)
def test_a_wrong_actor_gradient_falls_outside_the_float32_bound(wrong):
    c = so.case(11, 18, 5, 'relu', True, True, 65, np.float32)
    pol = _policy_for(c, wrong)
    args = (pol, c['critics'], c['obs'], c['eps'], c['log_alpha'], c['target_entropy'], c['act_scale'], c['act_shift'])
    with np.errstate(all='ignore'):
        w = c['want_actor'] if pol is c['policy'] else so.actor_gradient(*args)
        bad = so.actor_gradient(*args, wrong=wrong)
    assert all(np.isfinite(w[p]['flat']).all() and np.isfinite(w[p]['bound']).all() for p in ('mu', 'sigma'))
    out = [not so.inside(bad[p]['flat'], w[p], np.float32)[0] for p in ('mu', 'sigma')]
    assert any(out), wrong


@pytest.mark.parametrize('wrong', ('larger', 'no_1e6', 'absorbing'))
def test_a_wrong_target_falls_outside_the_float32_bound(wrong):
    c = so.case(11, 18, 5, 'relu', True, True, 65, np.float32)
    pol = _policy_for(c, wrong)
    args = (pol, c['targets'], c['obs'], c['reward'], c['absorbing'], c['gamma'], c['log_alpha'], c['eps'], c['act_scale'], c['act_shift'])
    with np.errstate(all='ignore'):
        want = c['want_target'] if pol is c['policy'] else so.target(*args)
        bad = so.target(*args, wrong=wrong)
    assert (c['absorbing'] > 0.5).any() and np.isfinite(want['y'].v).all() and np.isfinite(want['y'].e).all()
    assert not so.inside_v(bad['y'].v, want['y'], np.float32)[0], wrong
