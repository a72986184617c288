"""CPU-only checks of tests/offgrad_oracle.py, the float64 restatement that tests/test_gpu_offgrad.py holds libatacom_offgrad.so
to: it equals torch's float64 autograd of the two loss expressions of examples/td3_air_hockey.py (modules composed of
nn.Linear) to 1e-12 of scale; torch's own float32 autograd lies inside its float32 bound on every element; and the bound is not
vacuous -- three deliberately wrong restatements fall outside it on at least one element of every shape case they differ on."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import offgrad_oracle as og

CASES = [c + (mm,) for c in og.SHAPE_CASES for mm in og.MEAN_MODES]
IDS = ['%s-%d-%d-%s-%s-%s-mm%d' % (c[:6] + (c[6],)) for c in CASES]


def _lin(W, b, dtype):
    lay = nn.Linear(W.shape[1], W.shape[0], bias=b is not None)
    with torch.no_grad():
        lay.weight.copy_(torch.as_tensor(np.asarray(W, dtype=np.float64)))
        if b is not None:
            lay.bias.copy_(torch.as_tensor(np.asarray(b, dtype=np.float64)))
    return lay.to(dtype)


def _t(v, dtype):
    return None if v is None else torch.as_tensor(np.asarray(v, dtype=np.float64)).to(dtype)


class Actor(nn.Module):                    # examples/td3_air_hockey.py's Actor, with the normalisation and both mean modes
    def __init__(self, net, mean_mode, dtype):
        super().__init__()
        self._h1, self._h2, self._h3 = _lin(net['W1'], net['b1'], dtype), _lin(net['W2'], net['b2'], dtype), _lin(net['W3'], net['b3'], dtype)
        self.shift, self.scale, self.s = _t(net.get('obs_shift'), dtype), _t(net.get('obs_scale'), dtype), _t(net.get('act_scale'), dtype)
        self.act = torch.relu if net['activation'] == 'relu' else torch.tanh
        self.mean_mode = mean_mode

    def forward(self, x):
        if self.shift is not None:
            x = (x - self.shift) * self.scale
        m = self._h3(self.act(self._h2(self.act(self._h1(x)))))
        if not self.mean_mode:
            return m
        return torch.tanh(m) if self.s is None else self.s * torch.tanh(m)


class Critic(nn.Module):                   # examples/td3_air_hockey.py's Critic (TD3) and the reference's DDPG critic
    def __init__(self, c, dtype):
        super().__init__()
        self._h1, self._h2_s, self._h2_a, self._h3 = (_lin(c['W1'], c['b1'], dtype), _lin(c['W2'], c['b2'], dtype),
                                                      _lin(c['W2a'], None, dtype), _lin(c['W3'], c['b3'], dtype))
        self.shift, self.scale, self.s = _t(c.get('obs_shift'), dtype), _t(c.get('obs_scale'), dtype), _t(c.get('act_scale'), dtype)
        self.act = torch.relu if c['activation'] == 'relu' else torch.tanh
        self.kind = c['kind']

    def forward(self, s, a):
        if self.shift is not None:
            s = (s - self.shift) * self.scale
        if self.s is not None:
            a = a / self.s
        h1 = self.act(self._h1(torch.cat((s, a), -1) if self.kind == og.TD3 else s))
        return self._h3(self.act(self._h2_s(h1) + self._h2_a(a))).squeeze(-1)


def _grads(loss, layers):
    loss.backward()
    return np.concatenate([p.grad.detach().double().numpy().reshape(-1) for lay in layers for p in lay.parameters()])


def autograd_critic(c, cr, dtype, idx=None):
    net = Critic(cr, dtype)
    x, a, t = _t(c['obs'], dtype), _t(c['action'], dtype), _t(c['target'], dtype)
    if idx is not None:
        x, a = x[torch.as_tensor(idx)], a[torch.as_tensor(idx)]
    loss = ((net(x, a) - t) ** 2).mean()
    g = _grads(loss, (net._h1, net._h2_s, net._h3, net._h2_a))          # W1, b1, W2, b2, W3, b3, W2a: the library's order
    return g, float(loss.detach())


def autograd_actor(c, dtype, idx=None):
    """-> (gradient, loss, action, dq/da): the loss expression's autograd, with the two intermediates that the chain is cut at."""
    actor, critic = Actor(c['actor'], c['mean_mode'], dtype), Critic(c['critics'][0], dtype)
    x = _t(c['obs'], dtype)
    if idx is not None:
        x = x[torch.as_tensor(idx)]
    a = actor(x)
    a.retain_grad()
    loss = -critic(x, a).mean()
    g = _grads(loss, (actor._h1, actor._h2, actor._h3))
    return g, float(loss.detach()), a.detach().double().numpy(), -a.grad.double().numpy() * x.shape[0]


def held(got, want, dtype, c, idx):
    """What a float32 evaluation of the actor's gradient is held to (offgrad_oracle.case says why): its action inside the
    actor's forward bound; its dq/da inside the bound of dq/da at ITS action taken as exact; its gradient inside the bound of
    the actor's backward pass from ITS dq/da taken as exact; and, where the end-to-end bound covers every row, inside that."""
    g, loss, a, dq = got
    assert np.all(np.abs(a - want['a']) <= want['e_a'])
    at = og.actor_gradient(c['actor'], c['critics'][0], c['obs'], c['mean_mode'], idx, action=a)
    assert at['kinks'] == 0
    assert np.all(np.abs(dq - at['dqda']) <= at['e_dqda'])
    assert abs(loss - at['stats'][0]) <= at['stats_bound'][0]
    frm = og.actor_gradient(c['actor'], c['critics'][0], c['obs'], c['mean_mode'], idx, dqda=dq)
    assert frm['kinks'] == 0
    ok, worst = og.inside(g, frm)
    assert ok, worst
    if want['kinks'] == 0:
        ok, worst = og.inside(g, want)
        assert ok, worst
        assert np.all(np.abs(dq - want['dqda']) <= want['e_dqda']) and abs(loss - want['stats'][0]) <= want['stats_bound'][0]


@pytest.mark.parametrize('shape', CASES, ids=IDS)
def test_the_restatement_is_float64_autograd_and_float32_autograd_is_inside_the_bound(shape):
    *sh, mm = shape
    seed = og.SHAPE_SEEDS[og.SHAPE_CASES.index(tuple(sh))]
    for n_idx in (0, 40):                                 # every row in order; 40 rows through idx, with repeats
        c = og.case(seed, *sh, 65, mean_mode=mm, n_idx=n_idx)
        assert not og.row_kinks(c).any() and all(w['kinks'] == 0 for w in c['want_critic'])
        assert c['want_actor']['kinks'] == 0 or sh[3] == 'relu'
        if n_idx:
            assert len(set(c['idx'].tolist())) < n_idx
        for cr, want in zip(c['critics'], c['want_critic']):
            g64, l64 = autograd_critic(c, cr, torch.float64, c['idx'])
            assert np.all(np.abs(g64 - want['flat']) <= 1e-12 * want['scale'] + 1e-14)
            assert abs(l64 - want['stats'][0]) <= 1e-12 * want['stats_scale'][0] + 1e-14
            g32, l32 = autograd_critic(c, cr, torch.float32, c['idx'])
            ok, worst = og.inside(g32, want)
            assert ok, worst
            assert abs(l32 - want['stats'][0]) <= want['stats_bound'][0]
        want = c['want_actor']
        g64, l64, a64, dq64 = autograd_actor(c, torch.float64, c['idx'])
        assert np.all(np.abs(g64 - want['flat']) <= 1e-12 * want['scale'] + 1e-14)
        assert abs(l64 - want['stats'][0]) <= 1e-12 * want['stats_scale'][0] + 1e-14
        assert np.all(np.abs(a64 - want['a']) <= 1e-12 * want['scale_a'] + 1e-14)
        assert np.all(np.abs(dq64 - want['dqda']) <= 1e-12 * want['scale_dqda'] + 1e-14)
        held(autograd_actor(c, torch.float32, c['idx']), want, np.float32, c, c['idx'])


@pytest.mark.parametrize('shape', og.SHAPE_CASES, ids=['-'.join(str(v) for v in s) for s in og.SHAPE_CASES])
def test_the_bound_is_not_vacuous(shape):
    """A wrong restatement falls outside the bound of the right one on at least one element.  A restatement that does not
    differ from the right one on a case cannot: the 1 / act_scale without an act_scale, the as columns of a DDPG critic."""
    kind, D, k, act, norm, scaled = shape
    c = og.case(og.SHAPE_SEEDS[og.SHAPE_CASES.index(shape)], *shape, 65)
    want = c['want_actor']
    for wrong, differs in (('no_w2a', True), ('no_scale', scaled)):
        bad = og.actor_gradient(c['actor'], c['critics'][0], c['obs'], c['mean_mode'], wrong=wrong)
        for key, bound in (('flat', 'bound'), ('dqda', 'e_dqda')):
            out = np.abs(bad[key] - want[key]) > want[bound]
            assert out.any() == differs, (wrong, key)
    for cr, want in zip(c['critics'], c['want_critic']):
        bad = og.critic_gradient(cr, c['obs'], c['action'], c['target'], wrong='no_as_cols')
        out = np.abs(bad['flat'] - want['flat']) > want['bound']
        assert out.any() == (kind == og.TD3)


def test_a_given_action_and_a_given_dqda_cut_the_chain():
    """The two sharper references of the GPU test: dq/da at an action taken as exact carries no actor error, and the actor's
    gradient from a dq/da taken as exact carries no critic error; from the oracle's own values both reproduce it."""
    c = og.case(og.SHAPE_SEEDS[5], *og.SHAPE_CASES[5], 65)            # tanh: act' carries the forward error
    want = c['want_actor']
    at = og.actor_gradient(c['actor'], c['critics'][0], c['obs'], 1, action=want['a'])
    assert np.allclose(at['dqda'], want['dqda'], rtol=0, atol=1e-15) and np.all(at['e_dqda'] <= want['e_dqda']) and np.any(at['e_dqda'] < want['e_dqda'])
    frm = og.actor_gradient(c['actor'], c['critics'][0], c['obs'], 1, dqda=want['dqda'])
    assert np.allclose(frm['flat'], want['flat'], rtol=0, atol=1e-15) and np.all(frm['bound'] <= want['bound']) and np.any(frm['bound'] < want['bound'])


def test_row_cases_have_no_kinks():
    """What the GPU row cases stand on, asserted here so that the reference alone satisfies it."""
    for rows in sorted({r for r, _ in og.ROW_CASES}):
        c = og.case(300 + rows, *og.ROW_SHAPE, rows)
        assert not og.row_kinks(c).any() and all(w['kinks'] == 0 for w in c['want_critic'])
        want = c['want_actor']
        assert og.actor_gradient(c['actor'], c['critics'][0], c['obs'], 1, action=want['a'])['kinks'] == 0
        assert og.actor_gradient(c['actor'], c['critics'][0], c['obs'], 1, dqda=want['dqda'])['kinks'] == 0
