"""CPU-only checks of tests/edge_cases.py, the cases that sit exactly on a ReLU kink (K1, K2), a tie of the two critics (T), a
clamp bound of log sigma (C) and the absorbing threshold (A), and of what the oracles say there.  For every construction and every
module it applies to:
  * the premise holds in float32 numpy and in float64: the engineered pre-activations are exactly 0, q_1 == q_2 bit for bit,
    l_raw == the bound;
  * the oracle equals a float64 torch autograd evaluation on which the project's convention is imposed.  At K1, K2 and A that is
    torch's own answer (relu'(0) = 0; the reference's flag is a bool).  At T and C it is not: torch.min splits the gradient
    0.5 / 0.5 at a tie and torch.clamp passes it at x == min and x == max; the tests show both differences and their size
    (include/atacom_soft_hip.h and DESIGN.md section 7h state the two departures);
  * each wrong= variant of the oracles (the gate `h >= 0`, critic 2 at a tie, an inclusive clamp gate, `absorbing >= 0.5`, applied
    to the engineered units, rows and elements only) falls outside the float32 bound on the named elements: a device that made the
    mistake would fail tests/test_gpu_gradient_edges.py."""
import numpy as np
import pytest
import torch

import edge_cases as ec
import fit_oracle as fo
import offgrad_oracle as og
import soft_oracle as so
import trust_oracle as to
from test_fit_oracle import torch_gradient
from test_offgrad_oracle import autograd_actor, autograd_critic
from test_soft_oracle import _close, _critic, _flat, _mlp, _net, _t
from test_trust_oracle import torch_fvp

F32, F64 = np.float32, np.float64
KINKS = [(n,) + p for n in ('K1', 'K2') for p in ec.PAIRS]
KINK_IDS = ['%s-%d-%d' % k for k in KINKS]


def _premise(name, net, x, j1, j2, a=None):
    """K1: a1[:, j1] == a2[:, j2] == 0 on every row.  K2: a1[:, j1] is exactly 0 on S_ROWS, positive on the other odd rows,
    negative on the other even rows, and a2[:, j2] == relu(a1[:, j1]) bit for bit.  In float32 numpy and in float64."""
    for dt in (F32, F64):
        a1, a2 = ec.pre_activations(net, x, a, dt)
        if name == 'K1':
            assert (a1[:, j1] == 0).all() and (a2[:, j2] == 0).all()
        else:
            kind = ec.row_kind(x, net['obs_shift'])
            S = np.zeros(ec.ROWS, bool)
            S[list(ec.S_ROWS)] = True
            odd = np.arange(ec.ROWS) % 2 == 1
            assert np.array_equal(kind == 0, S) and (kind[~S & odd] > 0).all() and (kind[~S & ~odd] < 0).all()
            assert np.array_equal(np.sign(a1[:, j1]).astype(int), kind) and (np.abs(a1[~S, j1]) > 0.05).all()
            assert np.array_equal(a2[:, j2], np.maximum(a1[:, j1], 0))
            assert (a2[kind <= 0, j2] == 0).all() and (a2[kind > 0, j2] > 0).all()


def _f64_close(got, want, what):
    err = np.abs(np.asarray(got, F64).reshape(-1) - want['flat'])
    allow = 1e-12 * want['scale'] + 1e-14
    assert (err <= allow).all(), (what, float((err / allow).max()))


def _outside(name, bad, want, n_in, j1, j2, w2a=0, bound='bound'):
    """The named elements: K1 -- the slices that are exactly 0 (value and bound) and no longer are; K2 -- db1[j1] and db2[j2]."""
    flat, e = want['flat'], want[bound]
    if name == 'K1':
        sl = ec.unit_slices(n_in, j1, j2, w2a)
        assert (flat[sl] == 0).all() and (e[sl] == 0).all()
        o_b1, o_W2 = 64 * n_in, 64 * n_in + 64
        groups = [np.arange(j1 * n_in, (j1 + 1) * n_in), np.arange(o_W2 + 64 * j2, o_W2 + 64 * (j2 + 1))] + ([sl[-w2a:]] if w2a else [])
        assert all((bad[g] != 0).any() for g in groups)
    b = ec.bias_slots(n_in, j1, j2)
    assert (np.abs(bad[b] - flat[b]) > e[b]).all(), (name, bad[b], flat[b], e[b])


# ------------------------------------------------------------------------------------------------------------ K1 and K2
@pytest.mark.parametrize('head', [fo.VALUE, fo.PPO_CLIP], ids=['value', 'ppo'])
@pytest.mark.parametrize('name,j1,j2', KINKS, ids=KINK_IDS)
def test_fit_at_a_kink(name, j1, j2, head):
    for dt in (F32, F64):
        c = ec.fit_case(name, j1, j2, head, dt)
        assert c['want']['kinks'] == 0 and fo.oracle(dict(c, exempt=None), head)['kinks'] > 0
        _premise(name, c['net'], c['x'], j1, j2)
    got, stats = torch_gradient(c, head, torch.float64)                    # torch's own answer: relu'(0) = 0
    _f64_close(got, c['want'], (name, head))
    c32 = ec.fit_case(name, j1, j2, head, F32)
    _outside(name, fo.oracle(c32, head, wrong='kink_open')['flat'], c32['want'], fo.ROW_SHAPE[head][0], j1, j2)


@pytest.mark.parametrize('name,j1,j2', KINKS, ids=KINK_IDS)
def test_trust_at_a_kink(name, j1, j2):
    n_in = to.ROW_SHAPE[0]
    for dt in (F32, F64):
        c = ec.trust_case(name, j1, j2, dt)
        assert c['want']['kinks'] == 0 and to.fvp(c['net'], c['std'], c['x'], c['v'], c['damping'])['kinks'] > 0
        _premise(name, c['net'], c['x'], j1, j2)
        v = c['v'][ec.unit_slices(n_in, j1, j2)]
        assert (v != 0).all()                                              # the direction is not zero on the engineered components
    _f64_close(torch_fvp(c, torch.float64, c['damping']), c['want'], name)
    c32 = ec.trust_case(name, j1, j2, F32)
    bad = to.fvp(c32['net'], c32['std'], c32['x'], c32['v'], c32['damping'], mistake='kink_open', exempt=c32['exempt'])['flat']
    _outside(name, bad, c32['want'], n_in, j1, j2)


@pytest.mark.parametrize('kind', [og.DDPG, og.TD3])
@pytest.mark.parametrize('name,j1,j2', KINKS, ids=KINK_IDS)
def test_offgrad_critics_at_a_kink(name, j1, j2, kind):
    for dt in (F32, F64):
        c = ec.offgrad_case(name, 'critics', j1, j2, kind, dt)
        assert og.row_kinks(c).any() and not og.row_kinks(c, c['exempt']).any()
        for cr in c['critics']:
            assert (cr['W2a'][j2] == 0).all() and (cr['W2a'] != 0).any()
            _premise(name, cr, c['obs'], j1, j2, c['action'])
    # torch's own answer, on the float32 case's values (test_offgrad_oracle's modules hold float32-representable weights)
    c = ec.offgrad_case(name, 'critics', j1, j2, kind, F32)
    n1 = c['critics'][0]['W1'].shape[1]
    for j, (cr, want) in enumerate(zip(c['critics'], c['want_critic'])):
        _f64_close(autograd_critic(c, cr, torch.float64)[0], want, (name, kind, j))
    g, loss, a, dq = autograd_actor(c, torch.float64)
    _f64_close(g, c['want_actor'], (name, kind, 'actor'))
    assert (np.abs(dq - c['want_actor']['dqda']) <= 1e-12 * c['want_actor']['scale_dqda'] + 1e-14).all()
    c32 = ec.offgrad_case(name, 'critics', j1, j2, kind, F32)
    for j, (cr, want) in enumerate(zip(c32['critics'], c32['want_critic'])):
        bad = og.critic_gradient(cr, c32['obs'], c32['action'], c32['target'], wrong='kink_open', exempt=c32['exempt']['critics'][j])['flat']
        _outside(name, bad, want, n1, j1, j2, c32['k'])


@pytest.mark.parametrize('name,j1,j2', KINKS, ids=KINK_IDS)
def test_offgrad_actor_at_a_kink(name, j1, j2):
    for dt in (F32, F64):
        c = ec.offgrad_case(name, 'actor', j1, j2, og.TD3, dt)
        assert og.row_kinks(c).any() and not og.row_kinks(c, c['exempt']).any()
        _premise(name, c['actor'], c['obs'], j1, j2)
    c32 = ec.offgrad_case(name, 'actor', j1, j2, og.TD3, F32)
    _f64_close(autograd_actor(c32, torch.float64)[0], c32['want_actor'], name)
    at = og.actor_gradient(c32['actor'], c32['critics'][0], c32['obs'], 1, dqda=c32['want_actor']['dqda'], exempt=c32['exempt'])
    bad = og.actor_gradient(c32['actor'], c32['critics'][0], c32['obs'], 1, dqda=c32['want_actor']['dqda'], exempt=c32['exempt'], wrong='kink_open')
    assert at['kinks'] == 0
    _outside(name, bad['flat'], at, c32['D'], j1, j2)


def _soft_sample(c, mu, sigma, x, eps, strict):
    """test_soft_oracle._sample written out (rsample is m + s eps), with the clamp's gradient torch's own (inclusive at both
    bounds) or, `strict`, the project's: the clamped value's gradient passes only where lmin < l_raw < lmax."""
    m, lr = _mlp(mu, x), _mlp(sigma, x)
    lmin, lmax = c['policy']['log_std_min'], c['policy']['log_std_max']
    l = torch.clamp(lr, lmin, lmax)
    if strict:
        l = torch.where((lmin < lr) & (lr < lmax), lr, l.detach())
    s = l.exp()
    u = m + s * eps
    t = torch.tanh(u)
    k = eps.shape[1]
    a = t * _t(so._vec(c['act_scale'], k)) + _t(so._vec(c['act_shift'], k, 0.0))
    logp = torch.distributions.Normal(m, s).log_prob(u).sum(1) - torch.log(1.0 - t.pow(2) + 1e-6).sum(1)
    return a, logp, lr


def _soft_actor_torch(c, strict_clamp=True, first_at_tie=True):
    """float64 autograd of SAC's actor loss -> (mu flat, sigma flat, q1, q2, l_raw)."""
    x, eps = _t(c['obs']), _t(c['eps'])
    mu, sigma = _net(c['policy']['mu']), _net(c['policy']['sigma'])
    cq = [_net(cr) for cr in c['critics']]
    a, logp, lr = _soft_sample(c, mu, sigma, x, eps, strict_clamp)
    q1, q2 = _critic(cq[0], x, a), _critic(cq[1], x, a)
    q = torch.where(q2 < q1, q2, q1) if first_at_tie else torch.minimum(q1, q2)
    (np.exp(c['log_alpha']) * logp - q).mean().backward()
    return _flat(mu), _flat(sigma), q1.detach().numpy(), q2.detach().numpy(), lr.detach().numpy()


def _soft_critics_torch(c):
    x = _t(c['obs'])
    for j, cr in enumerate(c['critics']):
        net = _net(cr)
        ((_critic(net, x, _t(c['action'])) - _t(c['target'])) ** 2).mean().backward()
        _f64_close(_flat(net), c['want_critic'][j], ('critic', j))


@pytest.mark.parametrize('which', ['policy', 'critics'])
@pytest.mark.parametrize('name,j1,j2', KINKS, ids=KINK_IDS)
def test_soft_at_a_kink(name, j1, j2, which):
    D, k = ec.SOFT_SHAPE
    for dt in (F32, F64):
        c = ec.soft_case(name, which, j1, j2, 'relu', dt)
        assert so.row_flags(c).any() and not so.row_flags(c, c['exempt']).any()
        w = c['want_actor']
        assert not w['kink'].any() and not w['tie'].any() and not w['edge'].any()
        if which == 'policy':
            for net in (c['policy']['mu'], c['policy']['sigma']):
                _premise(name, net, c['obs'], j1, j2)
        else:
            for cr in c['critics'] + c['targets']:
                _premise(name, cr, c['obs'], j1, j2, c['action'])
                _premise(name, cr, c['obs'], j1, j2, w['a'].v)
    gm, gs = _soft_actor_torch(c, strict_clamp=False, first_at_tie=False)[:2]          # torch's own answer
    _f64_close(gm, w['mu'], (name, which, 'mu'))
    _f64_close(gs, w['sigma'], (name, which, 'sigma'))
    _soft_critics_torch(c)
    c32 = ec.soft_case(name, which, j1, j2, 'relu', F32)
    if which == 'policy':
        w = c32['want_actor']
        frm = so.actor_gradient(*ec.soft_actor_args(c32), dq=w['dqda'].v, exempt=c32['exempt'])
        bad = so.actor_gradient(*ec.soft_actor_args(c32), dq=w['dqda'].v, exempt=c32['exempt'], wrong='kink_open')
        for part in ('mu', 'sigma'):
            _outside(name, bad[part]['flat'], frm[part], D, j1, j2)
    else:
        for j, cr in enumerate(c32['critics']):
            bad = so.critic_gradient(cr, c32['obs'], c32['action'], c32['target'], exempt=c32['exempt']['critics'][j], wrong='kink_open')
            _outside(name, bad['flat'], c32['want_critic'][j], D + k, j1, j2)


@pytest.mark.parametrize('j1,j2', ec.PAIRS)
def test_soft_critic_unit_dead_through_a_zero_action_element(j1, j2):
    """K1 with W1[j1, D + 0] kept: the unit is dead because the action's element 0 is exactly 0, and its gate alone keeps
    W1[j1, D + 0] out of dq/da_0."""
    D, k = ec.SOFT_SHAPE
    for dt in (F32, F64):
        c = ec.soft_case('K1', 'critics_a0', j1, j2, 'relu', dt)
        w = c['want_actor']
        assert (w['a'].v[:, 0] == 0).all() and (c['action'][:, 0] == 0).all() and all(cr['W1'][j1, D] != 0 for cr in c['critics'])
        for cr in c['critics'] + c['targets']:
            _premise('K1', cr, c['obs'], j1, j2, c['action'])
            _premise('K1', cr, c['obs'], j1, j2, w['a'].v.astype(dt))
    gm, gs = _soft_actor_torch(c, strict_clamp=False, first_at_tie=False)[:2]
    _f64_close(gm, w['mu'], 'mu')
    _f64_close(gs, w['sigma'], 'sigma')
    c32 = ec.soft_case('K1', 'critics_a0', j1, j2, 'relu', F32)
    w = c32['want_actor']
    bad = so.actor_gradient(*ec.soft_actor_args(c32), exempt=c32['exempt'], wrong='kink_open')
    out = np.abs(bad['dqda'].v[:, 0] - w['dqda'].v[:, 0]) > w['dqda'].e[:, 0]
    print('dq/da_0 with the open gate: outside the float32 bound on %d of %d rows' % (int(out.sum()), ec.ROWS))
    assert out.sum() > ec.ROWS // 2
    assert np.array_equal(bad['dqda'].v[:, 1:], w['dqda'].v[:, 1:])


# -------------------------------------------------------------------------------------------------------------------- T
def _policy_np(c, dt):
    """(m, l_raw, a) of the case's policy in `dt` numpy arithmetic."""
    out = []
    for net in (c['policy']['mu'], c['policy']['sigma']):
        a1, a2 = ec.pre_activations(net, c['obs'], None, dt)
        out.append(np.maximum(a2, 0) @ net['W3'].astype(dt).T + net['b3'].astype(dt))
    m, lr = out
    l = np.clip(lr, dt(c['policy']['log_std_min']), dt(c['policy']['log_std_max']))
    a = c['act_scale'].astype(dt) * np.tanh(m + np.exp(l) * c['eps'].astype(dt)) + c['act_shift'].astype(dt)
    return m, lr, a.astype(dt)


def test_tie_of_the_two_critics():
    D, k = ec.SOFT_SHAPE
    tie = np.zeros(ec.ROWS, bool)
    tie[list(ec.TIE_ROWS)] = True
    for dt in (F32, F64):
        c = ec.soft_case('T', None, 5, 42, 'relu', dt)
        assert so.row_flags(c).any() and not so.row_flags(c, c['exempt']).any()
        m, lr, a = _policy_np(c, dt)
        q1, q2 = a[:, 0] + dt(4.0), a[:, 1] + dt(4.0)
        assert np.array_equal(m[:, 0], m[:, 1]) and np.array_equal(lr[:, 0], lr[:, 1])
        assert np.array_equal(q1 == q2, tie) and (q1[~tie] < q2[~tie]).any() and (q2[~tie] < q1[~tie]).any()
        for j, cr in enumerate(c['critics']):                          # the critic's own chain gives fl(a_j + 4), every unit but one dead
            a1, a2 = ec.pre_activations(cr, c['obs'], a, dt)
            assert np.array_equal(a1[:, 0], (q1, q2)[j]) and np.array_equal(a2[:, 0], (q1, q2)[j]) and (a1[:, 1:] == 0).all() and (a2[:, 1:] == 0).all()
        w = c['want_actor']
        assert np.array_equal(w['q'][0].v == w['q'][1].v, tie) and not w['tie'].any() and not w['kink'].any() and not w['edge'].any()
        e0, e1 = np.eye(k)[0], np.eye(k)[1]
        assert (w['dqda'].v[~w['two']] == e0).all() and (w['dqda'].v[w['two']] == e1).all() and not w['two'][tie].any()
    # float64 autograd with the selection imposed is the oracle; torch's own minimum is the mean of the two selections
    w = c['want_actor']
    second = so.actor_gradient(*ec.soft_actor_args(c), exempt=c['exempt'], wrong='tie_second')
    assert second['two'][tie].all() and np.array_equal(second['two'][~tie], w['two'][~tie])
    gm, gs, q1, q2, _ = _soft_actor_torch(c, first_at_tie=True)
    assert np.array_equal(q1 == q2, tie)
    _f64_close(gm, w['mu'], 'mu, critic 1 at a tie')
    _f64_close(gs, w['sigma'], 'sigma, critic 1 at a tie')
    own_m, own_s = _soft_actor_torch(c, first_at_tie=False)[:2]
    for own, part in ((own_m, 'mu'), (own_s, 'sigma')):
        half = dict(flat=0.5 * (w[part]['flat'] + second[part]['flat']), scale=w[part]['scale'] + second[part]['scale'])
        _f64_close(own, half, part + ': torch.minimum splits a tie 0.5 / 0.5')
        diff = np.abs(own - w[part]['flat'])
        print('T %s: torch.minimum differs from the device convention by up to %.3g (%.3g of the largest element)' % (
            part, diff.max(), diff.max() / np.abs(w[part]['flat']).max()))
        assert (diff > 1e-12 * w[part]['scale'] + 1e-14).any()
    # the wrong selection is outside the float32 bound: dq/da on every tie row, and the mu network's gradient
    c32 = ec.soft_case('T', None, 5, 42, 'relu', F32)
    w = c32['want_actor']
    bad = so.actor_gradient(*ec.soft_actor_args(c32), exempt=c32['exempt'], wrong='tie_second')
    assert (np.abs(bad['dqda'].v - w['dqda'].v) > w['dqda'].e)[tie][:, :2].all()
    assert not so.inside(bad['mu']['flat'], w['mu'], F32)[0]


# -------------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize('activation', ['relu', 'tanh'])
def test_log_sigma_on_a_clamp_bound(activation):
    D, k = ec.SOFT_SHAPE
    o_W3 = 64 * D + 64 + 4096 + 64
    named = np.concatenate([np.arange(o_W3, o_W3 + 128), o_W3 + 64 * k + np.arange(2)])          # dW3[0:2, :] and db3[0:2] of sigma
    for dt in (F32, F64):
        c = ec.soft_case('C', None, 5, 42, activation, dt)
        pol = c['policy']
        assert float(dt(pol['log_std_min'])) == pol['log_std_min'] and float(dt(pol['log_std_max'])) == pol['log_std_max']
        assert so.row_flags(c).any() and not so.row_flags(c, c['exempt']).any()
        sg = pol['sigma']
        f = np.tanh if activation == 'tanh' else (lambda z: np.maximum(z, 0))
        x1 = ec.first_input(sg, c['obs'], None, dt)
        lr = f(f(x1 @ sg['W1'].T + sg['b1']) @ sg['W2'].T + sg['b2']) @ sg['W3'].T + sg['b3']
        assert lr.dtype == dt and (lr[:, 0] == dt(pol['log_std_max'])).all() and (lr[:, 1] == dt(pol['log_std_min'])).all()
        w = c['want_actor']
        assert not w['edge'].any() and w['clamped'].all() and w['stats'][3] == 1.0
        assert (w['dl'].v[:, :2] == 0).all() and (w['sigma']['flat'][named] == 0).all() and (w['sigma']['bound'][named] == 0).all()
        rest = w['lr'].v[:, 2:]                                            # the other elements: rows open and rows beyond both bounds
        assert (rest < pol['log_std_min']).any() and (rest > pol['log_std_max']).any() and w['open'][:, 2:].any()
        assert (w['lr'].v[:, 0] == pol['log_std_max']).all() and (w['lr'].v[:, 1] == pol['log_std_min']).all()
    # float64 autograd with the strict gate imposed is the oracle; torch.clamp's own gradient is the inclusive gate's
    gm, gs = _soft_actor_torch(c, strict_clamp=True)[:2]
    _f64_close(gm, w['mu'], 'mu')
    _f64_close(gs, w['sigma'], 'sigma, strict gate')
    opened = so.actor_gradient(*ec.soft_actor_args(c), exempt=c['exempt'], wrong='edge_open')
    own_m, own_s = _soft_actor_torch(c, strict_clamp=False)[:2]
    _f64_close(own_m, w['mu'], 'mu: dm = du is not gated')
    _f64_close(own_s, opened['sigma'], 'sigma: torch.clamp passes the gradient at x == min and x == max')
    diff = np.abs(own_s - w['sigma']['flat'])
    print('C %s: torch.clamp differs from the device convention by up to %.3g on db3[0:2] (largest element of the gradient %.3g)' % (
        activation, diff[named[-2:]].max(), np.abs(w['sigma']['flat']).max()))
    assert (own_s[named[-2:]] != 0).all() and (diff[named] > 0).any()
    # the target's forward values do not notice the edge
    wt = c['want_target']
    assert not wt['edge'].any() and not wt['kink'].any() and not wt['tie'].any()
    # an inclusive gate is outside the float32 bound on the slices that are exactly 0
    c32 = ec.soft_case('C', None, 5, 42, activation, F32)
    w = c32['want_actor']
    bad = so.actor_gradient(*ec.soft_actor_args(c32), exempt=c32['exempt'], wrong='edge_open')['sigma']['flat']
    assert (bad[named[-2:]] != 0).all() and (bad[named[:64]] != 0).any() and (bad[named[64:128]] != 0).any()
    assert (np.abs(bad[named] - w['sigma']['flat'][named]) > w['sigma']['bound'][named])[-2:].all()


# -------------------------------------------------------------------------------------------------------------------- A
def _kinds(c):
    """[ROWS] the absorbing column's four values by row: 0.5, the next value above, -0.0, 1.0."""
    ab, v = c['absorbing'], ec.ABSORBING(c['dtype'])
    assert ab.dtype == c['dtype'] and v[0] == 0.5 and v[1] > 0.5 and float(v[1]) - 0.5 <= 2.0 ** -23 and np.signbit(v[2]) and v[2] == 0
    kinds = np.arange(ec.ROWS) % 4
    assert np.array_equal(ab, v[kinds]) and np.array_equal(np.signbit(ab), kinds == 2)
    return kinds


def test_absorbing_at_the_threshold_soft_target():
    for dt in (F32, F64):
        c = ec.soft_case('A', None, 5, 42, 'relu', dt)
        kinds = _kinds(c)
        assert not so.row_flags(c).any() and c['exempt'] == {}
        w = c['want_target']
        dropped = np.isin(kinds, (1, 3))
        assert (w['y'].v[dropped] == c['reward'][dropped].astype(F64)).all() and (w['y'].v[~dropped] != c['reward'][~dropped]).all()
    # torch, the flag read as the bool the reference stores
    x, eps = _t(c['obs']), _t(c['eps'])
    mu, sigma, tq = _net(c['policy']['mu']), _net(c['policy']['sigma']), [_net(cr) for cr in c['targets']]
    with torch.no_grad():
        a, logp, _ = _soft_sample(c, mu, sigma, x, eps, False)
        qmin = torch.minimum(_critic(tq[0], x, a), _critic(tq[1], x, a))
        keep = (~(_t(c['absorbing']) > 0.5)).double()
        y = _t(c['reward']) + c['gamma'] * keep * (qmin - np.exp(c['log_alpha']) * logp)
    _close(y.numpy(), w['y'].v, w['y'].s, 'y')
    c32 = ec.soft_case('A', None, 5, 42, 'relu', F32)
    w = c32['want_target']
    bad = so.target(*ec.soft_target_args(c32), wrong='absorbing_ge')['y'].v
    out = np.abs(bad - w['y'].v) > w['y'].e
    assert np.array_equal(out, _kinds(c32) == 0)


def test_absorbing_at_the_threshold_td3_target():
    import offpolicy_oracle as oo
    for dt in (F32, F64):
        c, ref = ec.offpolicy_case(dt)
        kinds = _kinds(c)
        dropped = np.isin(kinds, (1, 3))
        assert (ref['y'][dropped] == c['reward'][dropped].astype(F64)).all() and (ref['y'][~dropped] != c['reward'][~dropped]).all()
        bad = oo.target(c['actor'], c['critics'], c['next_obs'], c['reward'], c['absorbing'], c['gamma'], c['eps'], c['noise_std'],
                        c['noise_clip'], c['low'], c['high'], c['mean_mode'], dt, wrong='absorbing_ge')['y']
        y2 = oo.target_from_action(c['critics'], c['next_obs'], ref['a'], c['reward'], c['absorbing'], c['gamma'], dt)
        bad2 = oo.target_from_action(c['critics'], c['next_obs'], ref['a'], c['reward'], c['absorbing'], c['gamma'], dt, wrong='absorbing_ge')
        if dt == F32:
            out = np.abs(bad - ref['y']) > ref['e_y']                      # the end-to-end bound carries the actor's error: wide
            assert out[kinds == 0].any() and not out[kinds != 0].any()
            assert np.array_equal(np.abs(bad2[0] - y2[0]) > y2[1], kinds == 0)
    # torch: examples/td3_air_hockey.py's modules (which hold float32-representable weights), the flag read as a bool
    from test_offgrad_oracle import Actor, Critic, _t as t64
    dt = F32
    c, ref = ec.offpolicy_case(dt)
    with torch.no_grad():
        x = t64(c['next_obs'], torch.float64)
        a = Actor(c['actor'], c['mean_mode'], torch.float64)(x)
        n = torch.clamp(float(dt(c['noise_std'])) * t64(c['eps'], torch.float64), -float(dt(c['noise_clip'])), float(dt(c['noise_clip'])))
        a = torch.minimum(torch.maximum(a + n, t64(c['low'], torch.float64)), t64(c['high'], torch.float64))
        q = torch.minimum(*(Critic(cr, torch.float64)(x, a) for cr in c['critics']))
        keep = (~(t64(c['absorbing'], torch.float64) > 0.5)).double()
        y = t64(c['reward'], torch.float64) + float(dt(c['gamma'])) * keep * q
    assert (np.abs(y.numpy() - ref['y']) <= 1e-12 * ref['scale_y'] + 1e-14).all()
