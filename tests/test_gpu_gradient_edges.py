"""GPU tests of the gradient kernels' conventions EXACTLY at the points where a gradient is discontinuous, on the cases of
tests/edge_cases.py: a ReLU pre-activation of exactly 0 (act' = 0: `h > 0`), the two critics equal bit for bit (critic 1), a log
sigma exactly on a clamp bound (the gate is strict on both sides), an absorbing flag of exactly 0.5 (kept: `> 0.5`).  The
compared quantities are exact values in every arithmetic and order of summation, so the device and the float64 oracles take the
same decision by construction; tests/test_edge_cases_oracle.py checks the premises on the CPU and shows that a device with any of
the four mistakes would fail here.

Every call is 65 rows, once with the default grid and once with n_blocks = 2; per-row outputs are bit-equal between the two.
Exact claims are compared with 0 (by value: -0 passes) or with the stated vector; everything else is held to the oracles'
float32 bounds and to 1e-12 scale + 1e-14 in float64, as tests/test_gpu_{soft,offgrad,fit,trust,offpolicy}.py do, with the
engineered units, rows and elements -- and nothing else -- exempt from the oracles' kink, tie and edge flags."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_cases as ec                                       # noqa: E402
import fit_oracle as fo                                       # noqa: E402
import offgrad_oracle as og                                   # noqa: E402
import offpolicy_oracle as oo                                 # noqa: E402
import soft_oracle as so                                      # noqa: E402
import trust_oracle as to                                     # noqa: E402

DEV = 'cuda:0'
DT = {'f32': torch.float32, 'f64': torch.float64}
NP = {'f32': np.float32, 'f64': np.float64}
GRIDS = (0, 2)
KINKS = [(n,) + p for n in ('K1', 'K2') for p in ec.PAIRS]
KINK_IDS = ['%s-%d-%d' % k for k in KINKS]
_cache = {}


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _nan(dt, *shape):
    return torch.full(shape, float('nan'), dtype=DT[dt], device=DEV)


def _inside(dt, got, want, what, key='flat', bound='bound', scale='scale'):
    got = _np(got)
    assert np.isfinite(got).all(), what
    ok, worst = og.inside(got, want, NP[dt], key, bound, scale)
    print('%s %s %s: worst |error| / allowance %.4f' % (what, key, dt, worst))
    assert ok, (what, key, dt, 'worst |error| / allowance %.3f' % worst)


def _inside_v(dt, got, want, what):
    got = _np(got)
    assert np.isfinite(got).all(), what
    ok, worst = so.inside_v(got, want, NP[dt])
    print('%s %s: worst |error| / allowance %.4f' % (what, dt, worst))
    assert ok, (what, dt, 'worst |error| / allowance %.3f' % worst)


def _zero(t, where, what):
    """Exactly 0 by value on the named positions (so that -0 passes), and not everywhere else."""
    v = t.detach().cpu().numpy().reshape(-1)
    assert (v[where] == 0).all(), (what, v[where][v[where] != 0][:8])
    rest = np.ones(v.size, bool)
    rest[where] = False
    assert (v[rest] != 0).any(), what


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ----------------------------------------------------------------------------------------------------------------- soft
def _soft(dt, *spec):
    def make():
        from test_gpu_soft import _objects
        c = ec.soft_case(*spec, dtype=NP[dt])
        return (c,) + _objects(c)
    return _once(('soft', dt) + spec, make)


def _soft_kw(c):
    return dict(act_scale=_t(c['act_scale']), act_shift=_t(c['act_shift']))


def _soft_target(dt, c, pol, tgs, la, n_blocks, what):
    """tests/test_gpu_soft.py's _check_target with the case's description handed to the oracle -> (y, action_out, logp_out)."""
    from rl_on_manifold_amd import soft_td_target
    M, k = c['eps'].shape
    aout, lp = _nan(dt, M, k), _nan(dt, M)
    y = soft_td_target(pol, tgs, _t(c['obs']), _t(c['reward']), _t(c['absorbing']), c['gamma'], la, _t(c['eps']), action_out=aout,
                       logp_out=lp, n_blocks=n_blocks, **_soft_kw(c))
    want = c['want_target']
    what = what + ('target', n_blocks)
    _inside_v(dt, aout, want['a'], what + ('a',))
    _inside_v(dt, lp, want['logp'], what + ('logp',))
    at = so.target(*ec.soft_target_args(c), action=_np(aout), logp=_np(lp), exempt=c['exempt'])
    assert not at['kink'].any() and not at['tie'].any() and not at['edge'].any()
    _inside_v(dt, y, at['y'], what + ('y at the device action and logp',))
    if dt == 'f64' or want['kinks_e2e'] == 0:
        _inside_v(dt, y, want['y'], what + ('y end to end',))
    return y, aout, lp


def _soft_critics(dt, c, crs, n_blocks, what):
    from rl_on_manifold_amd import soft_critic_gradient
    gs = soft_critic_gradient(crs, _t(c['obs']), _t(c['action']), _t(c['target']), n_blocks=n_blocks)
    for j, (g, want) in enumerate(zip(gs, c['want_critic'])):
        _inside(dt, g.flat, want, what + ('critic', j, n_blocks))
        _inside(dt, g.stats, want, what + ('critic', j, n_blocks), 'stats', 'stats_bound', 'stats_scale')
    return gs


def _soft_actor(dt, c, pol, crs, la, n_blocks, what):
    """tests/test_gpu_soft.py's _check_actor with the case's description handed to the oracle: the chain cut at the device's
    intermediates, and end to end in float64 -> (ActorGradients, the per-row outputs)."""
    from rl_on_manifold_amd import soft_actor_gradient
    M, k = c['eps'].shape
    o = dict(action_out=_nan(dt, M, k), logp_out=_nan(dt, M), q_out=_nan(dt, M, 2), dqda_out=_nan(dt, M, k))
    g = soft_actor_gradient(pol, crs, _t(c['obs']), _t(c['eps']), la, c['target_entropy'], n_blocks=n_blocks, **o, **_soft_kw(c))
    want, ex = c['want_actor'], c['exempt']
    what = what + ('actor', n_blocks)
    _inside_v(dt, o['action_out'], want['a'], what + ('a',))
    _inside_v(dt, o['logp_out'], want['logp'], what + ('logp',))
    args = ec.soft_actor_args(c)
    a_np, q_np, dq_np = _np(o['action_out']), _np(o['q_out']), _np(o['dqda_out'])
    at = so.actor_gradient(*args, action=a_np, q=q_np, exempt=ex)
    assert not at['kink'].any() and not at['tie'].any() and not at['edge'].any()              # zero rows exempt beyond the engineered
    for j in range(2):
        _inside_v(dt, o['q_out'][:, j], at['q'][j], what + ('q_%d at the device action' % (j + 1),))
    _inside_v(dt, o['dqda_out'], at['dqda'], what + ('dq/da at the device action',))
    frm = so.actor_gradient(*args, action=a_np, q=q_np, dq=dq_np, exempt=ex)
    for part in ('mu', 'sigma'):
        _inside(dt, getattr(g, part).flat, frm[part], what + (part, 'from the device dq/da'))
    _inside(dt, g.stats, at, what + ('at the device action',), 'stats', 'stats_bound', 'stats_scale')
    if dt == 'f64' or want['kinks_e2e'] == 0:
        for part in ('mu', 'sigma'):
            _inside(dt, getattr(g, part).flat, want[part], what + (part, 'end to end'))
        _inside(dt, g.stats, want, what + ('end to end',), 'stats', 'stats_bound', 'stats_scale')
    assert float(g.stats[3]) == float(NP[dt](int(want['clamped'].sum())) / NP[dt](M))
    return g, o


def _same_rows(a, b):
    assert all(torch.equal(x, y) for x, y in zip(a, b)), 'a per-row output depends on the grid'


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('which', ['policy', 'critics'])
@pytest.mark.parametrize('name,j1,j2', KINKS, ids=KINK_IDS)
def test_soft_gradients_at_a_relu_kink(dt, name, j1, j2, which):
    """K1 and K2 in the mu and sigma networks (their own gradients) or in both critics (the critics' gradients, and dqda_out
    inside its bound).  K1: dW1[j1, :], db1[j1], dW2[j2, :], db2[j2] of every engineered network are exactly 0."""
    c, pol, crs, tgs, la = _soft(dt, name, which, j1, j2, 'relu')
    D, k = ec.SOFT_SHAPE
    what = ('soft', name, which, j1, j2)
    rows = []
    for nb in GRIDS:
        g, o = _soft_actor(dt, c, pol, crs, la, nb, what)
        rows.append(tuple(o.values()))
        if which == 'critics':
            gs = _soft_critics(dt, c, crs, nb, what)
        if name == 'K1':
            for t, n_in in ([(g.mu.flat, D), (g.sigma.flat, D)] if which == 'policy' else [(x.flat, D + k) for x in gs]):
                _zero(t, ec.unit_slices(n_in, j1, j2), what + (nb,))
    _same_rows(*rows)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('j1,j2', ec.PAIRS)
def test_soft_dqda_with_a_critic_unit_dead_through_a_zero_action_element(dt, j1, j2):
    """K1 in the critics with W1[j1, D + 0] kept and the action's element 0 exactly 0 on every row: the unit's contribution to
    dq/da_0 is gated off (edge_cases.soft_case says why only this column can keep its weight)."""
    c, pol, crs, tgs, la = _soft(dt, 'K1', 'critics_a0', j1, j2, 'relu')
    what = ('soft', 'K1', 'critics_a0', j1, j2)
    rows = []
    for nb in GRIDS:
        g, o = _soft_actor(dt, c, pol, crs, la, nb, what)
        assert o['action_out'][:, 0].eq(0).all() and o['action_out'][:, 1:].ne(0).all()          # the premise, from the device
        rows.append(tuple(o.values()))
    _same_rows(*rows)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_soft_actor_selects_critic_one_at_a_tie(dt):
    """T: on the tie rows q_1 == q_2 bit for bit with dq/da = (1, 0, ...) for critic 1 and (0, 1, 0, ...) for critic 2."""
    c, pol, crs, tgs, la = _soft(dt, 'T', None, 5, 42, 'relu')
    k = ec.SOFT_SHAPE[1]
    tie = torch.zeros(ec.ROWS, dtype=torch.bool, device=DEV)
    tie[list(ec.TIE_ROWS)] = True
    e0, e1 = (torch.eye(k, dtype=DT[dt], device=DEV)[j] for j in (0, 1))
    rows = []
    for nb in GRIDS:
        g, o = _soft_actor(dt, c, pol, crs, la, nb, ('soft', 'T'))
        a, q, dq = o['action_out'], o['q_out'], o['dqda_out']
        # the premise, from the device's own outputs
        assert torch.equal(a[tie, 0], a[tie, 1]) and torch.equal(q[tie, 0], q[tie, 1])
        assert torch.equal(q[:, 0] == q[:, 1], tie)
        first, second = q[:, 0] < q[:, 1], q[:, 1] < q[:, 0]
        print('T %s n_blocks %d: %d tie rows, %d rows with q_1 < q_2, %d rows with q_2 < q_1' % (dt, nb, int(tie.sum()), int(first.sum()), int(second.sum())))
        assert int(tie.sum()) == len(ec.TIE_ROWS) and first.any() and second.any()
        assert (dq[tie | first] == e0).all(), 'critic 1 at a tie and where q_1 < q_2'
        assert (dq[second] == e1).all(), 'critic 2 where q_2 < q_1'
        rows.append(tuple(o.values()))
    _same_rows(*rows)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('activation', ['relu', 'tanh'])
def test_soft_clamp_gate_is_strict_on_both_bounds(dt, activation):
    """C: log sigma 0 sits exactly on log_std_max and log sigma 1 exactly on log_std_min, on every row: dl = 0 there, so the
    sigma network's dW3[0:2, :] and db3[0:2] are exactly 0 and every row counts as clamped; the forward values of both calls do
    not notice the edge, and the mu network's gradient, which is not gated, stays inside its bound."""
    c, pol, crs, tgs, la = _soft(dt, 'C', None, 5, 42, activation)
    D, k = ec.SOFT_SHAPE
    o_W3 = 64 * D + 64 + 4096 + 64
    named = np.concatenate([np.arange(o_W3, o_W3 + 128), o_W3 + 64 * k + np.arange(2)])
    rows, ys = [], []
    for nb in GRIDS:
        g, o = _soft_actor(dt, c, pol, crs, la, nb, ('soft', 'C', activation))
        _zero(g.sigma.flat, named, ('soft', 'C', activation, nb))
        assert float(g.stats[3]) == 1.0
        rows.append(tuple(o.values()))
        ys.append(_soft_target(dt, c, pol, tgs, la, nb, ('soft', 'C', activation)))
    _same_rows(*rows)
    _same_rows(*ys)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_soft_target_reads_the_absorbing_flag_above_one_half(dt):
    """A: 0.5 is kept, the next value above 0.5 is dropped, -0.0 is kept, 1.0 is dropped."""
    c, pol, crs, tgs, la = _soft(dt, 'A', None, 5, 42, 'relu')
    ys = [_soft_target(dt, c, pol, tgs, la, nb, ('soft', 'A')) for nb in GRIDS]
    _same_rows(*ys)
    dropped = _t(np.isin(np.arange(ec.ROWS) % 4, (1, 3)))
    y, r = ys[0][0], _t(c['reward'])
    assert torch.equal(y[dropped], r[dropped]) and (y[~dropped] != r[~dropped]).all()


# ------------------------------------------------------------------------------------------------------------ offpolicy
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_td3_target_reads_the_absorbing_flag_above_one_half(dt):
    from rl_on_manifold_amd import td_target
    from test_gpu_offpolicy import _inside as inside, _objects

    def make():
        c, ref = ec.offpolicy_case(NP[dt])
        return (c, ref) + _objects(c)
    c, ref, pol, crs = _once(('offpolicy', dt), make)
    outs = []
    for nb in GRIDS:
        aout = _nan(dt, ec.ROWS, c['action'].shape[1])
        y = td_target(pol, crs, _t(c['next_obs']), _t(c['reward']), _t(c['absorbing']), c['gamma'], eps=_t(c['eps']), noise_std=c['noise_std'],
                      noise_clip=c['noise_clip'], low=_t(c['low']), high=_t(c['high']), n_blocks=nb, action_out=aout)
        inside(dt, y, ref['y'], ref['e_y'], ref['scale_y'], ('td3', 'A', nb, 'y'))
        y2, e2 = oo.target_from_action(c['critics'], c['next_obs'], aout.cpu().numpy(), c['reward'], c['absorbing'], c['gamma'], NP[dt])
        inside(dt, y, y2, e2, ref['scale_y'], ('td3', 'A', nb, 'y from the device action'))
        outs.append((y, aout))
    _same_rows(*outs)
    dropped = _t(np.isin(np.arange(ec.ROWS) % 4, (1, 3)))
    y, r = outs[0][0], _t(c['reward'])
    assert torch.equal(y[dropped], r[dropped]) and (y[~dropped] != r[~dropped]).all()


# -------------------------------------------------------------------------------------------------------------- offgrad
def _offgrad(dt, *spec):
    def make():
        from test_gpu_offgrad import _objects
        c = ec.offgrad_case(*spec, dtype=NP[dt])
        return (c,) + _objects(c)
    return _once(('offgrad', dt) + spec, make)


def _offgrad_actor(dt, c, pol, cr, n_blocks, what):
    """tests/test_gpu_offgrad.py's _check_actor with the case's description handed to the oracle."""
    from rl_on_manifold_amd import actor_gradient
    M, k, ex = ec.ROWS, c['k'], c['exempt']
    aout, dq = _nan(dt, M, k), _nan(dt, M, k)
    g = actor_gradient(pol, cr, _t(c['obs']), action_out=aout, dqda_out=dq, n_blocks=n_blocks)
    want = c['want_actor']
    what = what + ('actor', n_blocks)
    _inside(dt, aout, want, what, 'a', 'e_a', 'scale_a')
    at = og.actor_gradient(c['actor'], c['critics'][0], c['obs'], 1, action=_np(aout), exempt=ex)
    assert at['kinks'] == 0
    _inside(dt, dq, at, what + ('at the device action',), 'dqda', 'e_dqda', 'scale_dqda')
    _inside(dt, g.stats, at, what + ('at the device action',), 'stats', 'stats_bound', 'stats_scale')
    frm = og.actor_gradient(c['actor'], c['critics'][0], c['obs'], 1, dqda=_np(dq), exempt=ex)
    assert frm['kinks'] == 0
    _inside(dt, g.flat, frm, what + ('from the device dq/da',))
    if dt == 'f64' or want['kinks'] == 0:
        _inside(dt, g.flat, want, what + ('end to end',))
        _inside(dt, dq, want, what + ('end to end',), 'dqda', 'e_dqda', 'scale_dqda')
    return g, aout, dq


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('kind', [og.DDPG, og.TD3])
@pytest.mark.parametrize('name,j1,j2', KINKS, ids=KINK_IDS)
def test_offgrad_with_the_critics_at_a_relu_kink(dt, name, j1, j2, kind):
    """The critics' gradients, dW2a included, and the actor's gradient through the engineered first critic."""
    from rl_on_manifold_amd import critic_gradient
    c, pol, crs = _offgrad(dt, name, 'critics', j1, j2, kind)
    n1 = c['critics'][0]['W1'].shape[1]
    what = ('offgrad', name, 'critics', j1, j2, kind)
    rows = []
    for nb in GRIDS:
        gs = critic_gradient(crs, _t(c['obs']), _t(c['action']), _t(c['target']), n_blocks=nb)
        for j, (g, want) in enumerate(zip(gs, c['want_critic'])):
            _inside(dt, g.flat, want, what + ('critic', j, nb))
            _inside(dt, g.stats, want, what + ('critic', j, nb), 'stats', 'stats_bound', 'stats_scale')
            if name == 'K1':
                _zero(g.flat, ec.unit_slices(n1, j1, j2, c['k']), what + (j, nb))
        rows.append(_offgrad_actor(dt, c, pol, crs[0], nb, what)[1:])
    _same_rows(*rows)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('kind', [og.DDPG, og.TD3])
@pytest.mark.parametrize('name,j1,j2', KINKS, ids=KINK_IDS)
def test_offgrad_with_the_actor_at_a_relu_kink(dt, name, j1, j2, kind):
    c, pol, crs = _offgrad(dt, name, 'actor', j1, j2, kind)
    what = ('offgrad', name, 'actor', j1, j2, kind)
    rows = []
    for nb in GRIDS:
        g, aout, dq = _offgrad_actor(dt, c, pol, crs[0], nb, what)
        if name == 'K1':
            _zero(g.flat, ec.unit_slices(c['D'], j1, j2), what + (nb,))
        rows.append((aout, dq))
    _same_rows(*rows)


# ----------------------------------------------------------------------------------------------------------- fit, trust
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('head', [fo.VALUE, fo.PPO_CLIP], ids=['value', 'ppo'])
@pytest.mark.parametrize('name,j1,j2', KINKS, ids=KINK_IDS)
def test_fit_gradients_at_a_relu_kink(dt, name, j1, j2, head):
    from rl_on_manifold_amd import MlpPolicy, fit
    from test_gpu_fit import _inside as inside

    def make():
        c = ec.fit_case(name, j1, j2, head, NP[dt])
        net = c['net']
        pol = MlpPolicy(*(_t(net[k]) for k in fo.NAMES), std=_t(c['std']), obs_shift=_t(net['obs_shift']), obs_scale=_t(net['obs_scale']),
                        activation=net['activation'])
        return c, pol, {k: _t(c[k]) for k in ('x', 'action', 'weight', 'logp_old')}
    c, pol, t = _once(('fit', dt, name, j1, j2, head), make)
    for nb in GRIDS:
        if head == fo.VALUE:
            g = fit.value_gradient(pol, t['x'], t['weight'], n_blocks=nb)
        else:
            g = fit.policy_gradient(pol, t['x'], t['action'], t['weight'], t['logp_old'], clip=c['clip'], n_blocks=nb)
        inside(dt, g, c['want'], ('fit', name, j1, j2, head, nb))
        if name == 'K1':
            _zero(g.flat, ec.unit_slices(fo.ROW_SHAPE[head][0], j1, j2), ('fit', name, j1, j2, head, nb))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('name,j1,j2', KINKS, ids=KINK_IDS)
def test_fisher_vector_product_at_a_relu_kink(dt, name, j1, j2):
    """K1 with damping = 0: the W1[j1, :], b1[j1], W2[j2, :], b2[j2] components of F v are exactly 0 for a direction that is not
    zero there (the tangent and the backward pass both read the gate).  K2 is held to trust_oracle.fvp."""
    from rl_on_manifold_amd import trust
    from test_gpu_trust import _policy

    def make():
        c = ec.trust_case(name, j1, j2, NP[dt])
        return c, _policy(c['net'], c['std']), _t(c['x']), _t(c['v'])
    c, pol, x, v = _once(('trust', dt, name, j1, j2), make)
    want = c['want']
    sl = ec.unit_slices(to.ROW_SHAPE[0], j1, j2)
    assert (c['v'][sl] != 0).all() and c['damping'] == (0.0 if name == 'K1' else to.DAMPING)
    for nb in GRIDS:
        got = trust.fisher_vector_product(pol, x, v, damping=c['damping'], n_blocks=nb)
        what = ('trust', name, j1, j2, nb)
        _inside(dt, got, want, what)
        if dt == 'f32':                                            # the norm rule of tests/test_gpu_trust.py
            err = _np(got) - want['flat']
            assert np.linalg.norm(err) <= 1e-2 * np.linalg.norm(want['flat']), what
        if name == 'K1':
            _zero(got, sl, what)
