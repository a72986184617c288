"""Float64 restatement of what libatacom_offgrad.so computes (include/atacom_offgrad_hip.h; test infrastructure only): the
gradient of a DDPG / TD3 critic's mean-squared TD error and the deterministic policy gradient of the actor, with the bound a
float32 evaluation is held to, per element, and the case builder the CPU and GPU tests share.  A helper module: it holds no test.

PINNED: tests/test_offgrad_oracle.py checks both gradients against torch's float64 autograd of the two loss expressions of
examples/td3_air_hockey.py to 1e-12 of scale, holds torch's own FLOAT32 autograd to the float32 bound on every element (the
actor's gradient through the chain cut at its own action and its own dq/da: `case` says why), and shows that three deliberately
wrong restatements fall outside it.

Built from what the two neighbouring oracles export.  The forward chains are those of offpolicy_oracle (`_normalise`, `_layer`,
`_hidden`: the critic's two-branch layer 2 as critic_q chains it, kept here per layer because a backward pass needs the
activations); the backward pass is first-order error propagation with every second-order term kept, from fit_oracle's
primitives `_act_prime` (act' from the activation's value), `_back` (a transposed product W^T delta times act') and `_wgrad`
(sum_r delta_r act_r^T with gamma(M + 3) for the roundings of each product, of the sum over the M rows IN ANY ORDER and of the
division by M).

SAFETY (= 2, for the matrix cores, which are not documented to round every partial sum to nearest) is placed as in
offpolicy_oracle: on the gamma of a product that runs on the matrix cores and on nothing else -- what a product inherits is
carried as it is.  fit_oracle's primitives take the inner dimension, not a factor, so they are handed the dimension n' with
gamma(n') = gamma(SAFETY n) >= SAFETY gamma(n) (gamma is convex): `_k` below.  The row arithmetic between the products (the
head, the squash and its derivative, the divisions by act_scale) runs on the vector unit, one rounding u per operation.

The bound means nothing within a forward error of a ReLU kink, so both gradients count the rows that have a pre-activation, of
the actor or of a critic, within its forward bound of 0 (`kinks`); `case` draws such rows again until there is none and
asserts it.  Float64 is held to 1e-12 scale + 1e-14, `scale` being the same backward pass on absolute values started from the
TERMS of dy (fit_oracle's convention).
"""
import functools

import numpy as np

from evaluate_oracle import SAFETY, TANH_ABS, U32, gamma
from fit_oracle import _act_prime, _back, _kink, _units, _wgrad
import offpolicy_oracle as oo
from offpolicy_oracle import DDPG, TD3, _f64, _hidden, _layer, _normalise

PARAMS = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'W2a')          # the order of a critic's gradient
ACTOR_PARAMS = PARAMS[:6]


def _k(n, offset):
    """The dimension to hand a fit_oracle primitive that applies gamma(dimension + offset), so that it applies
    gamma(SAFETY (n + offset)) >= SAFETY gamma(n + offset)."""
    return int(SAFETY * (n + offset)) - offset


def _of(exempt, key, j=None):
    """The engineered (layer, unit) pairs of one network from a case's description {'actor': pairs, 'critics': [pairs, pairs], ...}
    (tests/edge_cases.py); None where there is none."""
    v = None if exempt is None else exempt.get(key)
    return v if v is None or j is None else v[j]


def critic_forward(c, x, a, e_a=None, exempt=None):
    """critic_q's chain with everything a backward pass needs: x1, as, h1, h2, q (and e_*), mag_q, the pre-activations a1, a2.
    exempt: this critic's engineered (layer, unit) pairs, left out of `kink`."""
    act = c.get('activation', 'relu')
    a = _f64(a)
    s = _f64(c.get('act_scale'))
    s = np.ones(a.shape[1]) if s is None else s
    as_ = a / s
    e_as = (0.0 if e_a is None else e_a) / np.abs(s) + gamma(2) * np.abs(as_)
    xn, e_x = _normalise(c, x)
    if c['kind'] == TD3:
        x1, e_x1 = np.concatenate([xn, as_], 1), np.concatenate([e_x, e_as], 1)
    else:
        x1, e_x1 = xn, e_x
    a1, e_a1, _ = _layer(x1, e_x1, c['W1'], c['b1'])
    h1, e_h1 = _hidden(a1, e_a1, act)
    k = as_.shape[1]
    a2, e_a2, _ = _layer(np.concatenate([h1, as_], 1), np.concatenate([e_h1, e_as], 1),
                         np.concatenate([_f64(c['W2']), _f64(c['W2a'])], 1), c['b2'], n=64 + 4 * ((k + 3) // 4))
    h2, e_h2 = _hidden(a2, e_a2, act)
    q, e_q, mag = _layer(h2, e_h2, c['W3'], c['b3'])
    kink = np.zeros(x1.shape[0], bool)
    if act == 'relu':
        kink = _kink(a1, e_a1, exempt, 1) | _kink(a2, e_a2, exempt, 2)
    return dict(x1=x1, e_x1=e_x1, as_=as_, e_as=e_as, s=s, a1=a1, e_a1=e_a1, h1=h1, e_h1=e_h1, a2=a2, e_a2=e_a2, h2=h2, e_h2=e_h2,
                q=q[:, 0], e_q=e_q[:, 0], mag_q=mag[:, 0], kink=kink, act=act)


def actor_forward(net, x, exempt=None):
    """offpolicy_oracle.mlp's chain, per layer.  exempt: this network's engineered (layer, unit) pairs, left out of `kink`."""
    act = net.get('activation', 'relu')
    xn, e_x = _normalise(net, x)
    a1, e_a1, _ = _layer(xn, e_x, net['W1'], net['b1'])
    h1, e_h1 = _hidden(a1, e_a1, act)
    a2, e_a2, _ = _layer(h1, e_h1, net['W2'], net['b2'])
    h2, e_h2 = _hidden(a2, e_a2, act)
    m, e_m, mag = _layer(h2, e_h2, net['W3'], net['b3'])
    kink = np.zeros(xn.shape[0], bool)
    if act == 'relu':
        kink = _kink(a1, e_a1, exempt, 1) | _kink(a2, e_a2, exempt, 2)
    return dict(xn=xn, e_xn=e_x, h1=h1, e_h1=e_h1, h2=h2, e_h2=e_h2, m=m, e_m=e_m, mag_m=mag, kink=kink, act=act)


def _pack(parts, order, M, stats):
    """{name: (value, bound, scale)} unscaled by 1 / M -> the result dict of either gradient."""
    parts = {k: (v / M, e / M, sc / M) for k, (v, e, sc) in parts.items()}
    st, e_st, a_st = stats
    flat = lambda i: np.concatenate([parts[k][i].reshape(-1) for k in order])             # noqa: E731
    zeros = np.zeros(3)
    return dict(flat=flat(0), bound=flat(1), scale=flat(2), parts=parts, order=list(order),
                stats=np.append(st.sum() / M, zeros), stats_scale=np.append(a_st.sum() / M, zeros),
                stats_bound=np.append((e_st.sum() + gamma(M + 3) * (a_st + e_st).sum()) / M, zeros))


def _network_backward(W2, W3, dy, e_dy, S_dy, h1, e_h1, h2, e_h2, act, opn=None):
    """delta2, delta1 of a network from dy [M, n_out]: each (value, bound, |.| pass, scale pass).  opn: the (layer, unit) pairs
    whose gate reads h >= 0 (wrong='kink_open')."""
    ap2, e_ap2 = _act_prime(h2, e_h2, act, _units(opn, 2))
    ap1, e_ap1 = _act_prime(h1, e_h1, act, _units(opn, 1))
    d2, e_d2 = _back(W3, dy, e_dy, ap2, e_ap2, _k(8, 1))
    A_d2 = (np.abs(dy) @ np.abs(W3)) * np.abs(ap2)
    S_d2 = (S_dy @ np.abs(W3)) * np.abs(ap2)
    d1, e_d1 = _back(W2, d2, e_d2, ap1, e_ap1, _k(64, 1))
    A_d1 = (A_d2 @ np.abs(W2)) * np.abs(ap1)
    S_d1 = (S_d2 @ np.abs(W2)) * np.abs(ap1)
    return (d2, e_d2, A_d2, S_d2), (d1, e_d1, A_d1, S_d1)


def critic_gradient(c, x, a, target, idx=None, wrong=None, exempt=None):
    """atacom_offgrad_critic_gradient for one critic on rows x [R, D], a [R, k] (gathered through idx, if given) and target [M]
    (row r of the call) -> dict: flat, bound, scale [64 n1 + 64 + 4096 + 64 + 64 + 1 + 64 k] in the order of PARAMS; stats,
    stats_bound, stats_scale [4]; kinks; parts.  wrong='no_as_cols': the as columns of a TD3 critic's dW1 zeroed.
    exempt: this critic's engineered (layer, unit) pairs, left out of `kinks`; wrong='kink_open': their gate reads h >= 0."""
    x, a, t = _f64(x), _f64(a), _f64(target)
    if idx is not None:
        x, a = x[np.asarray(idx)], a[np.asarray(idx)]
    M = x.shape[0]
    f = critic_forward(c, x, a, exempt=exempt)
    act = f['act']
    W2, W3 = _f64(c['W2']), _f64(c['W3'])
    d = f['q'] - t
    e_d = f['e_q'] + U32 * np.abs(d)
    dy, e_dy = 2.0 * d[:, None], 2.0 * e_d[:, None]
    S_dy = 2.0 * (f['mag_q'] + np.abs(t))[:, None]
    stats = (d * d, (2.0 * np.abs(d) + e_d) * e_d + gamma(2) * d * d, d * d)
    D2, D1 = _network_backward(W2, W3, dy, e_dy, S_dy, f['h1'], f['e_h1'], f['h2'], f['e_h2'], act,
                               exempt if wrong == 'kink_open' else None)
    DY = (dy, e_dy, np.abs(dy), S_dy)
    one, zero = np.ones((M, 1)), np.zeros((M, 1))
    Mk = _k(M, 3)
    parts = {}
    for name, bias, dd, (h, e_h) in (('W1', 'b1', D1, (f['x1'], f['e_x1'])), ('W2', 'b2', D2, (f['h1'], f['e_h1'])),
                                     ('W3', 'b3', DY, (f['h2'], f['e_h2']))):
        parts[name] = _wgrad(*dd, h, e_h, Mk)
        parts[bias] = tuple(v[:, 0] for v in _wgrad(*dd, one, zero, Mk))
    parts['W2a'] = _wgrad(*D2, f['as_'], f['e_as'], Mk)
    if wrong == 'no_as_cols' and c['kind'] == TD3:
        D = x.shape[1]
        v = parts['W1'][0].copy()
        v[:, D:] = 0.0
        parts['W1'] = (v,) + parts['W1'][1:]
    out = _pack(parts, PARAMS, M, stats)
    out['kinks'] = int(f['kink'].sum())
    return out


def actor_gradient(actor, c, x, mean_mode=1, idx=None, action=None, dqda=None, wrong=None, exempt=None):
    """atacom_offgrad_actor_gradient on rows x [R, D] (gathered through idx, if given) -> dict: flat, bound, scale in the order of
    ACTOR_PARAMS; stats ...; kinks; parts; a, e_a (the action), dqda, e_dqda, scale_dqda [M, k].
    action: the action taken as exact (a device's action_out) instead of the actor's own -- what dqda is then held to;
    dqda: dq/da taken as exact (a device's dqda_out) -- what the actor's gradient is then held to: the critic's part of the
    chain is cut off, and with it its norms.
    wrong='no_w2a': the W2a branch dropped from dq/da; 'no_scale': the division by the critic's act_scale omitted.
    exempt: {'actor': pairs, 'critics': [pairs, ...]}, the engineered (layer, unit) pairs of the actor and of the critics (this
    call reads the first's), left out of `kinks`; wrong='kink_open': their gate reads h >= 0."""
    ex_a, ex_c = _of(exempt, 'actor'), _of(exempt, 'critics', 0)
    opn_a, opn_c = (ex_a, ex_c) if wrong == 'kink_open' else (None, None)
    x = _f64(x)
    if idx is not None:
        x = x[np.asarray(idx)]
    M = x.shape[0]
    fa = actor_forward(actor, x, ex_a)
    act = fa['act']
    k = fa['m'].shape[1]
    if mean_mode:
        sp = _f64(actor.get('act_scale'))
        sp = np.ones(k) if sp is None else sp
        t, e_t = np.tanh(fa['m']), fa['e_m'] + TANH_ABS
        a, e_a = sp * t, np.abs(sp) * e_t + U32 * np.abs(sp * t)
        v, e_v = _act_prime(t, e_t, 'tanh')
        gm, e_gm = sp * v, np.abs(sp) * e_v + U32 * np.abs(sp * v)
    else:
        a, e_a = fa['m'], fa['e_m']
        gm, e_gm = np.ones_like(a), np.zeros_like(a)
    if action is not None:
        a, e_a = _f64(action), None
    kink = fa['kink'].copy()
    if dqda is None:
        fc = critic_forward(c, x, a, e_a, ex_c)
        kink |= fc['kink']
        cact = fc['act']
        W1, W2, W2a, W3 = (_f64(c[n]) for n in ('W1', 'W2', 'W2a', 'W3'))
        ap2, e_ap2 = _act_prime(fc['h2'], fc['e_h2'], cact, _units(opn_c, 2))
        one, zero = np.ones((M, 1)), np.zeros((M, 1))
        d2, e_d2 = _back(W3, one, zero, ap2, e_ap2, 0)                  # delta2 = W3^T * act'(h2): a product on the vector unit
        A_d2 = np.abs(W3) * np.abs(ap2)
        Wb, dd, e_dd, A_dd = W2a, d2, e_d2, A_d2                        # dq/das = [delta2 | delta1] [W2a ; W1[:, D:]]
        if wrong == 'no_w2a':
            Wb = np.zeros_like(W2a)
        if c['kind'] == TD3:
            ap1, e_ap1 = _act_prime(fc['h1'], fc['e_h1'], cact, _units(opn_c, 1))
            d1, e_d1 = _back(W2, d2, e_d2, ap1, e_ap1, _k(64, 1))
            A_d1 = (A_d2 @ np.abs(W2)) * np.abs(ap1)
            D = x.shape[1]
            Wb, dd, e_dd, A_dd = (np.concatenate([Wb, W1[:, D:]], 0), np.concatenate([d2, d1], 1), np.concatenate([e_d2, e_d1], 1),
                                  np.concatenate([A_d2, A_d1], 1))
        ones_k = np.ones((M, k))
        gs, e_gs = _back(Wb, dd, e_dd, ones_k, np.zeros((M, k)), _k(Wb.shape[0], 1))
        sq = fc['s'] if wrong != 'no_scale' else np.ones(k)
        dq = gs / sq
        e_dq = e_gs / np.abs(sq) + U32 * np.abs(dq)
        S_dq = (A_dd @ np.abs(Wb)) / np.abs(sq)
        stats = (-fc['q'], fc['e_q'], fc['mag_q'])
    else:
        dq, e_dq = _f64(dqda), np.zeros((M, k))
        S_dq = np.abs(dq)
        stats = (np.zeros(M), np.zeros(M), np.zeros(M))
    dm = -(dq * gm)
    e_dm = np.abs(gm) * e_dq + np.abs(dq) * e_gm + e_dq * e_gm + U32 * np.abs(dm)
    S_dm = S_dq * np.abs(gm)
    W2p, W3p = _f64(actor['W2']), _f64(actor['W3'])
    D2, D1 = _network_backward(W2p, W3p, dm, e_dm, S_dm, fa['h1'], fa['e_h1'], fa['h2'], fa['e_h2'], act, opn_a)
    DY = (dm, e_dm, np.abs(dm), S_dm)
    one, zero = np.ones((M, 1)), np.zeros((M, 1))
    Mk = _k(M, 3)
    parts = {}
    for name, bias, dd_, (h, e_h) in (('W1', 'b1', D1, (fa['xn'], fa['e_xn'])), ('W2', 'b2', D2, (fa['h1'], fa['e_h1'])),
                                      ('W3', 'b3', DY, (fa['h2'], fa['e_h2']))):
        parts[name] = _wgrad(*dd_, h, e_h, Mk)
        parts[bias] = tuple(v[:, 0] for v in _wgrad(*dd_, one, zero, Mk))
    out = _pack(parts, ACTOR_PARAMS, M, stats)
    out.update(kinks=int(kink.sum()), a=a, e_a=e_a, dqda=dq, e_dqda=e_dq, scale_dqda=S_dq + 0.0,
               scale_a=(np.abs(sp) * (fa['mag_m'] + 1.0) if mean_mode else fa['mag_m']))
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
SHAPE_CASES, SHAPE_SEEDS, SHAPE_KEYS = oo.SHAPE_CASES, oo.SHAPE_SEEDS, oo.SHAPE_KEYS
ROW_CASES, ROW_SHAPE = oo.ROW_CASES, oo.ROW_SHAPE
MEAN_MODES = (1, 0)
REDRAWS = 200


def row_kinks(c, exempt=None):
    """Per row of the case's data: a ReLU pre-activation within its forward bound of 0 in a critic at the recorded action, in
    the actor, or in the first critic at the actor's action taken as exact -- there within TWICE the bound, so that the action
    a device forms, which lies within a small fraction of that bound of the actor's, finds the rows clear as well.
    exempt: {'actor': pairs, 'critics': [pairs, pairs]}, the engineered units left out; every other unit counts as ever."""
    x = c['obs']
    fa = actor_forward(c['actor'], x, _of(exempt, 'actor'))
    bad = fa['kink'].copy()
    for j, cr in enumerate(c['critics']):
        bad |= critic_forward(cr, x, c['action'], exempt=_of(exempt, 'critics', j))['kink']
    if c['mean_mode']:
        sp = _f64(c['actor'].get('act_scale'))
        act = (np.ones(fa['m'].shape[1]) if sp is None else sp) * np.tanh(fa['m'])
    else:
        act = fa['m']
    f = critic_forward(c['critics'][0], x, act)
    if f['act'] == 'relu':
        ex = _of(exempt, 'critics', 0)
        bad |= _kink(f['a1'], f['e_a1'], ex, 1, 2.0) | _kink(f['a2'], f['e_a2'], ex, 2, 2.0)
    return bad


@functools.lru_cache(maxsize=None)
def case(seed, kind, D, k, activation, normalise, act_scale, rows, mean_mode=1, dtype=np.float32, n_idx=0):
    """A case in `dtype` on offpolicy_oracle.case's data: actor, the critic pair, obs, the recorded action, and a target at
    Q_1 + N(0, 1) per row of the call.  With n_idx > 0 the call names n_idx rows through `idx`, unsorted and with repeats.

    No row sits at a ReLU kink (row_kinks), and that is asserted.  fit_oracle.case moves its seed on until the count is zero; with
    four networks per case and up to 600 rows a whole batch without one is too rare for that (about 16 rows in 600 sit at one), so
    here the ROWS that sit at one are drawn again, deterministically, from the distributions of offpolicy_oracle.case.
    -> dict with `want_critic` (one per critic) and `want_actor`; want_actor['kinks'] counts the rows that the END-TO-END bound
    of the actor's gradient does not cover (the critic's pre-activations within the bound that the actor's whole worst-case
    error gives them): zero for tanh networks, most rows for ReLU, which is why a float32 evaluation is held to the chain cut
    at its own action and its own dq/da (actor_gradient's `action=`, `dqda=`), where the bounds are sharp and no row sits at a
    kink.  Cached: the tests share one reference and leave it unchanged."""
    b = oo.case(seed, kind, D, k, activation, normalise, act_scale, rows, n_critics=2, mean_mode=mean_mode, dtype=dtype)
    rng = np.random.default_rng(seed + 77)
    c = dict(actor=b['actor'], critics=b['critics'], obs=b['next_obs'].copy(), action=b['action'].copy(), mean_mode=mean_mode,
             dtype=dtype, kind=kind, D=D, k=k, activation=activation)
    s = b['actor']['act_scale'] if mean_mode else np.ones(k, dtype)
    for _ in range(REDRAWS):
        bad = row_kinks(c)
        if not bad.any():
            break
        n = int(bad.sum())
        c['obs'][bad] = rng.normal(0.0, 1.0, (n, D)).astype(dtype)
        c['action'][bad] = (rng.uniform(-1.0, 1.0, (n, k)) * s).astype(dtype)
    assert not row_kinks(c).any(), 'rows at a kink after %d redraws' % REDRAWS
    idx = None
    if n_idx:
        idx = rng.integers(0, rows, n_idx)
        idx[1] = idx[0]                                   # a repeat, whatever the draw
    x, a = c['obs'], c['action']
    q1 = critic_forward(c['critics'][0], x if idx is None else x[idx], a if idx is None else a[idx])['q']
    c['target'], c['idx'] = (q1 + rng.normal(0.0, 1.0, q1.shape[0])).astype(dtype), idx
    c['want_critic'] = [critic_gradient(cr, x, a, c['target'], idx) for cr in c['critics']]
    c['want_actor'] = actor_gradient(c['actor'], c['critics'][0], x, mean_mode, idx)
    assert all(w['kinks'] == 0 for w in c['want_critic'])
    return c


def inside(got, want, dtype=np.float32, key='flat', bound='bound', scale='scale'):
    """(every element inside, the largest error over its allowance): float32 against the bound, float64 against
    1e-12 scale + 1e-14."""
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(-1) - np.asarray(want[key]).reshape(-1))
    allow = np.asarray(want[bound]).reshape(-1) if dtype == np.float32 else 1e-12 * np.asarray(want[scale]).reshape(-1) + 1e-14
    ratio = err / np.maximum(allow, 1e-300)
    return bool((err <= allow).all()), float(ratio.max())
