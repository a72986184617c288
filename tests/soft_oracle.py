"""Float64 restatement of what libatacom_soft.so computes (include/atacom_soft_hip.h; test infrastructure only): the squashed
Gaussian's sample and log-probability, the soft TD target, the critics' gradients, the actor's gradients with respect to the mu
and sigma networks and the gradient of the alpha loss, each with the bound a float32 evaluation is held to, per element, and the
case builder the CPU and GPU tests share.  A helper module: it holds no test.

PINNED: tests/test_soft_oracle.py checks every quantity against torch modules, torch.distributions.Normal(...).rsample /
log_prob and float64 autograd to 1e-12 of scale, and shows that six deliberately wrong restatements fall outside the float32 bound.

Built from what the neighbouring oracles export: the forward chains and the critic-free backward pass of offgrad_oracle
(actor_forward, _network_backward, _k, _pack's conventions), fit_oracle's _act_prime, _back and _wgrad, evaluate_oracle's gamma,
SAFETY (on the products that run on the matrix cores), TANH_ABS and random_net, optim_oracle's EXP_ULPS.  The row arithmetic
between the products runs on the vector unit, one rounding u per operation: the class V below carries (value, float32 bound,
magnitude) through the header's lines.

logf: the ROCm installation carries no document that states the HIP math API's bound, so the device's logf was measured against float64 over
the exercised argument range [1e-6, 1 + 1e-6] (2^22 points): LOG_MEASURED ulp at worst; LOG_ULPS allows twice that.
(profiles/soft.md holds both numbers.)

The log(w + 1e-6) term is ill-conditioned at saturation: its bound is per sample from the oracle's own 1 / (w + 1e-6).  The
bounded cases keep |u| moderate, so that the bound on logp stays below LOGP_BOUND on every row (`case` asserts it); the
saturation case (|u| up to about 8) is held to finiteness, to the per-sample bound, and in float64 to 1e-12 scale plus
8 * 2^-53 / (w + 1e-6) per element.  torch's own (u - m) / s loses digits for tiny s, so the cases keep the clamped log sigma
inside LOG_STD_RANGE, and `case` asserts that too.

The bounds mean nothing within a forward error of a ReLU kink, of a tie |q_1 - q_2| or of a clamp edge; `case` draws such rows
again until there is none (`row_flags`) and asserts it.  No row is excluded from a comparison.
"""
import functools
import math

import numpy as np

from evaluate_oracle import SAFETY, TANH_ABS, U32, gamma, random_net
from fit_oracle import _act_prime, _back, _kink, _units, _wgrad
from offgrad_oracle import _k, _network_backward, _of, actor_forward, inside  # noqa: F401
from offpolicy_oracle import _f64, _hidden, _layer, _normalise
from optim_oracle import EXP_ULPS

PARAMS = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
LOG_MEASURED = 1.8811                       # worst error of the device's logf over [1e-6, 1 + 1e-6], in ulps (measured)
LOG_ULPS = 2.0 * LOG_MEASURED               # what the bound allows: twice the measurement
U_MAX = 2.0                                 # the bounded cases keep |u| below this: w = 1 - tanh(u)^2 >= 0.07
LOGP_BOUND = 0.1                            # ... so that the float32 bound on logp stays below this on every row: a hundredth of
                                            # the |logp| of these cases, and gamma alpha 0.1 = 0.02 on a target of O(1)
LOG_STD_RANGE = (-2.0, 0.5)                 # the bounded cases' clamp range lies inside it
TINY = 2.0 ** -126


class V:
    """(value, float32 bound, magnitude): what a float32 evaluation may differ by, and the scale a float64 one is measured on."""
    __slots__ = ('v', 'e', 's')

    def __init__(self, v, e=None, s=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)
        self.s = np.abs(self.v) if s is None else np.broadcast_to(np.asarray(s, dtype=np.float64), self.v.shape)


def _rounded(v, e, s):
    return V(v, e + U32 * (np.abs(v) + e), s)


def mul(a, b):
    v = a.v * b.v
    return _rounded(v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e, a.s * b.s)


def add(a, b, sign=1.0):
    return _rounded(a.v + sign * b.v, a.e + b.e, a.s + b.s)


def div(a, b, floor=0.0):
    """floor: what |b| of a device cannot fall below, whatever its bound says."""
    v = a.v / b.v
    lo = np.maximum(np.abs(b.v) - b.e, floor)
    assert (lo > 0).all()
    return _rounded(v, (a.e + np.abs(v) * b.e) / lo, a.s / np.abs(b.v) + np.abs(v) * b.s / np.abs(b.v))


def _sum_k(x):
    """((x_0 + x_1) + ...) over the last axis."""
    k = x.v.shape[-1]
    return V(x.v.sum(-1), x.e.sum(-1) + gamma(max(k - 1, 0)) * (np.abs(x.v) + x.e).sum(-1), x.s.sum(-1))


def _vec(v, k, default=1.0):
    return np.ones(k) * (default if v is None else _f64(v))


# ------------------------------------------------------------------------------------------------------------- forward
WRONG_EDGES = ('kink_open', 'tie_second', 'edge_open', 'absorbing_ge')      # each applies to the engineered units, rows, elements only


def _cols(exempt, k):
    """[k] bool: the log sigma elements that a case's description places exactly on a clamp bound."""
    v = _of(exempt, 'edge')
    return np.zeros(k, bool) if v is None else np.asarray(v, bool)


def _rows(exempt, M):
    """[M] bool: the rows on which a case's description makes the two critics equal bit for bit."""
    v = _of(exempt, 'tie')
    return np.zeros(M, bool) if v is None else np.asarray(v, bool)


def sample(pol, x, eps, act_scale=None, act_shift=None, wrong=None, exempt=None):
    """The header's row arithmetic on rows x [M, D] with eps [M, k] -> dict of V: a, logp, t, w, e, p and m, lr; `open` [M, k]
    (the clamp gate), `clamped` [M], `edge` [M] (a log sigma within twice its bound of a clamp bound), `kink` [M], `sat` [M, k]
    (the float64 allowance 8 * 2^-53 / e).  wrong='no_1e6': the 1e-6 omitted.
    exempt: a case's description (tests/edge_cases.py): {'mu': pairs, 'sigma': pairs} the engineered (layer, unit) pairs left out
    of `kink`, {'edge': [k] bool} the log sigma elements placed exactly on a bound, left out of `edge`.  wrong='edge_open': the
    gate of those elements reads lmin <= l_raw <= lmax."""
    eps = _f64(eps)
    k = eps.shape[1]
    fm, fs = actor_forward(pol['mu'], x, _of(exempt, 'mu')), actor_forward(pol['sigma'], x, _of(exempt, 'sigma'))
    m, lr = V(fm['m'], fm['e_m'], fm['mag_m']), V(fs['m'], fs['e_m'], fs['mag_m'])
    lmin, lmax = pol['log_std_min'], pol['log_std_max']
    opn = (lmin < lr.v) & (lr.v < lmax)
    cols = _cols(exempt, k)
    if wrong == 'edge_open':
        opn = np.where(cols, (lmin <= lr.v) & (lr.v <= lmax), opn)
    edge = ((np.minimum(np.abs(lr.v - lmin), np.abs(lr.v - lmax)) <= 2.0 * lr.e) & ~cols).any(1)
    lv = np.clip(lr.v, lmin, lmax)
    l = V(lv, np.where(opn, lr.e, 0.0), np.where(opn, lr.s, np.abs(lv)))
    sv = np.exp(l.v)
    s = V(sv, sv * (np.expm1(l.e) + EXP_ULPS * 2 * U32 * np.exp(l.e)), sv * (1.0 + l.s))
    ev = V(eps)
    p = mul(s, ev)
    u = add(m, p)
    tv = np.tanh(u.v)
    t = V(tv, u.e + TANH_ABS, 1.0 + u.s)
    sc, sh = V(_vec(act_scale, k)), V(_vec(act_shift, k, 0.0))
    a = add(mul(sc, t), sh)
    wv, e_w = _act_prime(t.v, t.e, 'tanh')
    w = V(wv, e_w, 1.0 + 2.0 * t.s)
    e = w if wrong == 'no_1e6' else add(w, V(np.float64(1e-6), U32 * 1e-6))
    # a device's w = fma(-t, t, 1) is never negative (|t| <= 1), so its e is at least fl(1e-6): where the bound on e reaches below
    # that, the logarithm still lies above log(fl(1e-6)) -- the per-sample bound stays finite at saturation
    floor = TINY if wrong == 'no_1e6' else 1e-6 * (1.0 - 2.0 * U32)
    lo = np.maximum(e.v - e.e, floor)
    cv = np.log(e.v)
    e_c = np.maximum(np.log(e.v / lo), np.log1p(e.e / e.v)) + LOG_ULPS * 2 * U32 * np.abs(cv) + TINY
    c = V(cv, e_c, np.abs(cv) + e.s / np.abs(e.v))
    g = V(-0.5 * eps * eps, U32 * 0.5 * eps * eps)
    g = add(g, l, -1.0)
    g = add(g, V(np.float64(HALF_LOG_2PI), U32 * HALF_LOG_2PI), -1.0)
    logp = add(_sum_k(g), _sum_k(c), -1.0)
    return dict(a=a, logp=logp, t=t, w=w, e=e, p=p, m=m, lr=lr, u=u, s=s, open=opn, clamped=~opn.all(1), edge=edge,
                kink=fm['kink'] | fs['kink'], sat=8.0 * 2.0 ** -53 / np.abs(e.v))


def critic_forward(c, x, a, e_a=None, exempt=None):
    """The plain 2 x 64 critic on [xn | a], a raw, with everything a backward pass needs.  exempt: this critic's engineered
    (layer, unit) pairs, left out of `kink` and `kink2`."""
    act = c.get('activation', 'relu')
    a = _f64(a)
    xn, e_x = _normalise(c, x)
    x1 = np.concatenate([xn, a], 1)
    e_x1 = np.concatenate([e_x, np.zeros_like(a) if e_a is None else e_a], 1)
    a1, e_a1, _ = _layer(x1, e_x1, c['W1'], c['b1'])
    h1, e_h1 = _hidden(a1, e_a1, act)
    a2, e_a2, _ = _layer(h1, e_h1, c['W2'], c['b2'])
    h2, e_h2 = _hidden(a2, e_a2, act)
    q, e_q, mag = _layer(h2, e_h2, c['W3'], c['b3'])
    kink = np.zeros(x1.shape[0], bool)
    kink2 = kink.copy()
    if act == 'relu':
        kink = _kink(a1, e_a1, exempt, 1) | _kink(a2, e_a2, exempt, 2)
        kink2 = _kink(a1, e_a1, exempt, 1, 2.0) | _kink(a2, e_a2, exempt, 2, 2.0)
    return dict(x1=x1, e_x1=e_x1, h1=h1, e_h1=e_h1, h2=h2, e_h2=e_h2, q=V(q[:, 0], e_q[:, 0], mag[:, 0]), kink=kink, kink2=kink2, act=act)


def _alpha(log_alpha):
    al = math.exp(float(log_alpha))
    return V(np.float64(al), al * EXP_ULPS * 2 * U32)


def target(pol, critics, next_obs, reward, absorbing, g, log_alpha, eps, act_scale=None, act_shift=None, idx=None, action=None,
           logp=None, wrong=None, exempt=None):
    """atacom_soft_target -> dict: y (V), a, logp (V), q [2] (V), tie [M], kink [M], edge [M], sat [M] (the float64 allowance on y).
    action, logp: a device's action_out and logp_out taken as exact -- what y is then held to (offpolicy_oracle's
    target_from_action): the bound of the whole chain covers no row whose critic has a ReLU pre-activation within the error that
    the action's own bound gives it (`kinks_e2e` counts them: zero for tanh networks, most rows for ReLU).
    `kink`, `tie`: at the action taken as exact, within TWICE the bounds.
    wrong='larger': the larger critic; 'absorbing': (1 - absorbing) applied to q but not to alpha logp; 'no_1e6'.
    exempt: a case's description (sample's keys, and {'critics': [pairs, pairs]} for the pair this call is given, {'tie': [M]
    bool} the rows of an engineered tie): left out of kink, edge and tie; nothing else is.  wrong='absorbing_ge': the flag read
    as >= 0.5; 'edge_open' (sample)."""
    x, r, ab = _f64(next_obs), _f64(reward), _f64(absorbing)
    if idx is not None:
        x, r, ab = x[np.asarray(idx)], r[np.asarray(idx)], ab[np.asarray(idx)]
    s = sample(pol, x, eps, act_scale, act_shift, wrong=wrong, exempt=exempt)
    cut = action is not None
    a_v = _f64(action) if cut else s['a'].v
    fq = [critic_forward(c, x, a_v, None if cut else s['a'].e, _of(exempt, 'critics', j)) for j, c in enumerate(critics)]
    fx = fq if cut else [critic_forward(c, x, a_v, exempt=_of(exempt, 'critics', j)) for j, c in enumerate(critics)]
    q1, q2 = fq[0]['q'], fq[1]['q']
    two = q2.v < q1.v
    if wrong == 'larger':
        two = ~two
    q = V(np.where(two, q2.v, q1.v), np.where(two, q2.e, q1.e), np.where(two, q2.s, q1.s))
    tie = (np.abs(fx[0]['q'].v - fx[1]['q'].v) <= 2.0 * (fx[0]['q'].e + fx[1]['q'].e)) & ~_rows(exempt, x.shape[0])
    al = _alpha(log_alpha)
    lp = s['logp'] if logp is None else V(_f64(logp))
    z1 = mul(al, lp)
    keep = V(np.where((ab >= 0.5) if wrong == 'absorbing_ge' else (ab > 0.5), 0.0, 1.0))
    if wrong == 'absorbing':
        z = add(mul(keep, q), z1, -1.0)
    else:
        z = mul(keep, add(q, z1, -1.0))
    y = add(V(r), mul(V(np.float64(g)), z))
    kink = s['kink'] | fx[0]['kink2'] | fx[1]['kink2']
    return dict(y=y, a=s['a'], logp=s['logp'], q=(q1, q2), tie=tie, kink=kink, edge=s['edge'], clamped=s['clamped'],
                kinks_e2e=int((fq[0]['kink'] | fq[1]['kink']).sum()), sat=abs(float(g)) * al.v * s['sat'].sum(1), u=s['u'])


# ------------------------------------------------------------------------------------------------------------ backward
def _grads(net, fwd, dy, x_in, e_x_in, M, opn=None):
    """{name: (value, bound, scale)} of a network's six tensors from dy (a V [M, n_out]), unscaled by 1 / M.  opn: the (layer,
    unit) pairs whose gate reads h >= 0 (wrong='kink_open')."""
    D2, D1 = _network_backward(_f64(net['W2']), _f64(net['W3']), dy.v, dy.e, dy.s, fwd['h1'], fwd['e_h1'], fwd['h2'], fwd['e_h2'], fwd['act'],
                               opn)
    DY = (dy.v, dy.e, np.abs(dy.v), dy.s)
    one, zero = np.ones((M, 1)), np.zeros((M, 1))
    Mk = _k(M, 3)
    parts = {}
    for name, bias, dd, (h, e_h) in (('W1', 'b1', D1, (x_in, e_x_in)), ('W2', 'b2', D2, (fwd['h1'], fwd['e_h1'])),
                                     ('W3', 'b3', DY, (fwd['h2'], fwd['e_h2']))):
        parts[name] = _wgrad(*dd, h, e_h, Mk)
        parts[bias] = tuple(v[:, 0] for v in _wgrad(*dd, one, zero, Mk))
    return parts


def _pack(parts, M, stats):
    """offgrad_oracle._pack with any number of statistics: stats = [V [M]] -> means."""
    parts = {k: (v / M, e / M, sc / M) for k, (v, e, sc) in parts.items()}
    flat = lambda i: np.concatenate([parts[k][i].reshape(-1) for k in PARAMS])             # noqa: E731
    st = np.zeros(4), np.zeros(4), np.zeros(4)
    for j, t in enumerate(stats):
        st[0][j] = t.v.sum() / M
        st[1][j] = (t.e.sum() + gamma(M + 3) * (np.abs(t.v) + t.e).sum()) / M
        st[2][j] = t.s.sum() / M
    return dict(flat=flat(0), bound=flat(1), scale=flat(2), parts=parts, stats=st[0], stats_bound=st[1], stats_scale=st[2])


def critic_gradient(c, x, a, tgt, idx=None, exempt=None, wrong=None):
    """atacom_soft_critic_gradient for one critic -> dict: flat, bound, scale in the order of PARAMS; stats...; kinks.
    exempt: this critic's engineered (layer, unit) pairs, left out of `kinks`; wrong='kink_open': their gate reads h >= 0."""
    assert wrong in (None, 'kink_open')
    x, a, t = _f64(x), _f64(a), _f64(tgt)
    if idx is not None:
        x, a = x[np.asarray(idx)], a[np.asarray(idx)]
    M = x.shape[0]
    f = critic_forward(c, x, a, exempt=exempt)
    d = add(f['q'], V(t), -1.0)
    d = V(d.v, d.e, f['q'].s + np.abs(t))
    dy = V(2.0 * d.v[:, None], 2.0 * d.e[:, None], 2.0 * d.s[:, None])
    out = _pack(_grads(c, f, dy, f['x1'], f['e_x1'], M, exempt if wrong == 'kink_open' else None), M, [mul(d, d)])
    out['kinks'] = int(f['kink'].sum())
    return out


def dqda(c, f, D, opn=None):
    """dq/da of a critic from its forward dict: the a-columns of W1^T delta1 -> V [M, k].  opn: as in _grads."""
    W1, W2, W3 = (_f64(c[n]) for n in ('W1', 'W2', 'W3'))
    M = f['h1'].shape[0]
    ap2, e_ap2 = _act_prime(f['h2'], f['e_h2'], f['act'], _units(opn, 2))
    ap1, e_ap1 = _act_prime(f['h1'], f['e_h1'], f['act'], _units(opn, 1))
    d2, e_d2 = _back(W3, np.ones((M, 1)), np.zeros((M, 1)), ap2, e_ap2, 0)
    A_d2 = np.abs(W3) * np.abs(ap2)
    d1, e_d1 = _back(W2, d2, e_d2, ap1, e_ap1, _k(64, 1))
    A_d1 = (A_d2 @ np.abs(W2)) * np.abs(ap1)
    Wa = W1[:, D:]
    k = Wa.shape[1]
    gs, e_gs = _back(Wa, d1, e_d1, np.ones((M, k)), np.zeros((M, k)), _k(64, 1))
    return V(gs, e_gs, A_d1 @ np.abs(Wa))


def actor_gradient(pol, critics, x, eps, log_alpha, target_entropy, act_scale=None, act_shift=None, idx=None, action=None, q=None,
                   dq=None, wrong=None, exempt=None):
    """atacom_soft_actor_gradient -> dict: mu, sigma (each flat, bound, scale, parts), stats, stats_bound, stats_scale [4]
    (from mu's pack), a, logp (V), q (V, V), dqda (V), two [M], flags kink / tie / edge [M].
    The chain can be cut at a device's own intermediates, as offgrad_oracle.actor_gradient's:
      action: the action taken as exact (action_out) -- what q and dqda are then held to;
      q [M, 2]: the critics' values taken as exact (q_out): they decide the selection;
      dq [M, k]: dq/da taken as exact (dqda_out) -- what the gradients are then held to.
    wrong='no_alpha': the -alpha term of dl dropped; 'no_gate': the clamp gate ignored; 'larger': the larger critic selected;
    'no_1e6'; 'no_scale': act_scale missing from du.
    exempt: a case's description (target's keys): what it engineers is left out of kink, tie and edge; nothing else is.  On the
    engineered units, rows and elements only: wrong='kink_open': the ReLU gate reads h >= 0; 'tie_second': q_2 <= q_1 selects
    critic 2; 'edge_open': the clamp gate reads lmin <= l_raw <= lmax."""
    x = _f64(x)
    if idx is not None:
        x = x[np.asarray(idx)]
    M, D = x.shape
    opn = (exempt or {}) if wrong == 'kink_open' else {}
    s = sample(pol, x, eps, act_scale, act_shift, wrong=wrong, exempt=exempt)
    k = s['a'].v.shape[1]
    a_v, a_e = (s['a'].v, s['a'].e) if action is None else (_f64(action), None)
    fq = [critic_forward(c, x, a_v, a_e, _of(exempt, 'critics', j)) for j, c in enumerate(critics)]
    fx = fq if a_e is None else [critic_forward(c, x, a_v, exempt=_of(exempt, 'critics', j)) for j, c in enumerate(critics)]
    q1, q2 = fq[0]['q'], fq[1]['q']
    tied = _rows(exempt, M)
    tie = (np.abs(fx[0]['q'].v - fx[1]['q'].v) <= 2.0 * (fx[0]['q'].e + fx[1]['q'].e)) & ~tied
    qa, qb = (q1.v, q2.v) if q is None else (_f64(q)[:, 0], _f64(q)[:, 1])
    two = qb < qa
    if wrong == 'larger':
        two = ~two
    if wrong == 'tie_second':
        two = np.where(tied, qb <= qa, two)
    qs = V(np.where(two, q2.v, q1.v), np.where(two, q2.e, q1.e), np.where(two, q2.s, q1.s))
    g1, g2 = dqda(critics[0], fq[0], D, _of(opn, 'critics', 0)), dqda(critics[1], fq[1], D, _of(opn, 'critics', 1))
    sel = two[:, None]
    gq = V(np.where(sel, g2.v, g1.v), np.where(sel, g2.e, g1.e), np.where(sel, g2.s, g1.s))
    dqv = gq if dq is None else V(_f64(dq))
    al = _alpha(log_alpha)
    t, w, e, p = s['t'], s['w'], s['e'], s['p']
    r = div(mul(V(2.0 * t.v, 2.0 * t.e, 2.0 * t.s), w), e, floor=TINY if wrong == 'no_1e6' else 1e-6 * (1.0 - 2.0 * U32))
    sc = V(_vec(None if wrong == 'no_scale' else act_scale, k))
    du = add(mul(al, r), mul(dqv, mul(sc, w)), -1.0)
    dm = du
    dl = mul(du, p) if wrong == 'no_alpha' else add(mul(du, p), al, -1.0)
    gate = np.ones_like(s['open']) if wrong == 'no_gate' else s['open']
    dl = V(np.where(gate, dl.v, 0.0), np.where(gate, dl.e, 0.0), np.where(gate, dl.s, 0.0))
    fm, fs = actor_forward(pol['mu'], x), actor_forward(pol['sigma'], x)
    term = add(mul(al, s['logp']), qs, -1.0)
    ent = add(s['logp'], V(np.float64(target_entropy)))
    stats = [term, s['logp'], V(-ent.v, ent.e, ent.s), V(s['clamped'].astype(np.float64))]
    out = dict(mu=_pack(_grads(pol['mu'], fm, dm, fm['xn'], fm['e_xn'], M, _of(opn, 'mu')), M, stats),
               sigma=_pack(_grads(pol['sigma'], fs, dl, fs['xn'], fs['e_xn'], M, _of(opn, 'sigma')), M, []))
    out.update(stats=out['mu']['stats'], stats_bound=out['mu']['stats_bound'], stats_scale=out['mu']['stats_scale'], a=s['a'],
               logp=s['logp'], q=(q1, q2), dqda=gq, two=two, tie=tie, edge=s['edge'], clamped=s['clamped'], open=s['open'], lr=s['lr'],
               kink=s['kink'] | fx[0]['kink2'] | fx[1]['kink2'], kinks_e2e=int((fq[0]['kink'] | fq[1]['kink']).sum()), sat=s['sat'],
               u=s['u'], dm=dm, dl=dl)
    return out


def alpha_step32(x, g, m, v, head, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
    """The header's Adam step on one value, every operation an individually rounded float32 one (optim_oracle.step32 with
    scale = 1) -> (x, m, v, head)."""
    import optim_oracle
    o = optim_oracle.step32(np.array([x], np.float32), np.array([g], np.float32), np.array([m], np.float32), np.array([v], np.float32),
                            head, lr=lr, betas=betas, eps=eps)
    return o['p'][0], o['m'][0], o['v'][0], o['head']


# ---------------------------------------------------------------------------------------------------------------- cases
ROW_CASES = [(1, 0), (15, 0), (16, 0), (17, 0), (63, 0), (64, 0), (65, 0), (200, 1), (200, 2), (600, 1)]
ROW_SHAPE = (18, 5, 'relu', True, True)
# (D, k, activation, normalise, act_scale and act_shift): every ceil(D / 4) and every ceil((D + k) / 4) from 1 to 8
SHAPE_CASES = [(1, 1, 'relu', True, True), (4, 1, 'tanh', False, False), (12, 3, 'relu', False, True), (18, 5, 'tanh', True, False),
               (20, 2, 'relu', True, True), (24, 8, 'tanh', False, True), (31, 1, 'relu', True, False), (8, 4, 'tanh', True, True),
               (16, 2, 'relu', False, False), (26, 2, 'tanh', True, True)]
REDRAWS = 200
GAMMA, LOG_ALPHA = 0.99, math.log(0.2)


def random_policy(rng, D, k, activation, normalise, dtype, saturate=False):
    mu, sigma = random_net(rng, D, k, activation, normalise, dtype), random_net(rng, D, k, activation, False, dtype)
    sigma['obs_shift'], sigma['obs_scale'] = mu['obs_shift'], mu['obs_scale']          # a policy has one normalisation
    if saturate:
        mu['W3'], mu['b3'] = (mu['W3'] * dtype(8.0)).astype(dtype), (mu['b3'] * dtype(8.0)).astype(dtype)
    # the clamp range from the sigma network's own outputs on probe observations, so that rows lie beyond both bounds
    probe = actor_forward(sigma, rng.normal(0.0, 1.0, (256, D)))['m']
    centre = float(np.median(probe))
    sigma['b3'] = (sigma['b3'].astype(np.float64) - centre - 0.75).astype(dtype)
    probe = probe - centre - 0.75
    lo, hi = np.floor(np.quantile(probe, 0.2) * 64.0) / 64.0, np.ceil(np.quantile(probe, 0.8) * 64.0) / 64.0
    lo, hi = max(lo, LOG_STD_RANGE[0]), min(hi, LOG_STD_RANGE[1])                     # inside the range that torch's (u - m) / s holds
    return dict(mu=mu, sigma=sigma, log_std_min=float(lo), log_std_max=float(max(hi, lo + 1.0 / 64.0)))


def random_soft_critic(rng, D, k, activation, normalise, dtype):
    c = random_net(rng, D + k, 1, activation, False, dtype)
    if normalise:
        c['obs_shift'] = rng.uniform(-1.0, 1.0, D).astype(dtype)
        c['obs_scale'] = rng.uniform(0.2, 2.0, D).astype(dtype)
    return c


def row_flags(c, exempt=None):
    """Per row of the case's data: at a ReLU kink (of a policy network, of a critic at the recorded action, of a critic at the
    policy's action within TWICE its bound), at a tie of the two critics, or at a clamp edge -- for the online and the target pair.
    exempt: a case's description (target's keys; 'critics' describes both pairs): what it engineers is left out, nothing else."""
    x, sc, sh = c['obs'], c['act_scale'], c['act_shift']
    bad = np.zeros(x.shape[0], bool)
    for j, cr in enumerate(c['critics']):
        bad |= critic_forward(cr, x, c['action'], exempt=_of(exempt, 'critics', j))['kink']
    for pair in (c['critics'], c['targets']):
        t = target(c['policy'], pair, x, c['reward'], c['absorbing'], c['gamma'], c['log_alpha'], c['eps'], sc, sh, exempt=exempt)
        bad |= t['kink'] | t['tie'] | t['edge']
        if not c['saturate']:
            bad |= (np.abs(t['u'].v) + t['u'].e > U_MAX).any(1)
    return bad


@functools.lru_cache(maxsize=None)
def case(seed, D, k, activation, normalise, with_act, rows, dtype=np.float32, n_idx=0, saturate=False):
    """A case in `dtype`: the policy, the online and the target critic pair, obs (used as next_obs too), the recorded action,
    reward, absorbing, eps (row r of the CALL), log_alpha, gamma, target_entropy and a target at Q_1 + N(0, 1) per row of the
    call.  With n_idx > 0 the call names n_idx rows through `idx`, unsorted and with repeats; eps then has n_idx rows.
    -> dict with want_target, want_critic (one per critic) and want_actor.  Cached: the tests share one reference."""
    rng = np.random.default_rng(seed)
    pol = random_policy(rng, D, k, activation, normalise, dtype, saturate)
    assert LOG_STD_RANGE[0] <= pol['log_std_min'] < pol['log_std_max'] <= LOG_STD_RANGE[1], (pol['log_std_min'], pol['log_std_max'])
    c = dict(policy=pol, critics=[random_soft_critic(rng, D, k, activation, normalise, dtype) for _ in range(2)],
             targets=[random_soft_critic(rng, D, k, activation, normalise, dtype) for _ in range(2)], dtype=dtype, D=D, k=k,
             activation=activation, saturate=saturate, gamma=float(dtype(GAMMA)), log_alpha=float(dtype(LOG_ALPHA)), target_entropy=float(-k))
    c['act_scale'] = rng.uniform(0.5, 2.0, k).astype(dtype) if with_act else None
    c['act_shift'] = rng.uniform(-0.5, 0.5, k).astype(dtype) if with_act else None
    sc, sh = _vec(c['act_scale'], k), _vec(c['act_shift'], k, 0.0)
    c['obs'] = rng.normal(0.0, 1.0, (rows, D)).astype(dtype)
    c['action'] = (rng.uniform(-1.0, 1.0, (rows, k)) * sc + sh).astype(dtype)
    c['reward'] = rng.normal(0.0, 1.0, rows).astype(dtype)
    c['absorbing'] = (rng.uniform(0.0, 1.0, rows) < 0.25).astype(dtype)
    idx = None
    if n_idx:
        idx = rng.integers(0, rows, n_idx)
        idx[1] = idx[0]                                   # a repeat, whatever the draw
    M = n_idx or rows
    draw = lambda n: np.clip(rng.normal(0.0, 1.0, (n, k)), -2.0, 2.0).astype(dtype)         # noqa: E731
    c['eps'], c['idx'] = draw(M), idx
    if idx is None:
        for _ in range(REDRAWS):
            bad = row_flags(c)
            if not bad.any():
                break
            n = int(bad.sum())
            c['obs'][bad] = rng.normal(0.0, 1.0, (n, D)).astype(dtype)
            c['action'][bad] = (rng.uniform(-1.0, 1.0, (n, k)) * sc + sh).astype(dtype)
            c['eps'][bad] = draw(n)
        assert not row_flags(c).any(), 'rows at a kink, a tie or a clamp edge after %d redraws' % REDRAWS
    else:                                                    # eps belongs to the call's rows: redraw them and the storage's rows they name
        full = dict(c, obs=c['obs'][idx], action=c['action'][idx], reward=c['reward'][idx], absorbing=c['absorbing'][idx])
        for _ in range(REDRAWS):
            bad = row_flags(full)
            if not bad.any():
                break
            for j in sorted(set(idx[bad].tolist())):
                c['obs'][j] = rng.normal(0.0, 1.0, D).astype(dtype)
                c['action'][j] = (rng.uniform(-1.0, 1.0, k) * sc + sh).astype(dtype)
            c['eps'][bad] = draw(int(bad.sum()))
            full.update(obs=c['obs'][idx], action=c['action'][idx])
        assert not row_flags(full).any(), 'rows at a kink, a tie or a clamp edge after %d redraws' % REDRAWS
    x, a = c['obs'], c['action']
    q1 = critic_forward(c['critics'][0], x if idx is None else x[idx], a if idx is None else a[idx])['q'].v
    c['target'] = (q1 + rng.normal(0.0, 1.0, M)).astype(dtype)
    args = (c['log_alpha'], c['eps'], c['act_scale'], c['act_shift'], idx)
    c['want_target'] = target(pol, c['targets'], x, c['reward'], c['absorbing'], c['gamma'], *args)
    c['want_critic'] = [critic_gradient(cr, x, a, c['target'], idx) for cr in c['critics']]
    c['want_actor'] = actor_gradient(pol, c['critics'], x, c['eps'], c['log_alpha'], c['target_entropy'], c['act_scale'], c['act_shift'], idx)
    assert all(w['kinks'] == 0 for w in c['want_critic'])
    if not saturate:                                         # the bound on logp is small on every row, of both calls
        for w in (c['want_target'], c['want_actor']):
            assert (w['logp'].e <= LOGP_BOUND).all(), float(w['logp'].e.max())
    return c


def inside_v(got, want, dtype=np.float32, extra=None):
    """(every element inside, the largest error over its allowance) of an array against a V: float32 against the bound,
    float64 against 1e-12 scale + 1e-14 (+ extra)."""
    err = np.abs(np.asarray(got, dtype=np.float64).reshape(-1) - want.v.reshape(-1))
    allow = want.e.reshape(-1) if dtype == np.float32 else 1e-12 * want.s.reshape(-1) + 1e-14 + (0.0 if extra is None else np.asarray(extra).reshape(-1))
    return bool((err <= allow).all()), float((err / np.maximum(allow, 1e-300)).max())
