"""Float64 restatement of what libatacom_fit.so computes (include/atacom_fit_hip.h; test infrastructure only): the loss, the
statistics and every gradient of the value head and of PPO's clipped surrogate through the 2 x 64 network, with the bound a
float32 evaluation is held to, per element.  A helper module: it holds no test.

PINNED: tests/test_fit_oracle.py checks `gradient` against torch's float64 autograd of the expressions of
examples/ppo_air_hockey.py to 1e-12, and holds torch's own FLOAT32 autograd result to the float32 bound.

The float32 bound (DESIGN.md section 7c has the derivation) is first-order error propagation with every second-order term kept,
on top of the forward bounds of evaluate_oracle.forward, which are restated here per layer (e_x, e_h1, e_h2, e_y):

  * head.  VALUE: d = y - t carries e_d = e_y + u |d|, dy = 2 d.  PPO: z and logp carry the bounds of evaluate_oracle.log_prob;
    rho = exp(logp - logp_old) carries rho (expm1(e_arg) + gamma(4) exp(e_arg)) with e_arg = e_logp + u |logp - logp_old| -- to
    first order rho e_logp; g = -rho A and dy = g z / std follow by the product rule with gamma(3) for their own roundings.
  * act'.  relu' is exact away from the kink (asserted, see below); tanh' = 1 - h^2 carries 2 |h| e_h + e_h^2 + gamma(2) (1 + h^2).
  * the transposed products W^T delta carry |W|^T e_delta + gamma(K + 1) |W|^T (|delta| + e_delta), K the inner dimension.
  * a weight gradient sum_r delta_r act_r^T carries sum_r (e_delta |act| + |delta| e_act + e_delta e_act) and, for the roundings of
    each product, of the sum over the M rows IN ANY ORDER and of the division by M, gamma(M + 3) times the same backward pass on
    absolute values.  (`scale`, what a float64 evaluation is measured against, is that pass started from the TERMS of dy --
    |a| + |W3| |h2| + |b3| for the difference a - y, the terms of logp for rho -- instead of from its cancelled value.)
  * everything is multiplied by SAFETY = 2, carried over from evaluate_oracle for the matrix cores.

The bound means nothing within a forward error of a kink, so `gradient` counts the rows that have a relu pre-activation within
its forward bound of 0, or a ratio within its bound of 1 +- clip on the side where the advantage's sign makes the clamp bind
(`kinks`); the cases below are generated so that the count is zero, and `case` asserts it.
"""
import math

import numpy as np

from evaluate_oracle import LOG_2PI, SAFETY, TANH_ABS, U32, case_data, gamma, log_prob, random_net  # noqa: F401

VALUE, PPO_CLIP = 0, 1
NAMES = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def forward(net, x):
    """-> dict: xn, a1, h1, a2, h2, y and e_xn, e_a1, e_h1, e_a2, e_h2, e_y, the float32 bounds of evaluate_oracle.forward per
    layer, WITHOUT the factor SAFETY (it is applied once, to the final bounds)."""
    x = _f64(x)
    act = net.get('activation', 'relu')
    shift, scale = _f64(net.get('obs_shift')), _f64(net.get('obs_scale'))
    h = (x - (0.0 if shift is None else shift)) * (1.0 if scale is None else scale)
    e = gamma(2) * np.abs(h)
    out = dict(xn=h, e_xn=e)
    for li, (Wk, bk) in enumerate((('W1', 'b1'), ('W2', 'b2'), ('W3', 'b3'))):
        W, b = _f64(net[Wk]), _f64(net[bk])
        n = 4 * ((W.shape[1] + 3) // 4)
        a = h @ W.T + b
        e = e @ np.abs(W).T + gamma(n + 1) * ((np.abs(h) + e) @ np.abs(W).T + np.abs(b))
        if li < 2:
            h = np.maximum(a, 0.0) if act == 'relu' else np.tanh(a)
            out['a%d' % (li + 1)], out['e_a%d' % (li + 1)] = a, e
            if act == 'tanh':
                e = e + TANH_ABS
            out['h%d' % (li + 1)], out['e_h%d' % (li + 1)] = h, e
        else:
            out['y'], out['e_y'] = a, e
            out['mag_y'] = np.abs(h) @ np.abs(W).T + np.abs(b)
    return out


def _units(exempt, layer):
    """The units of hidden layer `layer` (1 or 2) among the engineered (layer, unit) pairs `exempt` (tests/edge_cases.py)."""
    return [] if exempt is None else [int(u) for l, u in exempt if l == layer]


def _kink(a, e, exempt=None, layer=0, factor=1.0):
    """Per row: a pre-activation within factor * its bound of 0, the engineered units of `exempt` left out."""
    at = np.abs(a) <= factor * e
    at[:, _units(exempt, layer)] = False
    return at.any(1)


def _act_prime(h, e_h, act, open_units=()):
    """(act', its bound) from the activation's value.  open_units: the units whose gate reads h >= 0 (wrong='kink_open')."""
    if act == 'relu':
        ap = (h > 0.0).astype(np.float64)
        ap[:, list(open_units)] = (h[:, list(open_units)] >= 0.0)
        return ap, np.zeros_like(h)
    return 1.0 - h * h, 2.0 * np.abs(h) * e_h + e_h * e_h + gamma(2) * (1.0 + h * h)


def _back(W, d, e_d, ap, e_ap, K):
    """delta_in = (d W) * act' for d [M, out], W [out, in] -> (value, bound)."""
    aW = np.abs(W)
    pre = d @ W
    e_pre = e_d @ aW + gamma(K + 1) * ((np.abs(d) + e_d) @ aW)
    val = pre * ap
    e = e_pre * np.abs(ap) + np.abs(pre) * e_ap + e_pre * e_ap + gamma(1) * np.abs(val)
    return val, e


def _wgrad(d, e_d, A_d, S_d, h, e_h, M):
    """sum_r d_r h_r^T -> (value, bound, scale), unscaled by 1 / M."""
    ah = np.abs(h)
    val = d.T @ h
    scale = S_d.T @ ah
    e = e_d.T @ ah + np.abs(d).T @ e_h + e_d.T @ e_h + gamma(M + 3) * ((A_d + e_d).T @ (ah + e_h))
    return val, e, scale


def gradient(net, x, head, weight, action=None, std=None, logp_old=None, clip=0.2, idx=None, exempt=None, wrong=None):
    """The call of atacom_fit_gradient on rows x [R, n_in] (gathered through idx, if given) -> dict:
    flat, bound, scale: [P (+ n_out)] in the library's order (bound: float32, per element; scale: the backward pass on absolute
        values, what a float64 evaluation is measured against);
    stats, stats_bound, stats_scale: [4];  kinks: the number of rows the bound does not cover (module docstring);
    parts: {name: (value, bound, scale)} of the same numbers by tensor;  inactive: [M] bool (PPO).
    exempt: the engineered (layer, unit) pairs of tests/edge_cases.py, left out of `kinks`; nothing else is.
    wrong='kink_open': the gate of those units reads h >= 0."""
    assert wrong in (None, 'kink_open')
    x, w = _f64(x), _f64(weight)
    act = net.get('activation', 'relu')
    if idx is not None:
        idx = np.asarray(idx)
        x, w = x[idx], w[idx]
        action = None if action is None else _f64(action)[idx]
        logp_old = None if logp_old is None else _f64(logp_old)[idx]
    M = x.shape[0]
    f = forward(net, x)
    y, e_y = f['y'], f['e_y']
    W2, W3 = _f64(net['W2']), _f64(net['W3'])
    kink = np.zeros(M, bool)
    if act == 'relu':
        kink |= _kink(f['a1'], f['e_a1'], exempt, 1, SAFETY) | _kink(f['a2'], f['e_a2'], exempt, 2, SAFETY)
    n_out = y.shape[1]
    ls = e_ls = np.zeros((M, n_out))
    inactive = np.zeros(M, bool)
    if head == VALUE:
        d = y[:, 0] - w
        e_d = e_y[:, 0] + U32 * np.abs(d)
        dy, e_dy = 2.0 * d[:, None], 2.0 * e_d[:, None]
        S_dy = 2.0 * (f['mag_y'] + np.abs(w)[:, None])
        S_ls = ls
        st = np.stack([d * d, np.zeros(M), np.zeros(M)], 1)
        e_st = np.stack([(2.0 * np.abs(d) + e_d) * e_d + gamma(2) * d * d, np.zeros(M), np.zeros(M)], 1)
        a_st = np.abs(st)
    else:
        a, s, lpo = _f64(action), _f64(std), _f64(logp_old)
        z = (a - y) / s
        const = np.abs(np.log(s)).sum() + 0.5 * n_out * LOG_2PI
        logp = (-0.5 * z * z - np.log(s)).sum(-1) - 0.5 * n_out * LOG_2PI
        e_z = (e_y / s) * (1.0 + gamma(4)) + gamma(4) * np.abs(z)
        e_lp = (np.abs(z) * e_z + 0.5 * e_z * e_z).sum(-1) + gamma(n_out + 3) * ((0.5 * (np.abs(z) + e_z) ** 2).sum(-1) + const)
        arg = logp - lpo
        e_arg = e_lp + U32 * np.abs(arg)
        rho = np.exp(arg)
        e_rho = rho * (np.expm1(e_arg) + gamma(4) * np.exp(e_arg))
        lo, hi = 1.0 - clip, 1.0 + clip
        inactive = ((w > 0) & (rho > hi)) | ((w < 0) & (rho < lo))
        kink |= ((w > 0) & (np.abs(rho - hi) <= SAFETY * e_rho + U32 * hi)) | ((w < 0) & (np.abs(rho - lo) <= SAFETY * e_rho + U32 * lo))
        g = np.where(inactive, 0.0, -rho * w)
        e_g = np.where(inactive, 0.0, np.abs(w) * e_rho + gamma(2) * np.abs(rho * w))
        g, e_g = g[:, None], e_g[:, None]
        dy = g * z / s
        e_dy = (np.abs(z) * e_g + np.abs(g) * e_z + e_g * e_z) / s + gamma(3) * np.abs(dy)
        ls = g * (z * z - 1.0)
        e_ls = e_g * np.abs(z * z - 1.0) + (np.abs(g) + e_g) * (2.0 * np.abs(z) * e_z + e_z * e_z) + gamma(3) * np.abs(g) * (z * z + 1.0)
        # what a float64 evaluation is measured against: the terms of a - y and of logp, not their cancelled values
        lp_scale = ((np.abs(z) * (f['mag_y'] + np.abs(a)) / s + 0.5 * z * z).sum(-1) + const + np.abs(lpo))[:, None]
        S_z = (np.abs(a) + f['mag_y']) / s
        S_dy = np.abs(g) * S_z / s + np.abs(dy) * lp_scale
        S_ls = np.abs(g) * (z * z + 1.0 + 2.0 * np.abs(z) * S_z) + np.abs(ls) * lp_scale
        term = -np.minimum(rho * w, np.clip(rho, lo, hi) * w)
        st = np.stack([term, inactive.astype(np.float64), lpo - logp], 1)
        e_st = np.stack([np.abs(w) * e_rho + gamma(2) * np.abs(term), np.zeros(M), e_lp + U32 * np.abs(arg)], 1)
        a_st = np.stack([np.abs(term), inactive.astype(np.float64), np.abs(lpo) + np.abs(z * z).sum(-1) * 0.5 + const], 1)
    # ---- backward, with the same pass on absolute values next to it
    opn = exempt if wrong == 'kink_open' else None
    ap2, e_ap2 = _act_prime(f['h2'], f['e_h2'], act, _units(opn, 2))
    ap1, e_ap1 = _act_prime(f['h1'], f['e_h1'], act, _units(opn, 1))
    A_dy = np.abs(dy)
    da2, e_da2 = _back(W3, dy, e_dy, ap2, e_ap2, 8)
    A_da2 = (A_dy @ np.abs(W3)) * np.abs(ap2)
    S_da2 = (S_dy @ np.abs(W3)) * np.abs(ap2)
    S_da1 = (S_da2 @ np.abs(W2)) * np.abs(ap1)
    da1, e_da1 = _back(W2, da2, e_da2, ap1, e_ap1, 64)
    A_da1 = (A_da2 @ np.abs(W2)) * np.abs(ap1)
    one, zero = np.ones((M, 1)), np.zeros((M, 1))
    parts = {}
    for name, bias, (d, e_d, A_d, S_d), (h, e_h) in (('W1', 'b1', (da1, e_da1, A_da1, S_da1), (f['xn'], f['e_xn'])),
                                                      ('W2', 'b2', (da2, e_da2, A_da2, S_da2), (f['h1'], f['e_h1'])),
                                                      ('W3', 'b3', (dy, e_dy, A_dy, S_dy), (f['h2'], f['e_h2']))):
        parts[name] = _wgrad(d, e_d, A_d, S_d, h, e_h, M)
        parts[bias] = tuple(v[:, 0] for v in _wgrad(d, e_d, A_d, S_d, one, zero, M))
    order = list(NAMES)
    if head == PPO_CLIP:
        parts['log_std'] = tuple(v[:, 0] for v in _wgrad(ls, e_ls, np.abs(ls), S_ls, one, zero, M))
        order.append('log_std')
    parts = {k: (v / M, SAFETY * e / M, sc / M) for k, (v, e, sc) in parts.items()}
    stats = np.append(st.sum(0) / M, 0.0)
    stats_scale = np.append(a_st.sum(0) / M, 0.0)
    stats_bound = np.append(SAFETY * (e_st.sum(0) + gamma(M + 3) * (a_st + e_st).sum(0)) / M, 0.0)
    flat = lambda i: np.concatenate([parts[k][i].reshape(-1) for k in order])             # noqa: E731
    return dict(flat=flat(0), bound=flat(1), scale=flat(2), stats=stats, stats_bound=stats_bound, stats_scale=stats_scale,
                kinks=int(kink.sum()), parts=parts, inactive=inactive, order=order)


# ---- the cases of tests/test_gpu_fit.py, shared with tests/test_fit_oracle.py (which holds torch's own float32 autograd to the
# same bound).  (n_in, n_out, activation, normalise, rows) as in evaluate_oracle; VALUE wherever n_out = 1.
SHAPE_CASES = [(4, 1, 'relu', True, 65), (4, 1, 'tanh', False, 65), (12, 3, 'tanh', False, 65), (12, 3, 'relu', True, 65),
               (18, 5, 'relu', False, 65), (18, 5, 'tanh', True, 65), (20, 2, 'tanh', True, 65), (20, 2, 'relu', False, 65),
               (25, 1, 'tanh', True, 65), (25, 1, 'relu', False, 65), (32, 8, 'relu', True, 65), (32, 8, 'tanh', False, 65)]
# (rows, n_blocks); 600 rows on one workgroup: ten tiles on four wavefronts, so a float32 wavefront walks two and three
ROW_CASES = [(1, 0), (15, 0), (16, 0), (17, 0), (63, 0), (64, 0), (65, 0), (200, 1), (200, 2), (600, 1)]
ROW_SHAPE = {VALUE: (25, 1, 'relu', True), PPO_CLIP: (18, 5, 'relu', True)}
CLIP = 0.2


def _cases():
    """(seed, head, n_in, n_out, activation, normalise, rows): every shape for PPO and, where n_out = 1, for VALUE; every row
    count for both heads."""
    out = []
    for i, (n_in, n_out, act, norm, rows) in enumerate(SHAPE_CASES):
        out.append((100 + i, PPO_CLIP, n_in, n_out, act, norm, rows))
        if n_out == 1:
            out.append((200 + i, VALUE, n_in, n_out, act, norm, rows))
    for head, shape in ROW_SHAPE.items():
        for rows in sorted({r for r, _ in ROW_CASES}):
            out.append((300 + rows, head) + shape + (rows,))
    return out


CASES = _cases()


def case(seed, head, n_in, n_out, activation, normalise, rows, dtype=np.float32, check=True, edge=None):
    """A case in `dtype`: dict(net, x, action, std, weight, logp_old, clip).  VALUE: targets at y + N(0, 1).  PPO: advantages
    N(0, 1); logp_old placed so that rho spans [0.5, 2]; std log-uniform in [1e-2, 2] (evaluate_oracle.case_data) and actions
    out to six standard deviations where the bound allows it (below).  With 64 rows or more a PPO batch holds inactive rows on each side and
    active rows of both signs.  The seed is moved on, deterministically, until no row sits at a kink (zero exclusions); `check`
    asserts what the docstring promises.  edge: a construction of tests/edge_cases.py, edge(net, x) -> the engineered
    (layer, unit) pairs; it changes net and x in place before anything is derived from them, and its units alone are left out of
    the count (c['exempt'])."""
    exempt = None
    for attempt in range(64):
        s = seed + 1000 * attempt
        net, x, action, std = case_data(s, n_in, n_out, activation, normalise, rows, dtype)
        if edge is not None:
            exempt = edge(net, x)
        rng = np.random.default_rng(s + 77)
        if head == VALUE:
            weight = (forward(net, x)['y'][:, 0] + rng.normal(0.0, 1.0, rows)).astype(dtype)
            c = dict(net=net, x=x, action=None, std=None, weight=weight, logp_old=None, clip=CLIP)
        else:
            # The forward bound of rho = exp(logp - logp_old) is sum_k |z_k| e_y / std_k to first order, and e_y is a worst-case
            # bound of 1e-4 to 1e-3: at std = 1e-2 an action six standard deviations out leaves rho unknown to tens of per cent and
            # every row "at a kink".  So the actions are placed where the bound still says something, |z_k| <= min(6, 0.01 std_k /
            # (n_out e_y_k)), and log rho is drawn uniformly over [log 0.5, log 2] LESS a band around log(1 - clip) and
            # log(1 + clip) of twice the row's own bound.
            f = forward(net, x)
            sd = std.astype(np.float64)
            zmax = np.minimum(6.0, 0.01 * sd / (n_out * f['e_y']))
            z = rng.uniform(0.0, 1.0, (rows, n_out)) * zmax * rng.choice([-1.0, 1.0], (rows, n_out))
            if rows > 1:
                z[0] = 0.0
            action = (f['y'] + z * sd).astype(dtype)
            logp, e_lp = log_prob(net, x, action, std)[:2]
            band = 2.0 * SAFETY * e_lp + 1e-3
            log_rho = rng.uniform(math.log(0.5), math.log(2.0), rows)
            for _ in range(200):
                bad = (np.abs(log_rho - math.log(1 - CLIP)) <= band) | (np.abs(log_rho - math.log(1 + CLIP)) <= band)
                if not bad.any():
                    break
                log_rho[bad] = rng.uniform(math.log(0.5), math.log(2.0), int(bad.sum()))
            if rows == 1:                             # a lone row is an active one: an inactive row has no gradient at all
                log_rho[:] = rng.uniform(math.log(0.9), math.log(1.1))
            lpo = (logp - log_rho).astype(dtype)
            weight = rng.normal(0.0, 1.0, rows).astype(dtype)
            c = dict(net=net, x=x, action=action, std=std, weight=weight, logp_old=lpo, clip=CLIP)
        c['exempt'] = exempt
        want = oracle(c, head)
        if want['kinks'] == 0:
            break
    if check:
        assert want['kinks'] == 0, 'no seed without a row at a kink'
        if head == PPO_CLIP and rows >= 64:
            w, ina = c['weight'].astype(np.float64), want['inactive']
            assert (ina & (w > 0)).any() and (ina & (w < 0)).any() and (~ina & (w > 0)).any() and (~ina & (w < 0)).any()
            rho = np.exp(log_prob(net, x, c['action'], std)[0] - c['logp_old'].astype(np.float64))
            assert rho.min() < 0.6 and rho.max() > 1.7 and 1e-2 <= c['std'].min() and c['std'].max() <= 2.0
    c['want'] = want
    return c


def oracle(c, head, idx=None, wrong=None):
    return gradient(c['net'], c['x'], head, c['weight'], c['action'], c['std'], c['logp_old'], c['clip'], idx, c.get('exempt'), wrong)
