"""Float64 restatement of what libatacom_trust.so and rl_on_manifold_amd/trust.py compute (include/atacom_trust_hip.h; test
infrastructure only): the product of the policy's Fisher matrix with a vector through the 2 x 64 network, with the bound a
float32 evaluation is held to per element; the conjugate-gradient loop; and the TRPO policy step with its line search.  A helper
module: it holds no test.

PINNED: tests/test_trust_oracle.py checks `fvp` against torch's float64 double backward through
torch.distributions.kl_divergence to 1e-12 of the element's scale, and holds torch's own FLOAT32 double backward to the float32
bound.  UNPINNED: `cg` and `trpo` restate MushroomRL 1.x's TRPO (conjugate gradients, step length, backtracking line search)
from its published source, which is not installed here; `cg` is checked against a dense solve.

The float32 bound (DESIGN.md section 7e has the derivation) extends fit_oracle's first-order propagation, second-order terms
kept, by the tangent pass.  With the forward bounds e_xn, e_h1, e_h2 of fit_oracle.forward, gamma(n) = n u / (1 - n u):

  * p1 = V1 xn + vb1 carries |V1| e_xn + gamma(n_in' + 1) (|V1| (|xn| + e_xn) + |vb1|), n_in' = n_in padded to a multiple of 4;
    t1 = p1 act'(a1) carries e_p1 |act'| + |p1| e_act' + e_p1 e_act' + gamma(1) |t1|, act' and its bound as in
    fit_oracle._act_prime (relu' is exact away from the kink, asserted);
  * p2 = W2 t1 + V2 h1 + vb2 is the sum of two products, each with the bound of a product, |W2| e_t1 + gamma(n) |W2| (|t1| +
    e_t1)  and  |V2| e_h1 + gamma(n) (|V2| (|h1| + e_h1) + |vb2|); the device adds both into one accumulator, so a term may
    pass through the roundings of both chains and n = 2 x 64 + 1 for each.  t2 and ty = W3 t2 + V3 h2 + vb3 likewise;
  * dy = ty / (std std) carries two more roundings: e_ty / std^2 (1 + gamma(2)) + gamma(2) |dy|;
  * the backward pass and the sums over the rows are fit_oracle's (_back, _wgrad), divided by M;
  * out = F v + d v: three more roundings (d itself, the product, the sum), gamma(3) (|F v| + |d v|);
  * the log-std block is 2 v + d v, three roundings on the device; the bound admits an evaluation that forms it like every
    other entry, as the mean over the M rows of the second derivative 2 (std_old / std)^2 v of the row's KL term: four
    roundings for the term, M + 3 for the sum and the division as in _wgrad, three for the damping: gamma(M + 10);
  * everything is multiplied ONCE by fit_oracle's SAFETY = 2 for the matrix cores.
`scale`, what a float64 evaluation is measured against (1e-12 scale + 1e-14), is the same pass on absolute values.

The bound means nothing within a forward error of a relu kink, so `fvp` counts the rows with a pre-activation within its forward
bound of 0 (`kinks`); the cases are generated so that the count is zero, and `case` asserts it.
"""
import math

import numpy as np

import evaluate_oracle as eo
import fit_oracle as fo
from fit_oracle import SAFETY, U32, _act_prime, _back, _kink, _units, _wgrad, forward, gamma

NAMES = fo.NAMES + ('log_std',)


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def shapes(n_in, n_out):
    return (('W1', (64, n_in)), ('b1', (64,)), ('W2', (64, 64)), ('b2', (64,)), ('W3', (n_out, 64)), ('b3', (n_out,)),
            ('log_std', (n_out,)))


def size(n_in, n_out):
    return sum(int(np.prod(s)) for _, s in shapes(n_in, n_out))


def split(flat, n_in, n_out):
    """A flat direction -> {name: array}, views."""
    out, o = {}, 0
    for name, shape in shapes(n_in, n_out):
        n = int(np.prod(shape))
        out[name] = flat[o:o + n].reshape(shape)
        o += n
    assert o == flat.shape[0]
    return out


def join(parts):
    return np.concatenate([np.asarray(parts[k]).reshape(-1) for k in NAMES])


def _two_products(W, t, e_t, V, h, e_h, vb):
    """W t + V h + vb for t, h [M, in] -> (value, bound, scale): one accumulator for both products."""
    aW, aV = np.abs(W), np.abs(V)
    n = W.shape[1] + V.shape[1] + 1
    val = t @ W.T + h @ V.T + vb
    e = e_t @ aW.T + e_h @ aV.T + gamma(n) * ((np.abs(t) + e_t) @ aW.T + (np.abs(h) + e_h) @ aV.T + np.abs(vb))
    return val, e


def _times(p, e_p, ap, e_ap):
    val = p * ap
    return val, e_p * np.abs(ap) + np.abs(p) * e_ap + e_p * e_ap + gamma(1) * np.abs(val)


MISTAKES = ('V2 transposed', "act'(a2) dropped from the tangent", 'std in place of std^2')


def fvp(net, std, x, v, damping=0.0, idx=None, mistake=None, exempt=None):
    """The call of atacom_trust_fvp on rows x [R, n_in] (gathered through idx, if given), direction v [P + n_out] -> dict:
    flat, bound, scale [P + n_out] in the library's order (bound: float32, per element; scale: the pass on absolute values);
    kinks: the number of rows the bound does not cover (module docstring).  `mistake`: one of MISTAKES, made on purpose -- what
    a wrong device would return, for the tests that show that the bound and the norm rule catch it.
    exempt: the engineered (layer, unit) pairs of tests/edge_cases.py, left out of `kinks`; nothing else is.
    mistake='kink_open': the gate of those units reads h >= 0, in the tangent and in the backward pass."""
    assert mistake is None or mistake in MISTAKES or mistake == 'kink_open'
    x, s, v = _f64(x), _f64(std), _f64(v)
    act = net.get('activation', 'relu')
    if idx is not None:
        x = x[np.asarray(idx)]
    M = x.shape[0]
    W1, W2, W3 = _f64(net['W1']), _f64(net['W2']), _f64(net['W3'])
    n_in, n_out = W1.shape[1], W3.shape[0]
    d = split(v, n_in, n_out)
    if mistake == MISTAKES[0]:
        d = dict(d, W2=d['W2'].T)
    f = forward(net, x)
    kink = np.zeros(M, bool)
    if act == 'relu':
        kink |= _kink(f['a1'], f['e_a1'], exempt, 1, SAFETY) | _kink(f['a2'], f['e_a2'], exempt, 2, SAFETY)
    opn = exempt if mistake == 'kink_open' else None
    ap1, e_ap1 = _act_prime(f['h1'], f['e_h1'], act, _units(opn, 1))
    ap2, e_ap2 = _act_prime(f['h2'], f['e_h2'], act, _units(opn, 2))
    tp2 = np.ones_like(ap2) if mistake == MISTAKES[1] else ap2
    # ---- tangent
    n1 = 4 * ((n_in + 3) // 4)
    aV1 = np.abs(d['W1'])
    p1 = f['xn'] @ d['W1'].T + d['b1']
    e_p1 = f['e_xn'] @ aV1.T + gamma(n1 + 1) * ((np.abs(f['xn']) + f['e_xn']) @ aV1.T + np.abs(d['b1']))
    t1, e_t1 = _times(p1, e_p1, ap1, e_ap1)
    p2, e_p2 = _two_products(W2, t1, e_t1, d['W2'], f['h1'], f['e_h1'], d['b2'])
    t2, e_t2 = _times(p2, e_p2, tp2, e_ap2)
    ty, e_ty = _two_products(W3, t2, e_t2, d['W3'], f['h2'], f['e_h2'], d['b3'])
    s2 = s if mistake == MISTAKES[2] else s * s
    dy = ty / s2
    e_dy = (e_ty / s2) * (1.0 + gamma(2)) + gamma(2) * np.abs(dy)
    # the same pass on absolute values
    S_t1 = (np.abs(f['xn']) @ aV1.T + np.abs(d['b1'])) * np.abs(ap1)
    S_t2 = (S_t1 @ np.abs(W2).T + np.abs(f['h1']) @ np.abs(d['W2']).T + np.abs(d['b2'])) * np.abs(ap2)
    S_dy = (S_t2 @ np.abs(W3).T + np.abs(f['h2']) @ np.abs(d['W3']).T + np.abs(d['b3'])) / s2
    # ---- backward: fit_oracle's, with the same pass on absolute values next to it
    A_dy = np.abs(dy)
    da2, e_da2 = _back(W3, dy, e_dy, ap2, e_ap2, 8)
    A_da2 = (A_dy @ np.abs(W3)) * np.abs(ap2)
    S_da2 = (S_dy @ np.abs(W3)) * np.abs(ap2)
    da1, e_da1 = _back(W2, da2, e_da2, ap1, e_ap1, 64)
    A_da1 = (A_da2 @ np.abs(W2)) * np.abs(ap1)
    S_da1 = (S_da2 @ np.abs(W2)) * np.abs(ap1)
    one, zero = np.ones((M, 1)), np.zeros((M, 1))
    parts = {}
    for name, bias, (dl, e_dl, A_dl, S_dl), (h, e_h) in (('W1', 'b1', (da1, e_da1, A_da1, S_da1), (f['xn'], f['e_xn'])),
                                                          ('W2', 'b2', (da2, e_da2, A_da2, S_da2), (f['h1'], f['e_h1'])),
                                                          ('W3', 'b3', (dy, e_dy, A_dy, S_dy), (f['h2'], f['e_h2']))):
        parts[name] = _wgrad(dl, e_dl, A_dl, S_dl, h, e_h, M)
        parts[bias] = tuple(a[:, 0] for a in _wgrad(dl, e_dl, A_dl, S_dl, one, zero, M))
    val, bound, scale = {}, {}, {}
    for k in fo.NAMES:
        Fv, e, sc = (a / M for a in parts[k])
        dv = damping * d[k]
        val[k] = Fv + dv
        bound[k] = SAFETY * (e + gamma(3) * (np.abs(Fv) + np.abs(dv)))
        scale[k] = sc + np.abs(dv)
    ls = d['log_std']
    val['log_std'] = 2.0 * ls + damping * ls
    scale['log_std'] = 2.0 * np.abs(ls) + np.abs(damping * ls)
    bound['log_std'] = SAFETY * gamma(M + 10) * scale['log_std']
    return dict(flat=join(val), bound=join(bound), scale=join(scale), kinks=int(kink.sum()))


def cg(matvec, g, iters=10, tol=1e-10):
    """MushroomRL's TRPO._conjugate_gradient, in the dtype of g -> (x, the squared residual, iterations run, the squared
    residual after each of them)."""
    x = np.zeros_like(g)
    r, p = g.copy(), g.copy()
    r2 = r.dot(r)
    n, hist = 0, []
    for _ in range(iters):
        z = matvec(p)
        a = r2 / p.dot(z)
        x = x + a * p
        r = r - a * z
        r2n = r.dot(r)
        p = r + (r2n / r2) * p
        r2 = r2n
        n += 1
        hist.append(float(r2))
        if r2 < tol:
            break
    return x, r2, n, hist


def cg_reference(c, iters=10, tol=1e-10, draws=8):
    """The natural gradient of a case (right-hand side: its `rhs`) by the float64 oracle -> dict: x, r2, n, hist;
    r: the oracle loop's own response to relative perturbations of 1e-12 of its matrix-vector products (`draws` draws, elementwise
       maximum of |x' - x|): the conditioning-aware allowance of a float64 device, as in tests/test_gpu_arm_limits.py;
    r32: ||x32 - x||inf of a NUMPY FLOAT32 run of the same loop on the float32-rounded oracle product: the allowance of a float32
       device, computed from the reference alone.  ONE number, not a vector: a single float32 run is one draw of the rounding
       errors, and where its deviation happens to vanish in an element says nothing about another float32 evaluation's there;
       its size does.  (profiles/trust.md records r32 / ||x||inf.)"""
    mv = lambda p: fvp(c['net'], c['std'], c['x'], p, c['damping'])['flat']                       # noqa: E731
    g = _f64(c['rhs'])
    x, r2, n, hist = cg(mv, g, iters, tol)
    rng = np.random.default_rng(1234)
    r = np.zeros_like(x)
    for _ in range(draws):
        def noisy(p):
            z = mv(p)
            return z * (1.0 + 1e-12 * rng.standard_normal(z.shape))
        r = np.maximum(r, np.abs(cg(noisy, g, iters, tol)[0] - x))
    x32 = cg(lambda p: mv(p.astype(np.float64)).astype(np.float32), g.astype(np.float32), iters, np.float32(tol))[0]
    return dict(x=x, r2=r2, n=n, hist=hist, r=r, r32=float(np.abs(x32.astype(np.float64) - x).max()))


# ---- the cases of tests/test_gpu_trust.py, shared with tests/test_trust_oracle.py
SHAPE_CASES = fo.SHAPE_CASES
ROW_CASES = fo.ROW_CASES
ROW_SHAPE = (18, 5, 'relu', True)
DAMPING = 1e-2
CASES = [(500 + i,) + c for i, c in enumerate(SHAPE_CASES)] + [(600 + r,) + ROW_SHAPE + (r,) for r in sorted({r for r, _ in ROW_CASES})]


def direction(rng, net, n_out, dtype):
    """N(0, 1) scaled per tensor by the weight's own magnitude (its root mean square); the log-std part by 1."""
    parts = {k: rng.normal(0.0, 1.0, np.shape(net[k])) * math.sqrt(float(np.mean(_f64(net[k]) ** 2))) for k in fo.NAMES}
    parts['log_std'] = rng.normal(0.0, 1.0, n_out)
    return join(parts).astype(dtype)


def case(seed, n_in, n_out, activation, normalise, rows, dtype=np.float32, check=True, edge=None, damping=DAMPING):
    """A case in `dtype`: dict(net, x, std, v, g, damping, want).  net, x and std are evaluate_oracle.case_data's (std
    log-uniform in [1e-2, 2]); v and g are two directions.  The seed is moved on, deterministically, until no row sits at a relu
    kink: zero exclusions, asserted.  edge: a construction of tests/edge_cases.py, edge(net, x) -> the engineered (layer, unit)
    pairs; it changes net and x in place, the directions are drawn before it from the network as drawn (so that they are not
    zero on the engineered rows), and its units alone are left out of the count (c['exempt'])."""
    exempt = None
    for attempt in range(64):
        s = seed + 1000 * attempt
        net, x, _, std = eo.case_data(s, n_in, n_out, activation, normalise, rows, dtype)
        rng = np.random.default_rng(s + 99)
        v, g = direction(rng, net, n_out, dtype), direction(rng, net, n_out, dtype)
        if edge is not None:
            exempt = edge(net, x)
        want = fvp(net, std, x, v, damping, exempt=exempt)
        if want['kinks'] == 0:
            break
    if check:
        assert want['kinks'] == 0, 'no seed without a row at a kink'
    # the right-hand side of the conjugate-gradient tests: (F + damping I) g, a vector the first iterations make progress on
    rhs = fvp(net, std, x, g, damping)['flat'].astype(dtype)
    return dict(net=net, x=x, std=std, v=v, g=g, rhs=rhs, damping=damping, want=want, n_in=n_in, n_out=n_out, exempt=exempt)


# ---- the TRPO policy step
def _theta(net, log_std):
    return join(dict({k: _f64(net[k]) for k in fo.NAMES}, log_std=_f64(log_std)))


def _net_of(net, theta, n_in, n_out):
    p = split(theta, n_in, n_out)
    out = dict(net)
    out.update({k: p[k] for k in fo.NAMES})
    return out, p['log_std']


def surrogate_and_kl(c, theta, old=None, ent_coeff=0.0):
    """L = mean rho A + ent_coeff H and the mean KL(old || theta) of a TRPO case at parameters theta -> (L, e_L, kl, e_kl): the
    values in float64 and the float32 forward bounds of an evaluation that forms logp and the mean as libatacom_evaluate.so
    does (evaluate_oracle.log_prob) and the rest by elementwise float32 operations.  old = (mean_old, e_mean_old, std_old)."""
    n_in, n_out = c['n_in'], c['n_out']
    net, log_std = _net_of(c['net'], theta, n_in, n_out)
    std = np.exp(log_std)
    A, lpo = _f64(c['adv']), _f64(c['logp_old'])
    M = A.shape[0]
    logp, e_lp, _, y, e_y = eo.log_prob(net, c['x'], c['action'], std)
    arg = logp - lpo
    e_arg = e_lp + U32 * np.abs(arg)
    rho = np.exp(arg)
    e_rho = rho * (np.expm1(e_arg) + gamma(4) * np.exp(e_arg))
    H = log_std.sum() + 0.5 * n_out * (1.0 + eo.LOG_2PI)
    L = (rho * A).mean() + ent_coeff * H
    e_L = (np.abs(A) * e_rho).mean() + gamma(M + 3) * np.abs(rho * A).mean() + gamma(n_out + 3) * abs(ent_coeff) * (np.abs(log_std).sum() + n_out * 1.5)
    if old is None:
        return L, e_L, 0.0, 0.0, (y, e_y, std)
    mo, e_mo, so = old
    # std = exp(log_std) formed in float32: the rounding of log_std's update is part of theta; exp adds a few units
    e_s = std * gamma(4)
    dm = mo - y
    e_dm = e_mo + e_y + U32 * np.abs(dm)
    q = (so * so + dm * dm) / (2.0 * std * std)
    terms = np.log(std / so) + q - 0.5
    e_terms = (2.0 * np.abs(dm) * e_dm + e_dm * e_dm) / (2.0 * std * std) + gamma(6) * (np.abs(np.log(std / so)) + q + 0.5) \
        + (e_s / std) * (1.0 + 2.0 * q)
    kl = terms.sum(-1).mean()
    e_kl = e_terms.sum(-1).mean() + gamma(M + n_out + 3) * (np.abs(np.log(std / so)) + q + 0.5).sum(-1).mean()
    return L, e_L, kl, e_kl, (y, e_y, std)


def trpo(c, max_kl=1e-2, ent_coeff=0.0, cg_iters=10, cg_damping=1e-2, cg_residual_tol=1e-10, line_search=10):
    """MushroomRL's TRPO policy step on a case dict(net, log_std, x, action, adv, logp_old, n_in, n_out), line by line -> dict:
    g, x (the natural gradient), shs, full, theta_old, theta (the final parameters), halvings, accepted, loss_old, loss_new, kl,
    cg_residual and `candidates`: per tried j (kl - 1.5 max_kl, its float32 bound, improve, its float32 bound)."""
    n_in, n_out = c['n_in'], c['n_out']
    net, log_std = c['net'], _f64(c['log_std'])
    std = np.exp(log_std)
    grad = fo.gradient(net, c['x'], fo.PPO_CLIP, c['adv'], c['action'], std, c['logp_old'], clip=1e30)
    g = -grad['flat']
    g[-n_out:] += ent_coeff
    x, r2, _, _ = cg(lambda p: fvp(net, std, c['x'], p, cg_damping)['flat'], g, cg_iters, cg_residual_tol)
    shs = 0.5 * x.dot(fvp(net, std, c['x'], x, cg_damping)['flat'])
    full = x / math.sqrt(shs / max_kl)
    theta_old = _theta(net, log_std)
    loss_old, e_old, _, _, old = surrogate_and_kl(c, theta_old, None, ent_coeff)
    out = dict(g=g, x=x, shs=shs, full=full, theta_old=theta_old, theta=theta_old, halvings=line_search, accepted=False,
               loss_old=loss_old, loss_new=loss_old, kl=0.0, cg_residual=r2, candidates=[])
    for j in range(line_search):
        theta = theta_old + full * 0.5 ** j
        loss, e_new, kl, e_kl, _ = surrogate_and_kl(c, theta, old, ent_coeff)
        improve = loss - loss_old
        out['candidates'].append((kl - 1.5 * max_kl, e_kl, improve, e_new + e_old))
        if kl <= 1.5 * max_kl and improve >= 0.0:
            out.update(theta=theta, halvings=j, accepted=True, loss_new=loss, kl=kl)
            break
    return out


def step_allowance(c, w, float32, cg_damping=1e-2, iters=10, tol=1e-10, draws=8):
    """What the full step `full` = x / sqrt(shs / max_kl) of a TRPO case may deviate by, elementwise: the natural_gradient rule
    (cg_reference) carried to the step, 1e-8 ||full||inf + 4 r, computed from the reference alone.
    float64: r = the elementwise response of the oracle's full step to relative perturbations of 1e-12 of its products.
    float32: r = ||full32 - full||inf of a float32 REFERENCE run of the chain that leads to the step -- g by torch's float32
    autograd of the surrogate on the CPU (the device's g is a float32 evaluation too, and the solve amplifies its rounding like
    any other), the loop in numpy float32 on the float32-rounded oracle product, shs and the division in float32."""
    std = np.exp(_f64(c['log_std']))
    mv = lambda p: fvp(c['net'], std, c['x'], p, cg_damping)['flat']                              # noqa: E731
    full = w['full']
    floor = 1e-8 * np.abs(full).max()
    if not float32:
        rng = np.random.default_rng(4321)
        r = np.zeros_like(full)
        for _ in range(draws):
            noisy = lambda p: mv(p) * (1.0 + 1e-12 * rng.standard_normal(p.shape))                # noqa: E731
            x = cg(noisy, w['g'], iters, tol)[0]
            r = np.maximum(r, np.abs(x / math.sqrt(0.5 * x.dot(noisy(x)) / c['max_kl']) - full))
        return floor + 4.0 * r
    import torch
    t = lambda a: None if a is None else torch.tensor(np.asarray(a, dtype=np.float32))            # noqa: E731
    net = c['net']
    P = [t(net[k]).requires_grad_() for k in fo.NAMES] + [t(c['log_std']).requires_grad_()]
    sh, sc = t(net['obs_shift']), t(net['obs_scale'])
    xn = t(c['x']) if sh is None else (t(c['x']) - sh) * sc
    f = torch.relu if net['activation'] == 'relu' else torch.tanh
    mu = f(f(xn @ P[0].T + P[1]) @ P[2].T + P[3]) @ P[4].T + P[5]
    logp = (-0.5 * ((t(c['action']) - mu) / P[6].exp()) ** 2 - P[6]).sum(-1) - 0.5 * c['n_out'] * eo.LOG_2PI
    loss = ((logp - t(c['logp_old'])).exp() * t(c['adv'])).mean() + c['ent_coeff'] * P[6].sum()
    g32 = torch.cat([a.reshape(-1) for a in torch.autograd.grad(loss, P)]).numpy()
    mv32 = lambda p: mv(p.astype(np.float64)).astype(np.float32)                                  # noqa: E731
    x32 = cg(mv32, g32, iters, np.float32(tol))[0]
    full32 = x32 / np.sqrt(np.float32(0.5) * x32.dot(mv32(x32)) / np.float32(c['max_kl']))
    assert full32.dtype == np.float32
    return floor + 4.0 * np.full_like(full, np.abs(full32.astype(np.float64) - full).max())


TRPO_SHAPE = (18, 5, 'relu', True, 200)
# seed, rows with a big advantage, max_kl, tries of the line search.  The float32 forward bounds of the KL divergence and of the
# surrogate are worst cases of about 1e-3 of max_kl = 1e-2, so a margin of 100 bounds asks for larger steps than the default:
# max_kl = 0.5 and 2.  The seeds were chosen on the oracle's own margins (tests/test_trust_oracle.py asserts them).
TRPO_CASES = {'a': dict(seed=701, big=0, max_kl=0.5, line_search=10), 'b': dict(seed=740, big=6, max_kl=2.0, line_search=10),
              'c': dict(seed=740, big=6, max_kl=2.0, line_search=2)}
BIG_ADVANTAGE = 200.0
BIG_Z = 0.4
ENT_COEFF = 5e-5


def trpo_case(name, dtype=np.float32):
    """The three line-search cases: 200 rows of the (18, 5) relu policy, std in [0.7, 1], actions drawn from the policy,
    logp_old the policy's own log-probability (rho = 1 at theta_old), advantages N(0, 1).  `big` rows carry an advantage of
    BIG_ADVANTAGE and an action BIG_Z of a draw away from the mean: the gradient is theirs, the full step overshoots their actions
    and is refused.  (a): accepted at j = 0; (b): after 2 to 4 halvings; (c): (b) with line_search = 2, nothing accepted."""
    spec = TRPO_CASES[name]
    n_in, n_out, act, norm, rows = TRPO_SHAPE
    net, x, _, _ = eo.case_data(spec['seed'], n_in, n_out, act, norm, rows, dtype)
    rng = np.random.default_rng(spec['seed'] + 55)
    log_std = rng.uniform(math.log(0.7), 0.0, n_out).astype(dtype)
    std = np.exp(_f64(log_std))
    y = forward(net, x)['y']
    z = rng.normal(0.0, 1.0, (rows, n_out))
    z[:spec['big']] *= BIG_Z
    action = (y + std * z).astype(dtype)
    logp_old = eo.log_prob(net, x, action, std)[0].astype(dtype)
    adv = rng.normal(0.0, 1.0, rows)
    adv[:spec['big']] = BIG_ADVANTAGE
    c = dict(net=net, log_std=log_std, x=x, action=action, adv=adv.astype(dtype), logp_old=logp_old, n_in=n_in, n_out=n_out,
             line_search=spec['line_search'], max_kl=spec['max_kl'], ent_coeff=ENT_COEFF)
    c['want'] = trpo(c, max_kl=c['max_kl'], ent_coeff=ENT_COEFF, line_search=spec['line_search'])
    return c
