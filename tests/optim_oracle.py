"""The oracle of libatacom_optim.so (include/atacom_optim_hip.h): the Adam step restated in numpy float64 (step64) and, in the
same order of operations, in numpy float32 (step32); the absolute bound on what a float32 implementation of that order may
differ from the float64 result by when both start from the same float32 inputs (bound32; derived in DESIGN.md section 7d); and
the inputs of the GPU tests (case), which tests/test_optim_oracle.py checks the float32 restatement against on the CPU.  A helper
module: it holds no test.

A group is handled as ONE flat vector of N values in the order of its gradient (W1, b1, W2, b2, W3, b3, then log std): the
arithmetic is elementwise and the layout is the tests' concern."""
import numpy as np

BETAS, EPS, LR = (0.9, 0.999), 1e-8, 3e-4
# (n_in, n_out, has log_std and std): N = 4353, 5889, 5962, 6800
SHAPES = ((1, 1, False), (25, 1, False), (18, 5, True), (32, 8, True))
STEPS = (1, 2, 10, 1000)                    # the t of the teacher-forced single steps
U = 2.0 ** -24                              # unit roundoff of float32
TINY = 2.0 ** -149                          # an operation that underflows is off by at most this much more
EXP_ULPS = 1.0                              # documented maximum error of the device's expf (HIP math API), in ulps


def group_size(n_in, n_out, has_log_std):
    return 64 * n_in + 64 + 4096 + 64 + 64 * n_out + n_out + (n_out if has_log_std else 0)


def segments(n_in, n_out, has_log_std):
    """[(name, shape)] in the order of the flat vector."""
    out = [('W1', (64, n_in)), ('b1', (64,)), ('W2', (64, 64)), ('b2', (64,)), ('W3', (n_out, 64)), ('b3', (n_out,))]
    return out + ([('log_std', (n_out,))] if has_log_std else [])


def scale_of(shape):
    """The example's loss is  policy + 0.5 value : a one-output network without log std is a critic."""
    return 0.5 if not shape[2] else 1.0


def fresh_head():
    return (0, 1.0, 1.0)


def head_at(t, betas=BETAS):
    """The head BEFORE step t: step = t - 1 and the running products of t - 1 factors (float64, in order)."""
    b1p = b2p = 1.0
    for _ in range(t - 1):
        b1p *= betas[0]
        b2p *= betas[1]
    return (t - 1, b1p, b2p)


def _scalars(head, lr, betas):
    step, b1p, b2p = head
    b1p, b2p = b1p * betas[0], b2p * betas[1]
    return (step + 1, b1p, b2p), lr / (1.0 - b1p), np.sqrt(1.0 - b2p)


def step64(p, grad, m, v, head, lr=LR, scale=1.0, betas=BETAS, eps=EPS, n_std=0):
    """One step in float64 -> dict(p, m, v, head, std (the exp of the last n_std parameters), and the intermediates the bound
    and the scales are made of)."""
    p, grad, m, v = (np.asarray(a, dtype=np.float64) for a in (p, grad, m, v))
    new_head, step_size, bc2s = _scalars(head, lr, betas)
    g = scale * grad
    mn = m + (g - m) * (1.0 - betas[0])
    vn = betas[1] * v + ((1.0 - betas[1]) * g) * g
    den = np.sqrt(vn) / bc2s + eps
    r = mn / den
    pn = p - step_size * r
    std = np.exp(pn[len(pn) - n_std:]) if n_std else np.zeros(0)
    return dict(p=pn, m=mn, v=vn, head=new_head, std=std, g=g, den=den, r=r, step_size=step_size, bc2s=bc2s,
                scale=dict(p=np.abs(p) + step_size * np.abs(r), m=np.abs(m) + np.abs(g), v=vn, std=std))


def step32(p, grad, m, v, head, lr=LR, scale=1.0, betas=BETAS, eps=EPS, n_std=0):
    """The same step with every elementwise operation an individually rounded float32 one, in the header's order; the head
    and the scalars are formed in float64 and rounded once."""
    f = np.float32
    p, grad, m, v = (np.asarray(a, dtype=f) for a in (p, grad, m, v))
    new_head, step_size, bc2s = _scalars(head, lr, betas)
    step_size, bc2s, omb1, beta2, omb2, eps, scale = (f(x) for x in (step_size, bc2s, 1.0 - betas[0], betas[1], 1.0 - betas[1], eps, scale))
    g = scale * grad
    mn = m + (g - m) * omb1
    vn = beta2 * v + (omb2 * g) * g
    pn = p - step_size * (mn / (np.sqrt(vn) / bc2s + eps))
    for a in (g, mn, vn, pn):
        assert a.dtype == f
    std = np.exp(pn[len(pn) - n_std:]) if n_std else np.zeros(0, dtype=f)
    return dict(p=pn, m=mn, v=vn, head=new_head, std=std)


def gam(k):
    """(1 + u)^k - 1 <= gam(k): the usual bound on k accumulated relative roundings."""
    return k * U / (1.0 - k * U)


def bound32(p, grad, m, v, head, lr=LR, scale=1.0, betas=BETAS, eps=EPS, n_std=0):
    """|float32 result - step64 result| <= this, elementwise, for p, m, v and std, when both start from the float32 values
    p, grad, m, v and the float32 side rounds each scalar once and each operation once (DESIGN.md section 7d walks through it).
    Absolute: where sqrt(v) / bc2s is below eps the eps term carries the denominator, and the cancellation in g - m is charged
    to |g| + |m|, not to the difference."""
    o = step64(p, grad, m, v, head, lr, scale, betas, eps, n_std)
    p, grad, m, v = (np.asarray(a, dtype=np.float64) for a in (p, grad, m, v))
    g, mn, vn, den, r, pn, step_size, bc2s = o['g'], o['m'], o['v'], o['den'], o['r'], o['p'], o['step_size'], o['bc2s']
    omb1, b2, omb2 = 1.0 - betas[0], betas[1], 1.0 - betas[1]
    ag, am = np.abs(g), np.abs(m)
    # g^ = fl(scale^ grad): two roundings.  d^ = fl(g^ - m): the error of g^, and one rounding of a difference of size <= |g^| + |m|
    e_d = gam(4) * ag + gam(2) * am + TINY
    # e^ = fl(d^ omb1^): the carried error, the rounding of omb1 and of the product
    e_e = omb1 * (e_d * (1 + gam(2)) + gam(2) * (ag + am)) + TINY
    e_m = e_e * (1 + gam(1)) + gam(1) * np.abs(mn) + TINY
    # v: fl(beta2^ v) has two roundings; fl(fl(omb2^ g^) g^) has omb2's, g^'s two twice, and two products' = 7; then the sum's
    e_v = (gam(2) * b2 * v + gam(7) * omb2 * g * g) * (1 + gam(1)) + gam(1) * vn + 3 * TINY * (1 + ag)
    sq = np.sqrt(vn)
    with np.errstate(divide='ignore', invalid='ignore'):
        e_sq = np.where(sq > 0, np.minimum(np.sqrt(e_v), e_v / np.where(sq > 0, sq, 1.0)), np.sqrt(e_v))
    e_sq = e_sq + U * (sq + e_sq)
    q = sq / bc2s
    e_q = (e_sq / bc2s) * (1 + gam(2)) + gam(2) * q + TINY
    e_den = (e_q + U * eps) * (1 + gam(1)) + gam(1) * den
    den_lo = den - e_den
    assert (den_lo > 0).all()
    e_r = (e_m / den_lo + np.abs(mn) * e_den / (den * den_lo)) * (1 + gam(1)) + gam(1) * np.abs(r) + TINY
    e_w = step_size * e_r * (1 + gam(2)) + gam(2) * step_size * np.abs(r) + TINY
    e_p = e_w * (1 + gam(1)) + gam(1) * np.abs(pn) + TINY
    e_l = e_p[len(e_p) - n_std:] if n_std else np.zeros(0)
    # std: exp of a log std that is off by e_l, and the device's exp, which is off by EXP_ULPS ulps (one ulp <= 2 u |value|)
    e_std = o['std'] * (np.expm1(e_l) + EXP_ULPS * 2 * U * np.exp(e_l)) + TINY
    return dict(p=e_p, m=e_m, v=e_v, std=e_std)


def gradients(rng, n):
    """Magnitudes log-uniform over 1e-12 .. 1e3, random signs, every sixteenth value exactly zero."""
    g = 10.0 ** rng.uniform(-12.0, 3.0, n) * rng.choice([-1.0, 1.0], n)
    g[::16] = 0.0
    return g


_hist = {}


def _history(shape):
    """{t: (p, m, v) in float64 BEFORE step t} for t in STEPS, from 999 oracle steps on gradients whose magnitudes stay each
    value's own (so m and v are the moments such gradients leave) -- made once per shape."""
    if shape not in _hist:
        N = group_size(*shape)
        rng = np.random.default_rng(1000 + N)
        p = rng.normal(0.0, 0.3, N)
        if shape[2]:
            p[N - shape[1]:] = rng.uniform(-1.5, 0.3, shape[1])       # log std
        base = gradients(rng, N)
        m, v, head, out = np.zeros(N), np.zeros(N), fresh_head(), {}
        for t in range(1, max(STEPS) + 1):
            if t in STEPS:
                assert head == head_at(t)
                out[t] = (p.copy(), m.copy(), v.copy())
            o = step64(p, base * rng.uniform(-0.5, 1.5, N), m, v, head, scale=scale_of(shape))
            p, m, v, head = o['p'], o['m'], o['v'], o['head']
        _hist[shape] = out
    return _hist[shape]


_cases = {}


def case(shape, t, dtype):
    """The inputs of one teacher-forced step and what the oracle makes of them: dict(p, grad, m, v in `dtype`, head, scale,
    n_std, want = step64 from those values, bound = bound32 (float32) or None)."""
    key = (shape, t, np.dtype(dtype).name)
    if key not in _cases:
        N = group_size(*shape)
        p, m, v = (a.astype(dtype) for a in _history(shape)[t])
        grad = gradients(np.random.default_rng(7 * N + t), N).astype(dtype)
        kw = dict(head=head_at(t), scale=scale_of(shape), n_std=shape[1] if shape[2] else 0)
        c = dict(p=p, grad=grad, m=m, v=v, shape=shape, **kw)
        c['want'] = step64(p, grad, m, v, **kw)
        c['bound'] = bound32(p, grad, m, v, **kw) if np.dtype(dtype) == np.float32 else None
        _cases[key] = c
    return _cases[key]


def inside(dtype, got, c, what=''):
    """got: dict(p, m, v, std) -> the worst |error| / bound; float32 inside bound32 on every element, float64 inside
    1e-12 scale + 1e-14.  Raises AssertionError."""
    worst = 0.0
    for k in ('p', 'm', 'v', 'std'):
        ref = c['want'][k]
        if ref.size == 0:
            continue
        a = np.asarray(got[k], dtype=np.float64).reshape(-1)
        assert a.shape == ref.shape and np.isfinite(a).all(), (what, k)
        bound = c['bound'][k] if np.dtype(dtype) == np.float32 else 1e-12 * c['want']['scale'][k] + 1e-14
        err = np.abs(a - ref)
        w = float((err / bound).max())
        print('%s %s %s: worst |error| / bound %.4g, worst |error| %.3g' % (what, np.dtype(dtype).name, k, w, err.max()))
        assert (err <= bound).all(), (what, k, 'worst |error| / bound %.3g on %d of %d' % (w, int((err > bound).sum()), err.size))
        worst = max(worst, w)
    return worst
