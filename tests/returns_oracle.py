"""Float64 restatement of what libatacom_returns.so computes (include/atacom_returns_hip.h; test infrastructure only): the
advantage recurrence, PPO's normalisation and the episode returns, each as loops over a flat MushroomRL-shaped dataset and in a
vectorised form, with the forward error bounds the device results are held to.

UNPINNED: MushroomRL is not available to this project's tests, so `compute_gae` (mushroom_rl/utils/value_functions.py), `compute_J`
(mushroom_rl/utils/dataset.py) and PPO's `(adv - mean) / (std + 1e-8)` are restated from its published 1.x source, not checked
against an installed copy (the status tests/policy_explore_oracle.py gives its noise processes).

The recurrence, per environment, for t = T-1 ... 0 with A[T] = 0:

    vn     = 0 if absorbing[t] else v_next[t]        (a select: v_next may be NaN / Inf there)
    d      = (reward[t] + gamma * vn) - v[t]
    A[t]   = d + (gamma * lam) * (0 if last[t] else A[t+1])
    ret[t] = A[t] + v[t]

which is compute_gae wherever absorbing implies last (`gae_mushroom_flat` below is the literal form, for that comparison).

Contraction: the kernels use EXPLICIT fused multiply-adds -- d = fma(gamma, vn, reward) - v, A = fma(gamma lam, carry, d),
j = fma(p, reward, j) -- and compile everything else with contraction off; gamma * lam is formed once in the call's dtype.  That
is three roundings where a term is formed and one for every step it travels, inside the four and two the bound below allows.
`gae_in_dtype` / `episodes_in_dtype` run those operations in numpy: in float32 the fused multiply-add is the float64 product (exact)
and sum rounded to float32 (a second rounding that differs from the fused one only at an exact float32 midpoint); in float64 numpy
has no fused operation and multiplies, then adds -- one more rounding of 2^-53 per fma, far inside every bound used here.
"""
import numpy as np

EPS = {np.dtype('float32'): 2.0 ** -24, np.dtype('float64'): 2.0 ** -53, 'f32': 2.0 ** -24, 'f64': 2.0 ** -53}


# ------------------------------------------------------------------ flat datasets (MushroomRL's shape)
def flatten(x):
    """[T, B] -> flat, environment by environment (rollout.to_mushroom_dataset's order)."""
    return np.ascontiguousarray(np.asarray(x).T).reshape(-1)


def flat_last(last):
    """The `last` flags of the flat dataset: the final step of every environment's block closes its episode."""
    la = np.asarray(last, dtype=bool).copy()
    la[-1] = True
    return flatten(la)


def gae_loops(reward, absorbing, last, v, v_next, gamma, lam):
    """The recurrence above as one backward loop over the flat dataset of [T, B] arrays -> (ret, adv), [T, B] float64."""
    T, B = np.shape(reward)
    r, ab, la = flatten(reward).astype(np.float64), flatten(absorbing).astype(bool), flat_last(last)
    vv, vn = flatten(v).astype(np.float64), flatten(v_next).astype(np.float64)
    gl = gamma * lam
    adv = np.zeros(T * B)
    nxt = 0.0
    for k in reversed(range(T * B)):
        x = 0.0 if ab[k] else vn[k]
        d = (r[k] + gamma * x) - vv[k]
        adv[k] = d + gl * (0.0 if la[k] else nxt)
        nxt = adv[k]
    unflat = lambda z: z.reshape(B, T).T.copy()           # noqa: E731
    return unflat(adv + vv), unflat(adv)


def gae_mushroom_flat(r, absorbing, last, v, v_next, gamma, lam):
    """compute_gae of MushroomRL 1.x, literally, on flat arrays (its V(s), V(ss) already evaluated) -> (ret, adv)."""
    gen_adv = np.empty_like(v)
    for rev_k in range(len(v)):
        k = len(v) - rev_k - 1
        if last[k] or rev_k == 0:
            gen_adv[k] = r[k] - v[k]
            if not absorbing[k]:
                gen_adv[k] += gamma * v_next[k]
        else:
            gen_adv[k] = r[k] + gamma * v_next[k] - v[k] + gamma * lam * gen_adv[k + 1]
    return gen_adv + v, gen_adv


def episodes_loops(reward, last, gamma):
    """compute_J of MushroomRL 1.x on the flat dataset of [T, B] arrays -> the list of episode returns, in dataset order."""
    r, la = flatten(reward).astype(np.float64), flat_last(last)
    js, j, n = [], 0.0, 0
    for k in range(len(r)):
        j += gamma ** n * r[k]
        n += 1
        if la[k] or k == len(r) - 1:
            js.append(j)
            j, n = 0.0, 0
    return js


# ------------------------------------------------------------------ vectorised over the environments
def _fma(dt):
    """a * b + c as the kernels' fused multiply-add, as closely as numpy can (see the module's docstring)."""
    if dt is np.float32:
        return lambda a, b, c: (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
    return lambda a, b, c: a * b + c


def gae_in_dtype(reward, absorbing, last, v, v_next, gamma, lam, dtype=np.float64):
    """The recurrence on [T, B] (or [..., T, B] with T second to last) arrays, every operation in `dtype` and in the kernel's
    order -> (ret, adv) of that dtype.  v = v_next = None: zeros."""
    dt = np.dtype(dtype).type
    r = np.asarray(reward).astype(dt)
    ab, la = np.asarray(absorbing) > 0.5, np.asarray(last) > 0.5
    vv = np.zeros_like(r) if v is None else np.asarray(v).astype(dt)
    vn = np.zeros_like(r) if v_next is None else np.asarray(v_next).astype(dt)
    g = dt(gamma)
    gl = dt(g * dt(lam))
    fma = _fma(dt)
    T = r.shape[-2]
    adv, ret = np.empty_like(r), np.empty_like(r)
    carry = np.zeros_like(r[..., 0, :])
    zero = dt(0)
    with np.errstate(invalid='ignore', over='ignore'):
        for t in reversed(range(T)):
            x = np.where(ab[..., t, :], zero, vn[..., t, :])
            d = fma(g, x, r[..., t, :]) - vv[..., t, :]
            carry = fma(gl, np.where(la[..., t, :], zero, carry), d)
            adv[..., t, :] = carry
            ret[..., t, :] = carry + vv[..., t, :]
    return ret, adv


def gae(reward, absorbing, last, v, v_next, gamma, lam):
    """The float64 reference -> (ret, adv)."""
    return gae_in_dtype(reward, absorbing, last, v, v_next, gamma, lam, np.float64)


def gae_bound(reward, absorbing, last, v, v_next, gamma, lam, eps):
    """The forward error of the recurrence in a format of unit roundoff eps -> (bound on ret, bound on adv), [..., T, B]:

        bound[t] = eps * sum over u >= t of the same episode of (2 (u - t) + 4) (gamma lam)^(u - t) m[u]
        m[u]     = |r[u]| + gamma |vn[u]| + |v[u]|

    four roundings where a term is formed plus two for every step it travels (the kernels' fused operations spend three and
    one); ret adds eps (|A| + |v|).  Evaluated by the
    recurrences S0[t] = m[t] + c S0[t+1], S1[t] = c (S1[t+1] + S0[t+1]) with c = gamma lam cut at `last`."""
    r = np.abs(np.asarray(reward, dtype=np.float64))
    ab, la = np.asarray(absorbing) > 0.5, np.asarray(last) > 0.5
    vv = np.zeros_like(r) if v is None else np.abs(np.asarray(v, dtype=np.float64))
    vn = np.zeros_like(r) if v_next is None else np.where(ab, 0.0, np.abs(np.asarray(v_next, dtype=np.float64)))
    m = r + gamma * vn + vv
    c = gamma * lam
    T = r.shape[-2]
    s0, s1 = np.zeros_like(r[..., 0, :]), np.zeros_like(r[..., 0, :])
    bound = np.empty_like(r)
    for t in reversed(range(T)):
        cont = np.where(la[..., t, :], 0.0, c)
        s1 = cont * (s1 + s0)
        s0 = m[..., t, :] + cont * s0
        bound[..., t, :] = eps * (2.0 * s1 + 4.0 * s0)
    _, a = gae(reward, absorbing, last, v, v_next, gamma, lam)
    return bound + eps * (np.abs(a) + vv), bound


def episodes_in_dtype(reward, last, gamma, dtype=np.float64):
    """The episode returns of [T, B] arrays, environment by environment, with the running product the kernel carries and every
    operation in `dtype` -> (list of j as float64, list of their bounds eps sum_u (u + 2) gamma^u |r[u]|)."""
    dt = np.dtype(dtype).type
    r = np.asarray(reward).astype(dt)
    la = np.asarray(last) > 0.5
    T, B = r.shape
    g, eps, fma = dt(gamma), EPS[np.dtype(dtype)], _fma(dt)
    js, bounds = [], []
    for b in range(B):
        j, p, bound, u = dt(0), dt(1), 0.0, 0
        for t in range(T):
            j = dt(fma(p, r[t, b], j))
            bound += (u + 2) * float(gamma) ** u * abs(float(r[t, b]))
            p = dt(p * g)
            u += 1
            if la[t, b] or t == T - 1:
                js.append(float(j))
                bounds.append(eps * bound)
                j, p, bound, u = dt(0), dt(1), 0.0, 0
    return js, bounds


def episode_sums(reward, last, gamma, sizes=None):
    """[sum of j, number of episodes, sum of j^2] over the real rows of [W, T, Bm] arrays, in float64, and the bound on the
    first: the per-episode bounds of a kernel in a format of unit roundoff `eps` are added by the caller."""
    r, la = np.asarray(reward, dtype=np.float64), np.asarray(last)
    W = r.shape[0]
    js = []
    for w in range(W):
        n = r.shape[2] if sizes is None else sizes[w]
        js += episodes_loops(r[w][:, :n], la[w][:, :n], gamma) if n else []
    js = np.asarray(js)
    return np.array([js.sum(), float(len(js)), (js * js).sum()]), js


def valid_rows(shape, sizes):
    """bool [W, T, Bm]: the real rows of ragged blocks."""
    W, T, Bm = shape
    m = np.arange(Bm)[None, :] < np.asarray(sizes if sizes is not None else [Bm] * W)[:, None]
    return np.broadcast_to(m[:, None, :], (W, T, Bm))


def normalize(adv, sizes=None):
    """PPO's (adv - mean) / (std + 1e-8) with the population std over the real rows of [W, T, Bm] -> (normalised, [count, mean,
    std]); padding rows are returned as they came."""
    a = np.asarray(adv, dtype=np.float64)
    m = valid_rows(a.shape, sizes)
    x = a[m]
    mean, std = x.mean(), x.std()
    return np.where(m, (a - mean) / (std + 1e-8), a), np.array([float(x.size), mean, std])


def stats_bound(adv, sizes=None):
    """How far mean and std of a sum / sum-of-squares accumulation in double (any order: n roundings of unit roundoff u = 2^-53
    at most on each sum) may lie from the exact ones -> (bound on mean, bound on std).  var = q / n - mean^2 inherits
    n u (E[x^2] + 2 |mean| E|x| + mean^2), and |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(b) as well as <= sqrt(|a - b|)."""
    a = np.asarray(adv, dtype=np.float64)
    x = a[valid_rows(a.shape, sizes)]
    n, u = x.size, 2.0 ** -53
    e_abs, e_sq, mean, std = np.abs(x).mean(), (x * x).mean(), x.mean(), x.std()
    d_mean = (n + 2) * u * e_abs
    d_var = (n + 4) * u * (e_sq + 2 * abs(mean) * e_abs + mean * mean)
    return d_mean, min(d_var / std if std > 0 else np.inf, np.sqrt(d_var)) + 2 * u * std
