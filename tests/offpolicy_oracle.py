"""Float64 restatement of what libatacom_offpolicy.so computes (include/atacom_offpolicy_hip.h; test infrastructure only): the
Q-value of the two-branch DDPG / TD3 critic, the fused TD target and the soft update, with the forward error bound a float32
evaluation is held to, per sample, and the case tables the CPU and GPU tests share.  A helper module: it holds no test.

PINNED: tests/test_offpolicy_oracle.py checks `critic_q` and `target` against modules composed from torch.nn.Linear and the
MushroomRL target expression written out in torch, both in float64, to 1e-12, and holds torch's own float32 evaluation to the
bound on every sample.

The float32 bound.  u = 2^-24, gamma(n) = n u / (1 - n u).  A layer's pre-activation a = W h + b,
computed in float32 in any order of summation, fused or not, from an input with elementwise error e, satisfies

    |a^ - a|  <=  |W| e  +  SAFETY gamma(n + 1) (|W| (|h| + e) + |b|)          n = the layer's inputs, padded to a multiple of 4

(evaluate_oracle.forward's recurrence; SAFETY = 2 because the matrix cores are not documented to round every partial sum to
nearest, and it multiplies the rounding of the layer alone: what the layer inherits, |W| e, is carried as it is).  This
placement DEPARTS from evaluate_oracle.forward, which multiplies the whole output bound by SAFETY, the input's gamma(2) and
the tanh's TANH_ABS included: a chopping adder doubles the unit roundoff of a layer's sums and of nothing else, so SAFETY
belongs on gamma(n + 1) alone, and the bound here is the tighter of the two to first order in u.
The activations are 1-Lipschitz, max(a, 0) is exact and the device's tanh adds TANH_ABS.  The chain of a target:

    input        xn = (x - shift) * scale                         e = gamma(2) |xn|
    actor        three layers                                     -> m, e_m
    squash       a' = s tanh(m)  (mean_mode 1; a' = m for 0)      e_a = |s| (e_m + TANH_ABS) + gamma(4) (|a'| + |n|)
                 -- the product, the noise product noise_std eps and the sum are four roundings of magnitudes <= |a'| + |n|;
    clamps       of the noise and of the action: 1-Lipschitz maps onto bounds that are exact in the dtype: they add nothing
    division     as = a'' / act_scale                             e_as = e_a / |act_scale| + gamma(2) |as|
    critic       layer 1 on xn (DDPG) or [xn | as] (TD3); layer 2 on [h1 | as] with [W2 | W2a], n = 64 + 4 ceil(k / 4); layer 3
    min          |min(a, b) - min(a^, b^)| <= max(e_a, e_b)
    target       y = r + g ((1 - ab) q)                           e_y = |g| (1 - ab) e_q + gamma(2) (|r| + |g q|)

Every step is Lipschitz, so the bound holds on every sample, the kinks of ReLU and of the clamps included.  The scalars
noise_std, noise_clip and gamma are rounded once to the dtype, as the device does, before anything is computed.  Float64 is
held to 1e-12 scale + 1e-14, scale being the magnitude sum of the output as in evaluate_oracle.
"""
import math

import numpy as np

from evaluate_oracle import SAFETY, TANH_ABS, gamma, random_net

DDPG, TD3 = 'ddpg', 'td3'


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _act(a, activation):
    return np.maximum(a, 0.0) if activation == 'relu' else np.tanh(a)


def _layer(h, e, W, b, n=None):
    """(a, e_a, mag) of a = W h + b from an input h with error e."""
    W, b = _f64(W), _f64(b)
    n = 4 * ((W.shape[1] + 3) // 4) if n is None else n
    aW = np.abs(W).T
    mag = np.abs(h) @ aW + np.abs(b)
    return h @ W.T + b, e @ aW + SAFETY * gamma(n + 1) * ((np.abs(h) + e) @ aW + np.abs(b)), mag


def _hidden(a, e, activation):
    return _act(a, activation), (e + TANH_ABS if activation == 'tanh' else e)


def _normalise(net, x):
    shift, scale = _f64(net.get('obs_shift')), _f64(net.get('obs_scale'))
    h = (_f64(x) - (0.0 if shift is None else shift)) * (1.0 if scale is None else scale)
    return h, gamma(2) * np.abs(h)


def mlp(net, x):
    """The plain 2 x 64 network (the actor) -> (y, e32, mag) with this module's recurrence."""
    act = net.get('activation', 'relu')
    h, e = _normalise(net, x)
    a, e, _ = _layer(h, e, net['W1'], net['b1'])
    h, e = _hidden(a, e, act)
    a, e, _ = _layer(h, e, net['W2'], net['b2'])
    h, e = _hidden(a, e, act)
    return _layer(h, e, net['W3'], net['b3'])


def critic_q(c, x, a, e_a=None):
    """c: dict with kind, W1 [64, n1], b1, W2, b2, W2a [64, k], W3 [1, 64], b3, optional obs_shift / obs_scale [D], act_scale [k]
    (None = 1) and activation; x [R, D], a [R, k] with elementwise error e_a (None: exact inputs) -> (q [R], e32 [R], mag [R])."""
    act = c.get('activation', 'relu')
    a = _f64(a)
    s = _f64(c.get('act_scale'))
    s = np.ones(a.shape[1]) if s is None else s
    as_ = a / s
    e_as = (0.0 if e_a is None else e_a) / np.abs(s) + gamma(2) * np.abs(as_)
    xn, e_x = _normalise(c, x)
    if c['kind'] == TD3:
        h, e = np.concatenate([xn, as_], 1), np.concatenate([e_x, e_as], 1)
    else:
        h, e = xn, e_x
    a1, e, _ = _layer(h, e, c['W1'], c['b1'])
    h, e = _hidden(a1, e, act)
    k = as_.shape[1]
    a2, e, _ = _layer(np.concatenate([h, as_], 1), np.concatenate([e, e_as], 1),
                      np.concatenate([_f64(c['W2']), _f64(c['W2a'])], 1), c['b2'], n=64 + 4 * ((k + 3) // 4))
    h, e = _hidden(a2, e, act)
    q, e, mag = _layer(h, e, c['W3'], c['b3'])
    return q[:, 0], e[:, 0], mag[:, 0]


def target(actor, critics, next_obs, reward, absorbing, g, eps=None, noise_std=0.0, noise_clip=0.0, low=None, high=None,
           mean_mode=1, dtype=np.float32, wrong=None):
    """-> dict: y, e_y, scale_y [R]; a (= a''), e_a, scale_a [R, k]; q [R, n_critics]; and what the case builder asserts its
    regimes from: noise_raw (noise_std eps), a_free (a' + n before the action clamp).  wrong='absorbing_ge': the flag read as
    >= 0.5."""
    g, noise_std, noise_clip = (float(dtype(v)) for v in (g, noise_std, noise_clip))
    m, e_m, mag_m = mlp(actor, next_obs)
    if mean_mode:
        s = _f64(actor.get('act_scale'))
        s = np.ones(m.shape[1]) if s is None else s
        a1 = s * np.tanh(m)
        e_a = np.abs(s) * (e_m + TANH_ABS)
        scale_a = np.abs(s) * (mag_m + 1.0)
    else:
        a1, e_a, scale_a = m, e_m, mag_m
    raw = np.zeros_like(a1) if eps is None else noise_std * _f64(eps)
    n = np.clip(raw, -noise_clip, noise_clip)
    free = a1 + n
    e_a = e_a + gamma(4) * (np.abs(a1) + np.abs(n))
    scale_a = scale_a + np.abs(n)
    a2 = free if low is None else np.clip(free, _f64(low), _f64(high))
    qs = [critic_q(c, next_obs, a2, e_a) for c in critics]
    q = np.min([v[0] for v in qs], 0)
    e_q = np.max([v[1] for v in qs], 0)
    mag_q = np.max([v[2] for v in qs], 0)
    r, keep = _f64(reward), 1.0 - _absorbed(absorbing, wrong)
    y = r + g * (keep * q)
    e_y = abs(g) * keep * e_q + gamma(2) * (np.abs(r) + np.abs(g * q))
    return dict(y=y, e_y=e_y, scale_y=np.abs(r) + abs(g) * mag_q, a=a2, e_a=e_a, scale_a=scale_a, q=np.stack([v[0] for v in qs], 1),
                noise_raw=raw, a_free=free)


def _absorbed(absorbing, wrong=None):
    assert wrong in (None, 'absorbing_ge')
    return (_f64(absorbing) >= 0.5) if wrong == 'absorbing_ge' else (_f64(absorbing) > 0.5)


def target_from_action(critics, next_obs, action, reward, absorbing, g, dtype=np.float32, wrong=None):
    """The critic half alone, from an action taken as exact (the a'' a device wrote): -> (y, e_y).  The same chain from the
    division on with e_a = 0: the sharper of the two float32 checks, because it does not carry the actor's error through the
    critics' norms."""
    g = float(dtype(g))
    qs = [critic_q(c, next_obs, action) for c in critics]
    q, e_q = np.min([v[0] for v in qs], 0), np.max([v[1] for v in qs], 0)
    r, keep = _f64(reward), 1.0 - _absorbed(absorbing, wrong)
    return r + g * (keep * q), abs(g) * keep * e_q + gamma(2) * (np.abs(r) + np.abs(g * q))


def soft_update(t, w, tau):
    """target = fl(fl(a w) + fl(b t)), a = (T) tau, b = (T)(1.0 - tau), in the arrays' own precision."""
    T = t.dtype.type
    a, b = T(tau), T(1.0 - tau)
    x = (a * w).astype(t.dtype)
    z = (b * t).astype(t.dtype)
    return (x + z).astype(t.dtype)


# ---------------------------------------------------------------------------------------------------------------- cases
def random_critic(rng, kind, D, k, activation='relu', normalise=True, act_scale=True, dtype=np.float32):
    def lin(o, i, bias=True):
        lim = math.sqrt(6.0 / (i + o))
        return rng.uniform(-lim, lim, (o, i)).astype(dtype), (rng.uniform(-0.3, 0.3, o).astype(dtype) if bias else None)
    n1 = D + k if kind == TD3 else D
    W1, b1 = lin(64, n1)
    W2, b2 = lin(64, 64)
    W2a, _ = lin(64, k, bias=False)
    W3, b3 = lin(1, 64)
    c = dict(kind=kind, W1=W1, b1=b1, W2=W2, b2=b2, W2a=W2a, W3=W3, b3=b3, activation=activation, obs_shift=None, obs_scale=None,
             act_scale=None)
    if normalise:
        c['obs_shift'] = rng.uniform(-1.0, 1.0, D).astype(dtype)
        c['obs_scale'] = rng.uniform(0.2, 2.0, D).astype(dtype)
    if act_scale:
        c['act_scale'] = rng.uniform(0.5, 2.0, k).astype(dtype)
    return c


# (kind, D, k, activation, normalise, act_scale given): DDPG (4, 1) is CH = 1, DDPG (32, 8) the maximum, TD3 n1 = 16, 25, 32
SHAPE_CASES = [(DDPG, 4, 1, 'relu', True, True), (DDPG, 18, 7, 'tanh', False, False), (DDPG, 32, 8, 'relu', True, True),
               (TD3, 13, 3, 'tanh', True, False), (TD3, 18, 7, 'relu', False, True), (TD3, 24, 8, 'tanh', True, True)]
SHAPE_SEEDS = [153, 100, 101, 101, 102, 101]      # 65 rows each; chosen so that every case passes assert_regimes in both dtypes
SHAPE_KEYS = ('kind', 'D', 'k', 'activation', 'normalise', 'act_scale')
# (rows, n_blocks); 600 rows on one workgroup: ten float32 tiles on four wavefronts, i.e. three rounds of phases
ROW_CASES = [(1, 0), (15, 0), (16, 0), (17, 0), (63, 0), (64, 0), (65, 0), (200, 1), (200, 2), (600, 1)]
ROW_SHAPE = (TD3, 18, 7, 'relu', True, True)
NOISE_STD, NOISE_CLIP, GAMMA, BOUND = 0.2, 0.5, 0.99, 0.8
# (name, n_critics, eps, bounds, mean_mode)
MODE_CASES = [('ddpg', 1, False, False, 1), ('td3', 2, True, True, 1), ('raw_mean', 2, True, True, 0)]


def case(seed, kind, D, k, activation, normalise, act_scale, rows, n_critics=2, with_eps=True, with_bounds=True, mean_mode=1,
         dtype=np.float32):
    """Everything of one target / q case, values exactly representable in `dtype`: actor (its W3 four times the initialisation
    scale, so that the tanh saturates on some rows and leaves others free), critics, next_obs of O(1), reward, absorbing on
    ~30 % of rows, eps uniform in +-4 (noise_std 0.2 against noise_clip 0.5: clipped beyond |eps| = 2.5), bounds at +-0.8 of
    the actor's act_scale, and the recorded action of a q call."""
    rng = np.random.default_rng(seed)
    actor = random_net(rng, D, k, activation, normalise, dtype)
    actor['W3'] = (actor['W3'] * (4.0 if mean_mode else 1.0)).astype(dtype)
    actor['act_scale'] = rng.uniform(0.5, 2.0, k).astype(dtype) if mean_mode else None
    critics = [random_critic(rng, kind, D, k, activation, normalise, act_scale, dtype) for _ in range(n_critics)]
    x = rng.normal(0.0, 1.0, (rows, D)).astype(dtype)
    s = actor['act_scale'] if mean_mode else np.ones(k, dtype)
    out = dict(actor=actor, critics=critics, next_obs=x, reward=rng.normal(0.0, 1.0, rows).astype(dtype),
               absorbing=(rng.random(rows) < 0.3).astype(dtype), eps=rng.uniform(-4.0, 4.0, (rows, k)).astype(dtype) if with_eps else None,
               low=(-BOUND * s).astype(dtype) if with_bounds else None, high=(BOUND * s).astype(dtype) if with_bounds else None,
               action=(rng.uniform(-1.0, 1.0, (rows, k)) * s).astype(dtype), mean_mode=mean_mode, gamma=GAMMA,
               noise_std=NOISE_STD if with_eps else 0.0, noise_clip=NOISE_CLIP if with_eps else 0.0, dtype=dtype)
    return out


def case_target(c):
    return target(c['actor'], c['critics'], c['next_obs'], c['reward'], c['absorbing'], c['gamma'], c['eps'], c['noise_std'],
                  c['noise_clip'], c['low'], c['high'], c['mean_mode'], c['dtype'])


def regimes(c, ref=None):
    """The share of elements (rows for the last four) in each regime of a full TD3 case."""
    ref = case_target(c) if ref is None else ref
    clip = float(c['dtype'](c['noise_clip']))
    raw, free = ref['noise_raw'], ref['a_free']
    lo, hi = _f64(c['low']), _f64(c['high'])
    q = ref['q']
    return dict(noise_low=np.mean(raw < -clip), noise_high=np.mean(raw > clip), noise_free=np.mean(np.abs(raw) < clip),
                act_low=np.mean(free < lo), act_high=np.mean(free > hi), act_free=np.mean((free > lo) & (free < hi)),
                q1_less=np.mean(q[:, 0] < q[:, 1]), q2_less=np.mean(q[:, 0] > q[:, 1]), absorbing=np.mean(_f64(c['absorbing']) > 0.5))


def assert_regimes(c, ref=None):
    r = regimes(c, ref)
    for name in ('noise_low', 'noise_high', 'noise_free', 'act_low', 'act_high', 'act_free'):
        assert r[name] >= 0.05, (name, r)
    assert r['q1_less'] >= 0.2 and r['q2_less'] >= 0.2, r
    assert 0.1 <= r['absorbing'] <= 0.5, r
    return r


def pair_case(seed, n_in, n_out, n_act, dtype):
    """(target tensors, online tensors) of one soft-update pair in the library's order W1, b1, W2, b2, W3, b3[, W2a]."""
    rng = np.random.default_rng(seed)
    shapes = [(64, n_in), (64,), (64, 64), (64,), (n_out, 64), (n_out,)] + ([(64, n_act)] if n_act else [])
    mk = lambda: [rng.normal(0.0, 1.0, s).astype(dtype) for s in shapes]          # noqa: E731
    return mk(), mk()


# (n_in, n_out, n_act): a plain network (an actor), a TD3 critic, a DDPG critic, the smallest network
PAIR_CASES = [(18, 7, 0), (25, 1, 7), (32, 1, 8), (1, 1, 0)]
