"""Cases that sit EXACTLY on the points where a gradient is discontinuous, for the four families of gradient kernels (fit, trust,
offgrad, soft) and the two TD targets: a ReLU pre-activation of exactly 0, two critics equal bit for bit, a log sigma exactly on a
clamp bound, an absorbing flag of exactly 0.5.  Pure numpy; a helper module: it holds no test.  tests/test_edge_cases_oracle.py
(CPU) and tests/test_gpu_gradient_edges.py use it.

The random cases of the oracles keep every row away from such points, because a float32 forward error could put a device and
the float64 oracle on different sides.  Here the compared quantity is an exact value in EVERY arithmetic and order of summation:
the products are 0 * finite = 0 or 1 * v = v, the sums are sums of exact zeros, and at most one rounding is shared by both
sides.  So the device and the oracle provably take the same decision, and the conventions the headers state are testable:
act'(0) = 0 (`h > 0`), critic 1 at a tie (`q_2 < q_1` selects critic 2), a clamp gate strict on both sides, `absorbing > 0.5`.

The constructions (each returns what it engineered, the `exempt` argument of the oracles):
  K1  dead_units: unit j1 of layer 1 and unit j2 of layer 2 have zero weights and bias, so a1[j1] = a2[j2] = 0 on every row.
  K2  pass_units + kink_rows: unit j1 passes input column 0 through, unit j2 passes h1[j1] through, and xn_0 is exactly 0 on the
      rows S_ROWS (x_0 == shift_0 bitwise), clearly positive on the odd rows and clearly negative on the even rows beside them.
  T   tie: the policy's outputs 0 and 1 are the same function, eps equal on TIE_ROWS, critic j passes a_j + 4 through.
  C   the sigma network's outputs 0 and 1 are the constants log_std_max and log_std_min.
  A   the absorbing column cycles through 0.5 (kept), the next value above 0.5 (dropped), -0.0 and 1.0.
Everything else stays random and is drawn again, as the oracles' own generators do, until every other unit, row and element is
clear of the oracles' flags; that is asserted, and no row is left out of a comparison."""
import functools

import numpy as np

import fit_oracle as fo
import offgrad_oracle as og
import offpolicy_oracle as oo
import soft_oracle as so
import trust_oracle as to

PAIRS = ((5, 42), (42, 5))        # (j1, j2): different groups of 16 and different v slots of the float32 mapping, and swapped
ROWS = 65                         # a full 64-row tile and a tail wave
S_ROWS = (0, 15, 16, 63, 64)      # first and last lane of a 16-block, a tile's last row, the tail wave
TIE_ROWS = tuple(sorted(set(range(0, ROWS, 3)) | set(S_ROWS)))
ABSORBING = lambda dtype: np.array([0.5, np.nextafter(dtype(0.5), dtype(1.0)), -0.0, 1.0], dtype)          # noqa: E731
ALL_UNITS = [(layer, u) for layer in (1, 2) for u in range(64)]
TRUST_SEED, OFFGRAD_SEED, SOFT_SEED, OFFPOLICY_SEED = 4200, 4300, 4400, 7
# The float32 bound of the PPO head grows with 1 / std^2 (fit_oracle's module docstring): with evaluate_oracle.case_data's std
# down to 1e-2 it is wider than what K2's gate moves db1[j1] and db2[j2] by, and a device with the wrong gate would pass.  4105 is
# the first seed from 4100 on at which the ORACLE's `kink_open` variant lies outside that bound on both, for both pairs of units
# (its std is 0.15 .. 1.3); the choice reads nothing but the oracle, and tests/test_edge_cases_oracle.py asserts what it claims.
FIT_SEEDS = {fo.VALUE: 4100, fo.PPO_CLIP: 4105}
SOFT_SHAPE = (18, 5)              # D, k: k >= 3, as T and C need


# ------------------------------------------------------------------------------------------------------- constructions
def dead_units(net, j1, j2):
    """K1 on a network's own arrays -> [(1, j1), (2, j2)]."""
    net['W1'][j1, :], net['b1'][j1] = 0.0, 0.0
    net['W2'][j2, :], net['b2'][j2] = 0.0, 0.0
    if 'W2a' in net:
        net['W2a'][j2, :] = 0.0
    return [(1, j1), (2, j2)]


def pass_units(net, j1, j2):
    """K2's units on a network's own arrays -> [(1, j1), (2, j2)]: a1[j1] = xn_0, a2[j2] = h1[j1], exactly."""
    dead_units(net, j1, j2)
    net['W1'][j1, 0] = 1.0
    net['W2'][j2, j1] = 1.0
    return [(1, j1), (2, j2)]


def kink_rows(x, shift, seed):
    """K2's rows: column 0 of x [ROWS, D] becomes shift_0 bitwise on S_ROWS, shift_0 + (0.5 .. 1.5) on the other odd rows and
    shift_0 - (0.5 .. 1.5) on the other even rows.  -> the column, for a generator that draws rows again to put it back."""
    rng = np.random.default_rng(seed)
    s0 = x.dtype.type(0.0) if shift is None else shift[0]
    r = np.arange(x.shape[0])
    col = (np.float64(s0) + np.where(r % 2 == 1, 1.0, -1.0) * rng.uniform(0.5, 1.5, x.shape[0])).astype(x.dtype)
    col[list(S_ROWS)] = s0
    x[:, 0] = col
    return col


def row_kind(x, shift):
    """-1 / 0 / +1 per row: the sign of xn_0, exact in every arithmetic."""
    s0 = 0.0 if shift is None else np.float64(shift[0])
    return np.sign(np.asarray(x[:, 0], np.float64) - s0).astype(int)


def first_input(net, x, a=None, dtype=np.float64):
    """What the first layer of `net` reads, in `dtype` arithmetic: the normalised observation and, for a critic whose first
    layer is wider than the observation, the action (over the critic's act_scale, if it has one)."""
    x = np.asarray(x, dtype)
    if net.get('obs_shift') is not None:
        x = (x - net['obs_shift'].astype(dtype)) * net['obs_scale'].astype(dtype)
    if net['W1'].shape[1] > x.shape[1]:
        a = np.asarray(a, dtype)
        if net.get('act_scale') is not None:
            a = a / net['act_scale'].astype(dtype)
        x = np.concatenate([x, a], 1)
    return x


def pre_activations(net, x, a=None, dtype=np.float64):
    """(a1, a2) of the two hidden layers in `dtype` numpy arithmetic, ReLU between them: what the premises are checked on."""
    W = lambda n: net[n].astype(dtype)                                                   # noqa: E731
    a1 = first_input(net, x, a, dtype) @ W('W1').T + W('b1')
    a2 = np.maximum(a1, 0) @ W('W2').T + W('b2')
    if 'W2a' in net:
        s = net.get('act_scale')
        a2 = a2 + (np.asarray(a, dtype) / (1 if s is None else s.astype(dtype))) @ W('W2a').T
    return a1, a2


def _edge(name, j1, j2, seed):
    """The callable that fit_oracle.case and trust_oracle.case take as `edge`."""
    def apply(net, x):
        if name == 'K1':
            return dead_units(net, j1, j2)
        units = pass_units(net, j1, j2)
        kink_rows(x, net['obs_shift'], seed)
        return units
    return apply


# ---------------------------------------------------------------------------------------------------------- fit, trust
@functools.lru_cache(maxsize=None)
def fit_case(name, j1, j2, head, dtype=np.float32):
    """fit_oracle.case of ROW_SHAPE[head] at ROWS rows with K1 or K2 applied -> the case; c['exempt'] names the units."""
    c = fo.case(FIT_SEEDS[head], head, *fo.ROW_SHAPE[head], ROWS, dtype=dtype, edge=_edge(name, j1, j2, FIT_SEEDS[head]))
    assert c['want']['kinks'] == 0 and c['exempt'] == [(1, j1), (2, j2)]
    c.update(name=name, j1=j1, j2=j2)
    return c


@functools.lru_cache(maxsize=None)
def trust_case(name, j1, j2, dtype=np.float32):
    """trust_oracle.case of ROW_SHAPE at ROWS rows with K1 (damping 0: the engineered components of F v are exactly 0) or K2
    (the usual damping)."""
    c = to.case(TRUST_SEED, *to.ROW_SHAPE, ROWS, dtype=dtype, edge=_edge(name, j1, j2, TRUST_SEED), damping=0.0 if name == 'K1' else to.DAMPING)
    assert c['want']['kinks'] == 0 and c['exempt'] == [(1, j1), (2, j2)]
    c.update(name=name, j1=j1, j2=j2)
    return c


def unit_slices(n_in, j1, j2, w2a=0):
    """The positions of dW1[j1, :], db1[j1], dW2[j2, :], db2[j2] (and dW2a[j2, :] of a critic with k = w2a) in a flat gradient of
    the libraries' order W1, b1, W2, b2, W3, b3[, W2a] -> an index array."""
    o_b1 = 64 * n_in
    o_W2 = o_b1 + 64
    o_b2 = o_W2 + 4096
    idx = list(range(j1 * n_in, (j1 + 1) * n_in)) + [o_b1 + j1] + list(range(o_W2 + 64 * j2, o_W2 + 64 * (j2 + 1))) + [o_b2 + j2]
    if w2a:
        o_W2a = o_b2 + 64 + 64 + 1
        idx += list(range(o_W2a + j2 * w2a, o_W2a + (j2 + 1) * w2a))
    return np.array(idx)


def bias_slots(n_in, j1, j2):
    """The positions of db1[j1] and db2[j2] in a flat gradient: K2's named elements."""
    return np.array([64 * n_in + j1, 64 * n_in + 64 + 4096 + j2])


# -------------------------------------------------------------------------------------------------------------- offgrad
@functools.lru_cache(maxsize=None)
def offgrad_case(name, which, j1, j2, kind, dtype=np.float32):
    """offgrad_oracle.case's data (ROW_SHAPE with the critic `kind`, mean_mode 1, ROWS rows) with K1 or K2 applied to `which`:
    'actor', or 'critics' (both).  -> the case with want_critic, want_actor and c['exempt'] = {'actor': pairs, 'critics':
    [pairs, pairs]}.  With K2 every network that is engineered normalises column 0 alike (the first critic's shift and scale),
    so that one observation column is exactly 0 for all of them."""
    shape = (kind,) + og.ROW_SHAPE[1:]
    D, k, activation = shape[1], shape[2], shape[3]
    b = oo.case(OFFGRAD_SEED, *shape, ROWS, n_critics=2, mean_mode=1, dtype=dtype)
    rng = np.random.default_rng(OFFGRAD_SEED + 77)
    c = dict(actor=b['actor'], critics=b['critics'], obs=b['next_obs'].copy(), action=b['action'].copy(), mean_mode=1, dtype=dtype,
             kind=kind, D=D, k=k, activation=activation, idx=None, name=name, which=which, j1=j1, j2=j2)
    nets = [c['actor']] if which == 'actor' else c['critics']
    for n in nets[1:]:
        n['obs_shift'][0], n['obs_scale'][0] = nets[0]['obs_shift'][0], nets[0]['obs_scale'][0]
    units = [(dead_units if name == 'K1' else pass_units)(n, j1, j2) for n in nets]
    exempt = {'actor': units[0]} if which == 'actor' else {'critics': units}
    col = kink_rows(c['obs'], nets[0]['obs_shift'], OFFGRAD_SEED) if name == 'K2' else None
    s = b['actor']['act_scale']
    for _ in range(og.REDRAWS):
        bad = og.row_kinks(c, exempt)
        if not bad.any():
            break
        n = int(bad.sum())
        c['obs'][bad] = rng.normal(0.0, 1.0, (n, D)).astype(dtype)
        c['action'][bad] = (rng.uniform(-1.0, 1.0, (n, k)) * s).astype(dtype)
        if col is not None:
            c['obs'][:, 0] = col
    assert not og.row_kinks(c, exempt).any(), 'rows at a kink after %d redraws' % og.REDRAWS
    x, a = c['obs'], c['action']
    q1 = og.critic_forward(c['critics'][0], x, a)['q']
    c['target'] = (q1 + rng.normal(0.0, 1.0, ROWS)).astype(dtype)
    c['exempt'] = exempt
    c['want_critic'] = [og.critic_gradient(cr, x, a, c['target'], exempt=og._of(exempt, 'critics', j)) for j, cr in enumerate(c['critics'])]
    c['want_actor'] = og.actor_gradient(c['actor'], c['critics'][0], x, 1, exempt=exempt)
    assert all(w['kinks'] == 0 for w in c['want_critic'])
    return c


# ----------------------------------------------------------------------------------------------------------------- soft
def _tie_critic(cr, D, j):
    """T's critic j: q = fl(a_j + 4) through one live unit per layer, everything else zero."""
    for n in so.PARAMS:
        cr[n][...] = 0.0
    cr['W1'][0, D + j], cr['b1'][0], cr['W2'][0, 0], cr['W3'][0, 0] = 1.0, 4.0, 1.0, 1.0


@functools.lru_cache(maxsize=None)
def soft_case(name, which=None, j1=5, j2=42, activation='relu', dtype=np.float32):
    """soft_oracle.case's data (SOFT_SHAPE, normalised, with act_scale and act_shift, ROWS rows, no idx) with one construction:
      'K1' / 'K2' on which = 'policy' (the mu and the sigma network) or 'critics' (the online and the target pair);
      'K1' on which = 'critics_a0': the critics' unit j1 keeps its weight on ACTION column 0, W1[j1, D + 0], and that action
           element is exactly 0 on every row (the mu network's output 0 is the constant 0, eps[:, 0] = 0, act_shift[0] = 0; the
           recorded action's column 0 is 0 too), so that the unit is dead by 0 * finite and its gate decides whether
           W1[j1, D + 0] reaches dq/da_0 -- with any other action element left random a unit with such a weight is not dead;
      'T', 'C', 'A' as the module docstring says ('T': both critic pairs).
    -> the case with want_target, want_critic, want_actor and c['exempt'], the description every oracle call takes.  The seed is
    moved on, as fit_oracle.case does, until the bound on logp is small on every row (soft_oracle.LOGP_BOUND); that is asserted."""
    for attempt in range(16):
        c = _soft_case(SOFT_SEED + 1000 * attempt, name, which, j1, j2, activation, dtype)
        if all((w['logp'].e <= so.LOGP_BOUND).all() for w in (c['want_target'], c['want_actor'])):
            break
    for w in (c['want_target'], c['want_actor']):
        assert (w['logp'].e <= so.LOGP_BOUND).all(), float(w['logp'].e.max())
    return c


def _soft_case(seed, name, which, j1, j2, activation, dtype):
    D, k = SOFT_SHAPE
    rng = np.random.default_rng(seed)
    pol = so.random_policy(rng, D, k, activation, True, dtype)
    lo, hi = dtype(pol['log_std_min']), dtype(pol['log_std_max'])
    assert float(lo) == pol['log_std_min'] and float(hi) == pol['log_std_max'], 'the clamp bounds round-trip through the dtype'
    c = dict(policy=pol, critics=[so.random_soft_critic(rng, D, k, activation, True, dtype) for _ in range(2)],
             targets=[so.random_soft_critic(rng, D, k, activation, True, dtype) for _ in range(2)], dtype=dtype, D=D, k=k,
             activation=activation, saturate=False, gamma=float(dtype(so.GAMMA)), log_alpha=float(dtype(so.LOG_ALPHA)),
             target_entropy=float(-k), idx=None, name=name, which=which, j1=j1, j2=j2)
    c['act_scale'] = rng.uniform(0.5, 2.0, k).astype(dtype)
    c['act_shift'] = rng.uniform(-0.5, 0.5, k).astype(dtype)
    c['obs'] = rng.normal(0.0, 1.0, (ROWS, D)).astype(dtype)
    c['action'] = (rng.uniform(-1.0, 1.0, (ROWS, k)) * c['act_scale'] + c['act_shift']).astype(dtype)
    c['reward'] = rng.normal(0.0, 1.0, ROWS).astype(dtype)
    c['absorbing'] = (rng.uniform(0.0, 1.0, ROWS) < 0.25).astype(dtype)
    draw = lambda n: np.clip(rng.normal(0.0, 1.0, (n, k)), -2.0, 2.0).astype(dtype)         # noqa: E731
    c['eps'] = draw(ROWS)
    mu, sigma, four = pol['mu'], pol['sigma'], c['critics'] + c['targets']
    exempt, col, tie = {}, None, np.zeros(ROWS, bool)
    if name in ('K1', 'K2') and which == 'policy':
        f = dead_units if name == 'K1' else pass_units
        exempt = {'mu': f(mu, j1, j2), 'sigma': f(sigma, j1, j2)}
        shift = mu['obs_shift']
    elif name in ('K1', 'K2'):
        for cr in four[1:]:
            cr['obs_shift'][0], cr['obs_scale'][0] = four[0]['obs_shift'][0], four[0]['obs_scale'][0]
        keep = [cr['W1'][j1, D].copy() for cr in four]
        units = [(dead_units if name == 'K1' else pass_units)(cr, j1, j2) for cr in four]
        exempt = {'critics': units[:2]}
        shift = four[0]['obs_shift']
        if which == 'critics_a0':
            assert name == 'K1'
            for cr, w in zip(four, keep):
                cr['W1'][j1, D] = w
            mu['W3'][0, :], mu['b3'][0], c['act_shift'][0] = 0.0, 0.0, 0.0
    elif name == 'T':
        assert activation == 'relu'
        for net in (mu, sigma):
            net['W3'][1, :], net['b3'][1] = net['W3'][0, :], net['b3'][0]
        c['act_scale'][1], c['act_shift'][1] = c['act_scale'][0], c['act_shift'][0]
        for pair in (c['critics'], c['targets']):
            for j, cr in enumerate(pair):
                _tie_critic(cr, D, j)
        tie[list(TIE_ROWS)] = True
        exempt = {'critics': [ALL_UNITS, ALL_UNITS], 'tie': tie}
    elif name == 'C':
        sigma['W3'][0, :], sigma['b3'][0] = 0.0, hi
        sigma['W3'][1, :], sigma['b3'][1] = 0.0, lo
        exempt = {'edge': np.arange(k) < 2}
    elif name == 'A':
        c['absorbing'] = ABSORBING(dtype)[np.arange(ROWS) % 4]
    else:
        raise ValueError(name)
    if name == 'K2':
        col = kink_rows(c['obs'], shift, seed)
    sc, sh = so._vec(c['act_scale'], k), so._vec(c['act_shift'], k, 0.0)

    def impose():
        if col is not None:
            c['obs'][:, 0] = col
        if which == 'critics_a0':
            c['eps'][:, 0], c['action'][:, 0] = 0.0, 0.0
        c['eps'][tie, 1] = c['eps'][tie, 0]

    impose()
    for _ in range(so.REDRAWS):
        bad = so.row_flags(c, exempt)
        if not bad.any():
            break
        n = int(bad.sum())
        c['obs'][bad] = rng.normal(0.0, 1.0, (n, D)).astype(dtype)
        c['action'][bad] = (rng.uniform(-1.0, 1.0, (n, k)) * sc + sh).astype(dtype)
        c['eps'][bad] = draw(n)
        impose()
    assert not so.row_flags(c, exempt).any(), 'rows at a kink, a tie or a clamp edge after %d redraws' % so.REDRAWS
    x, a = c['obs'], c['action']
    q1 = so.critic_forward(c['critics'][0], x, a)['q'].v
    c['target'] = (q1 + rng.normal(0.0, 1.0, ROWS)).astype(dtype)
    c['exempt'] = exempt
    args = (c['log_alpha'], c['eps'], c['act_scale'], c['act_shift'])
    c['want_target'] = so.target(pol, c['targets'], x, c['reward'], c['absorbing'], c['gamma'], *args, exempt=exempt)
    c['want_critic'] = [so.critic_gradient(cr, x, a, c['target'], exempt=so._of(exempt, 'critics', j)) for j, cr in enumerate(c['critics'])]
    c['want_actor'] = so.actor_gradient(pol, c['critics'], x, c['eps'], c['log_alpha'], c['target_entropy'], c['act_scale'], c['act_shift'],
                                        exempt=exempt)
    assert all(w['kinks'] == 0 for w in c['want_critic'])
    return c


def soft_actor_args(c):
    return (c['policy'], c['critics'], c['obs'], c['eps'], c['log_alpha'], c['target_entropy'], c['act_scale'], c['act_shift'])


def soft_target_args(c):
    return (c['policy'], c['targets'], c['obs'], c['reward'], c['absorbing'], c['gamma'], c['log_alpha'], c['eps'], c['act_scale'], c['act_shift'])


# ------------------------------------------------------------------------------------------------------------ offpolicy
@functools.lru_cache(maxsize=None)
def offpolicy_case(dtype=np.float32):
    """offpolicy_oracle.case of ROW_SHAPE at ROWS rows (the seed of tests/test_gpu_offpolicy.py's row cases) with A's absorbing
    column -> (case, offpolicy_oracle.case_target of it)."""
    c = oo.case(seed=OFFPOLICY_SEED, rows=ROWS, dtype=dtype, **dict(zip(oo.SHAPE_KEYS, oo.ROW_SHAPE)))
    c['absorbing'] = ABSORBING(dtype)[np.arange(ROWS) % 4]
    return c, oo.case_target(c)
