"""GPU tests of libatacom_soft.so (rl_on_manifold_amd/soft.py): SAC's fused soft target, the critics' gradients, the actor's
gradients with respect to the mu and sigma networks and the temperature's Adam step against the float64 oracle
(tests/soft_oracle.py), float32 inside its derived bound on EVERY element and float64 to 1e-12 of scale (+ 1e-14); row counts
around the 16-row block and the 64-row tile, one and several rounds per workgroup, repeated calls bit for bit, another grid with
the per-row outputs bit-equal; every ceil(D / 4) and ceil((D + k) / 4) path, both activations, with and without normalisation and
action scaling; a pair of critics against two single calls; the columns of a replay memory read in place through an unsorted idx
with repeats, NaN where the call must not read and poison around the outputs; a saturated policy; the hand-over to the device
Adam; AlphaAdam against torch's Adam and a numpy float32 restatement; one whole fit captured in a graph and replayed.

The float32 results are held to the chain cut at the device's own intermediates (soft_oracle.target and actor_gradient say why):
action_out and logp_out inside the policy's forward bounds, y and q_out inside the bound at the device's action (and logp) taken
as exact, dqda_out inside the bound of dq/da at that action, the gradients inside the bound of the backward pass from the
device's dq/da and selection -- and inside the end-to-end bound wherever that covers every row."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_oracle as po                                     # noqa: E402
import soft_oracle as so                                      # noqa: E402

DEV = 'cuda:0'
DT = {'f32': torch.float32, 'f64': torch.float64}
NP = {'f32': np.float32, 'f64': np.float64}
_cache = {}


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _objects(c):
    """(MlpPolicy, [SoftCritic] online, [SoftCritic] targets, log_alpha) on the device of an oracle case."""
    from rl_on_manifold_amd import MlpPolicy, SoftCritic
    mu, sg = c['policy']['mu'], c['policy']['sigma']
    pol = MlpPolicy(*(_t(mu[k]) for k in so.PARAMS), obs_shift=_t(mu['obs_shift']), obs_scale=_t(mu['obs_scale']), activation=mu['activation'],
                    sigma_weights=[_t(sg[k]) for k in so.PARAMS], squash=True, log_std_min=c['policy']['log_std_min'],
                    log_std_max=c['policy']['log_std_max'])
    mk = lambda cr: SoftCritic(*(_t(cr[k]) for k in so.PARAMS), n_act=c['k'], obs_shift=_t(cr['obs_shift']),         # noqa: E731
                               obs_scale=_t(cr['obs_scale']), activation=cr['activation'])
    la = torch.tensor([c['log_alpha']], dtype=DT['f32' if c['dtype'] == np.float32 else 'f64'], device=DEV)
    return pol, [mk(cr) for cr in c['critics']], [mk(cr) for cr in c['targets']], la


def _case(dt, shape, rows, seed, **kw):
    key = (dt, shape, rows, seed, tuple(sorted(kw.items())))
    if key not in _cache:
        c = so.case(seed, *shape, rows, dtype=NP[dt], **kw)
        _cache[key] = (c,) + _objects(c)
    return _cache[key]


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _inside(dt, got, want, what, key='flat', bound='bound', scale='scale'):
    got = _np(got)
    assert np.isfinite(got).all(), what
    ok, worst = so.inside(got, want, NP[dt], key, bound, scale)
    print('%s %s %s: worst |error| / allowance %.4f' % (what, key, dt, worst))
    assert ok, (what, key, dt, 'worst |error| / allowance %.3f' % worst)


def _inside_v(dt, got, want, what, extra=None):
    got = _np(got)
    assert np.isfinite(got).all(), what
    ok, worst = so.inside_v(got, want, NP[dt], extra)
    print('%s %s: worst |error| / allowance %.4f' % (what, dt, worst))
    assert ok, (what, dt, 'worst |error| / allowance %.3f' % worst)


def _nan(dt, *shape):
    return torch.full(shape, float('nan'), dtype=DT[dt], device=DEV)


def _kw(c):
    return dict(act_scale=c['act_scale'] if c['act_scale'] is None else _t(c['act_scale']),
                act_shift=c['act_shift'] if c['act_shift'] is None else _t(c['act_shift']),
                idx=None if c['idx'] is None else _t(c['idx']))


def _target(dt, c, pol, tgs, la, n_blocks=0):
    from rl_on_manifold_amd import soft_td_target
    M, k = c['eps'].shape
    aout, lp = _nan(dt, M, k), _nan(dt, M)
    y = soft_td_target(pol, tgs, _t(c['obs']), _t(c['reward']), _t(c['absorbing']), c['gamma'], la, _t(c['eps']), action_out=aout,
                       logp_out=lp, n_blocks=n_blocks, **_kw(c))
    return y, aout, lp


def _check_target(dt, c, pol, tgs, la, n_blocks, what, sat=False):
    y, aout, lp = _target(dt, c, pol, tgs, la, n_blocks)
    want = c['want_target']
    what = what + ('target',)
    extra = want['sat'] / (abs(c['gamma']) * np.exp(c['log_alpha'])) if sat else None
    _inside_v(dt, aout, want['a'], what + ('a',))
    _inside_v(dt, lp, want['logp'], what + ('logp',), extra)
    args = (c['policy'], c['targets'], c['obs'], c['reward'], c['absorbing'], c['gamma'], c['log_alpha'], c['eps'], c['act_scale'], c['act_shift'], c['idx'])
    at = so.target(*args, action=_np(aout), logp=_np(lp))
    assert not at['kink'].any() and not at['tie'].any()
    _inside_v(dt, y, at['y'], what + ('y at the device action and logp',))
    if dt == 'f64' or want['kinks_e2e'] == 0:
        _inside_v(dt, y, want['y'], what + ('y end to end',), want['sat'] if sat else None)
    return y, aout, lp


def _critics(dt, c, crs, n_blocks=0, **kw):
    from rl_on_manifold_amd import soft_critic_gradient
    idx = None if c['idx'] is None else _t(c['idx'])
    return soft_critic_gradient(crs, _t(c['obs']), _t(c['action']), _t(c['target']), idx=idx, n_blocks=n_blocks, **kw)


def _check_critics(dt, c, crs, n_blocks, what):
    gs = _critics(dt, c, crs, n_blocks)
    for j, (g, want) in enumerate(zip(gs, c['want_critic'])):
        _inside(dt, g.flat, want, what + ('critic', j))
        _inside(dt, g.stats, want, what + ('critic', j), 'stats', 'stats_bound', 'stats_scale')
        assert g.stats[1:].eq(0).all()
    return gs


def _actor(dt, c, pol, crs, la, n_blocks=0, **kw):
    from rl_on_manifold_amd import soft_actor_gradient
    M, k = c['eps'].shape
    outs = dict(action_out=_nan(dt, M, k), logp_out=_nan(dt, M), q_out=_nan(dt, M, 2), dqda_out=_nan(dt, M, k))
    g = soft_actor_gradient(pol, crs, _t(c['obs']), _t(c['eps']), la, c['target_entropy'], n_blocks=n_blocks, **outs, **_kw(c), **kw)
    return g, outs


def _check_actor(dt, c, pol, crs, la, n_blocks, what):
    g, o = _actor(dt, c, pol, crs, la, n_blocks)
    want = c['want_actor']
    what = what + ('actor',)
    _inside_v(dt, o['action_out'], want['a'], what + ('a',))
    _inside_v(dt, o['logp_out'], want['logp'], what + ('logp',))
    args = (c['policy'], c['critics'], c['obs'], c['eps'], c['log_alpha'], c['target_entropy'], c['act_scale'], c['act_shift'], c['idx'])
    a_np, q_np, dq_np = _np(o['action_out']), _np(o['q_out']), _np(o['dqda_out'])
    at = so.actor_gradient(*args, action=a_np, q=q_np)
    assert not at['kink'].any() and not at['tie'].any() and not at['edge'].any()
    for j in range(2):
        _inside_v(dt, o['q_out'][:, j], at['q'][j], what + ('q_%d at the device action' % (j + 1),))
    _inside_v(dt, o['dqda_out'], at['dqda'], what + ('dq/da at the device action',))
    frm = so.actor_gradient(*args, action=a_np, q=q_np, dq=dq_np)
    for part in ('mu', 'sigma'):
        _inside(dt, getattr(g, part).flat, frm[part], what + (part, 'from the device dq/da'))
    # the statistics: the loss at the device's action, the rest from the policy alone
    _inside(dt, g.stats, at, what + ('at the device action',), 'stats', 'stats_bound', 'stats_scale')
    if dt == 'f64' or want['kinks_e2e'] == 0:
        for part in ('mu', 'sigma'):
            _inside(dt, getattr(g, part).flat, want[part], what + (part, 'end to end'))
        _inside(dt, g.stats, want, what + ('end to end',), 'stats', 'stats_bound', 'stats_scale')
    # rows with a clamped log sigma contribute exactly nothing to the sigma network through their clamped elements
    M = a_np.shape[0]
    assert float(g.stats[3]) == float(NP[dt](int(want['clamped'].sum())) / NP[dt](M))
    return g, o


def _all_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('rows,n_blocks', so.ROW_CASES)
def test_row_counts_and_grids(dt, rows, n_blocks):
    """1 .. 600 rows: a lone row, a part-filled 16-block, a tail wave, 200 rows walked by one and by two workgroups, and 600 by
    one, whose wavefronts walk several rounds.  Two calls with the same grid give the same bits; another grid inside the bound
    gives the same per-row outputs, bit for bit."""
    c, pol, crs, tgs, la = _case(dt, so.ROW_SHAPE, rows, 300 + rows)
    what = (so.ROW_SHAPE, rows, n_blocks)
    t1 = _check_target(dt, c, pol, tgs, la, n_blocks, what)
    gs = _check_critics(dt, c, crs, n_blocks, what)
    ga, o = _check_actor(dt, c, pol, crs, la, n_blocks, what)
    assert _all_bits(t1, _target(dt, c, pol, tgs, la, n_blocks))
    gs2 = _critics(dt, c, crs, n_blocks)
    assert all(torch.equal(a.flat, b.flat) and torch.equal(a.stats, b.stats) for a, b in zip(gs, gs2))
    ga2, o2 = _actor(dt, c, pol, crs, la, n_blocks)
    assert torch.equal(ga.mu.flat, ga2.mu.flat) and torch.equal(ga.sigma.flat, ga2.sigma.flat) and torch.equal(ga.stats, ga2.stats)
    assert _all_bits(o.values(), o2.values())
    other = 3 if n_blocks != 3 else 2
    assert _all_bits(t1, _target(dt, c, pol, tgs, la, other))
    ga3, o3 = _actor(dt, c, pol, crs, la, other)
    assert _all_bits(o.values(), o3.values())
    for part in ('mu', 'sigma'):
        _inside(dt, getattr(ga3, part).flat, c['want_actor'][part] if dt == 'f64' else
                so.actor_gradient(c['policy'], c['critics'], c['obs'], c['eps'], c['log_alpha'], c['target_entropy'], c['act_scale'],
                                  c['act_shift'], c['idx'], action=_np(o3['action_out']), q=_np(o3['q_out']), dq=_np(o3['dqda_out']))[part],
                what + (part, 'another grid'))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('shape', so.SHAPE_CASES)
def test_every_first_layer_width_activation_and_option(dt, shape):
    """65 rows each: every ceil(D / 4) of the policy and ceil((D + k) / 4) of the critics from 1 to 8, both activations, with and
    without normalisation, with and without act_scale and act_shift."""
    c, pol, crs, tgs, la = _case(dt, shape, 65, 100 + so.SHAPE_CASES.index(shape))
    what = (shape,)
    _check_target(dt, c, pol, tgs, la, 0, what)
    _check_critics(dt, c, crs, 0, what)
    g, _ = _check_actor(dt, c, pol, crs, la, 0, what)
    w = c['want_actor']
    # rows beyond a clamp bound are present: their elements give the sigma network exactly nothing, Mu still receives du
    assert (~w['open']).any() and (w['dl'].v[~w['open']] == 0).all() and (w['dm'].v[~w['open']] != 0).any()


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_a_pair_of_critics_equals_two_single_calls(dt):
    c, pol, crs, tgs, la = _case(dt, so.ROW_SHAPE, 200, 500)
    pair = _critics(dt, c, crs, 2)
    for j in range(2):
        one = _critics(dt, c, crs[j], 2)
        assert torch.equal(one.flat, pair[j].flat) and torch.equal(one.stats, pair[j].stats)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_a_saturated_policy_stays_finite_and_inside_the_per_sample_bound(dt):
    """|u| up to about 8: log(w + 1e-6) is ill-conditioned, its bound per sample from the oracle's own 1 / (w + 1e-6); float64 is
    allowed 8 * 2^-53 / (w + 1e-6) per element on top of 1e-12 of scale."""
    c, pol, crs, tgs, la = _case(dt, (18, 5, 'tanh', True, True), 65, 21, saturate=True)
    assert float(np.abs(c['want_target']['u'].v).max()) > 5.0
    _check_target(dt, c, pol, tgs, la, 0, ('saturated',), sat=True)
    g, o = _actor(dt, c, pol, crs, la)
    for t in (g.mu.flat, g.sigma.flat, g.stats) + tuple(o.values()):
        assert torch.isfinite(t).all()
    if dt == 'f32':
        want = c['want_actor']
        frm = so.actor_gradient(c['policy'], c['critics'], c['obs'], c['eps'], c['log_alpha'], c['target_entropy'], c['act_scale'],
                                c['act_shift'], action=_np(o['action_out']), q=_np(o['q_out']), dq=_np(o['dqda_out']))
        _inside_v(dt, o['logp_out'], want['logp'], ('saturated', 'logp'))
        for part in ('mu', 'sigma'):
            _inside(dt, getattr(g, part).flat, frm[part], ('saturated', part))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_the_replay_memory_is_read_in_place(dt):
    """Unsorted idx with repeats into the storage of a ReplayMemory; NaN in every column and row the calls must not read; poison
    around the outputs."""
    from rl_on_manifold_amd import ReplayMemory
    shape, rows, n_idx = so.ROW_SHAPE, 200, 70
    c, pol, crs, tgs, la = _case(dt, shape, rows, 700, n_idx=n_idx)
    D, k = shape[0], shape[1]
    mem = ReplayMemory(rows + 7, D, k, dtype=DT[dt], device=DEV)
    nan = lambda *s: _nan(dt, *s)                                                         # noqa: E731
    idx = _t(c['idx'])
    kw = dict(act_scale=None if c['act_scale'] is None else _t(c['act_scale']), act_shift=None if c['act_shift'] is None else _t(c['act_shift']))
    # the target reads next_obs, reward, absorbing
    mem.add_fields(nan(rows, D), nan(rows, k), _t(c['reward']), _t(c['obs']), _t(c['absorbing']), nan(rows))
    mem.storage[rows:] = float('nan')
    used = np.zeros(rows, bool)
    used[c['idx']] = True
    mem.storage[:rows][_t(~used)] = float('nan')
    buf = nan(n_idx + 2)
    y = mem.soft_td_target(pol, tgs, idx, c['gamma'], la, _t(c['eps']), out=buf[1:-1], **kw)
    at = so.target(c['policy'], c['targets'], c['obs'], c['reward'], c['absorbing'], c['gamma'], c['log_alpha'], c['eps'], c['act_scale'],
                   c['act_shift'], c['idx'])
    assert torch.isnan(buf[0]) and torch.isnan(buf[-1]) and torch.isfinite(y).all()
    if dt == 'f64':
        _inside_v(dt, y, at['y'], ('memory', 'y'))
    direct = _check_target(dt, c, pol, tgs, la, 0, ('memory',))[0]
    assert torch.equal(y, direct)
    # the gradients read obs (and action)
    mem2 = ReplayMemory(rows + 7, D, k, dtype=DT[dt], device=DEV)
    mem2.add_fields(_t(c['obs']), _t(c['action']), nan(rows), nan(rows, D), nan(rows), nan(rows))
    mem2.storage[rows:] = float('nan')
    mem2.storage[:rows][_t(~used)] = float('nan')
    gs = mem2.soft_critic_gradient(crs, idx, _t(c['target']))
    ref = _critics(dt, c, crs)
    assert all(torch.equal(a.flat, b.flat) and torch.equal(a.stats, b.stats) for a, b in zip(gs, ref))
    for j in range(2):
        _inside(dt, gs[j].flat, c['want_critic'][j], ('memory', 'critic', j))
    pad = nan(n_idx + 2, k)
    ga = mem2.soft_actor_gradient(pol, crs, idx, _t(c['eps']), la, c['target_entropy'], action_out=pad[1:-1], **kw)
    gb, o = _actor(dt, c, pol, crs, la)
    assert torch.equal(ga.mu.flat, gb.mu.flat) and torch.equal(ga.sigma.flat, gb.sigma.flat) and torch.equal(ga.stats, gb.stats)
    assert torch.isnan(pad[0]).all() and torch.isnan(pad[-1]).all() and torch.equal(pad[1:-1], o['action_out'])
    st = mem2.storage
    assert all(torch.isnan(st[:, mem2.fields[n]]).all() for n in ('reward', 'next_obs', 'absorbing', 'last'))


def _policies(pol, crs):
    """The four Adam groups of a SAC fit: MlpPolicy objects over mu, sigma and the two critics."""
    from rl_on_manifold_amd import MlpPolicy
    t = pol.tensors
    sig = MlpPolicy(*(t[k] for k in ('sW1', 'sb1', 'sW2', 'sb2', 'sW3', 'sb3')))
    return [pol, sig, crs[0].as_policy(), crs[1].as_policy()]


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_one_device_adam_steps_all_four_networks(dt):
    """One Adam of four groups (per-group lr) from the results of the two gradient calls; float64 equals torch.optim.Adam over the
    same gradients to 1e-12."""
    from rl_on_manifold_amd import Adam
    c = so.case(800, *so.ROW_SHAPE, 65, dtype=NP[dt])
    pol, crs, tgs, la = _objects(c)                                                       # fresh objects: they are stepped
    nets = _policies(pol, crs)
    lrs = (3e-4, 1e-4, 1e-3, 2e-3)
    opt = Adam([dict(net=n, lr=lr) for n, lr in zip(nets, lrs)])
    gc = _critics(dt, c, crs)
    ga, _ = _actor(dt, c, pol, crs, la)
    grads = [ga.mu, ga.sigma, gc[0], gc[1]]
    before = [[n.tensors[k].clone() for k in so.PARAMS] for n in nets]
    opt.step(*grads)
    for n, g, b, lr in zip(nets, grads, before, lrs):
        ps = [p.detach().cpu().double().requires_grad_(True) for p in b]
        ref = torch.optim.Adam(ps, lr=lr)
        for p, name in zip(ps, so.PARAMS):
            p.grad = getattr(g, name).detach().cpu().double()
        ref.step()
        for p, name in zip(ps, so.PARAMS):
            got = n.tensors[name].detach().cpu().double()
            tol = 1e-12 * (p.abs() + lr) + 1e-14 if dt == 'f64' else 4 * 2.0 ** -24 * (p.abs() + lr)
            assert ((got - p.detach()).abs() <= tol).all(), name
            assert not torch.equal(got, b[so.PARAMS.index(name)].cpu().double())


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_alpha_adam_against_torch_and_the_float32_restatement(dt):
    """Steps 1, 2, 10, 1000 of one run: float64 to 1e-12 of torch's Adam, float32 bit-equal to the numpy float32 restatement."""
    from rl_on_manifold_amd import AlphaAdam
    rng = np.random.default_rng(5)
    grads = (rng.normal(0.0, 1.0, 1000) * 10.0 ** rng.uniform(-3, 1, 1000)).astype(NP[dt])
    la = torch.tensor([-1.5], dtype=DT[dt], device=DEV)
    opt = AlphaAdam(la, lr=3e-4)
    g_dev = _t(grads)
    x = NP[dt](-1.5)
    if dt == 'f64':
        p = torch.tensor([-1.5], dtype=torch.float64, requires_grad=True)
        ref = torch.optim.Adam([p], lr=3e-4)
    else:
        m = v = np.float32(0.0)
        head = po.fresh_head()
    for t in range(1, 1001):
        opt.step(g_dev[t - 1:t])
        if dt == 'f64':
            p.grad = torch.tensor([grads[t - 1]], dtype=torch.float64)
            ref.step()
        else:
            x, m, v, head = so.alpha_step32(x, grads[t - 1], m, v, head)
        if t in po.STEPS:
            got = la.cpu().numpy()[0]
            if dt == 'f64':
                assert abs(got - p.item()) <= 1e-12 * (abs(p.item()) + 3e-4 * t), t
            else:
                assert got == x and opt.moments.cpu().numpy().tolist() == [m, v], (t, got, x)
            assert int(opt.step_count.item()) == t
    snap = opt.snapshot()
    opt.step(g_dev[:1])
    opt.restore(snap)
    assert torch.equal(opt.state, snap[0]) and torch.equal(la, snap[1])
    opt.zero_state()
    assert int(opt.step_count.item()) == 0 and opt.pows.tolist() == [1.0, 1.0] and opt.moments.eq(0).all()


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_one_whole_fit_captured_and_replayed(dt):
    """target -> critic gradients -> actor gradients -> Adam -> AlphaAdam -> soft_update, captured with torch.cuda.graph on one
    stream and replayed: the parameters after N replays are bit-equal to N eager fits from the same state."""
    from rl_on_manifold_amd import Adam, AlphaAdam, soft_actor_gradient, soft_critic_gradient, soft_td_target, soft_update
    c = so.case(900, *so.ROW_SHAPE, 200, dtype=NP[dt], n_idx=70)
    pol, crs, tgs, la = _objects(c)
    nets = _policies(pol, crs)
    tnets = [t.as_policy() for t in tgs]
    opt = Adam([dict(net=n, lr=lr) for n, lr in zip(nets, (3e-4, 3e-4, 1e-3, 1e-3))])
    aopt = AlphaAdam(la, lr=1e-3)
    obs, act, rew, ab, eps, idx = (_t(c[k]) for k in ('obs', 'action', 'reward', 'absorbing', 'eps', 'idx'))
    kw = dict(act_scale=_t(c['act_scale']), act_shift=_t(c['act_shift']), idx=idx)
    y = torch.empty(70, dtype=DT[dt], device=DEV)
    out = {}

    def fit():
        soft_td_target(pol, tgs, obs, rew, ab, c['gamma'], la, eps, out=y, **kw)
        out['c'] = soft_critic_gradient(crs, obs, act, y, idx=idx, out=out.get('c'))
        out['a'] = soft_actor_gradient(pol, crs, obs, eps, la, c['target_entropy'], out=out.get('a'), **kw)
        opt.step(out['a'].mu, out['a'].sigma, out['c'][0], out['c'][1])
        aopt.step(out['a'].alpha_grad)
        soft_update(tnets, nets[2:], 0.005)

    params = [n.tensors[k] for n in nets + tnets for k in so.PARAMS] + [la]
    fit()                                                       # allocates the outputs and the workspaces
    start = [p.clone() for p in params]
    s_opt, s_a = opt.snapshot(), aopt.snapshot()
    N = 3
    for _ in range(N):
        fit()
    eager = [p.clone() for p in params]
    assert not torch.equal(eager[0], start[0]) and not torch.equal(eager[-1], start[-1])
    for p, s in zip(params, start):
        p.copy_(s)
    opt.restore(s_opt)
    aopt.restore(s_a)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            fit()
    for p, s in zip(params, start):                             # capture runs nothing, but start from the same state regardless
        p.copy_(s)
    opt.restore(s_opt)
    aopt.restore(s_a)
    for _ in range(N):
        graph.replay()
    torch.cuda.synchronize()
    for p, e in zip(params, eager):
        assert torch.equal(p, e)
