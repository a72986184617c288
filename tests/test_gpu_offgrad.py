"""GPU tests of libatacom_offgrad.so (rl_on_manifold_amd/offgrad.py): the gradient of the critics' mean-squared TD error and the
deterministic policy gradient of the actor against the float64 oracle (tests/offgrad_oracle.py), float32 inside its derived
bound on EVERY element and float64 to 1e-12 of scale; row counts around the 16-row block and the 64-row tile, one and several
rounds per workgroup, repeated calls bit for bit; every CH = ceil(n1 / 4) path of both critic kinds, both activations and both
mean modes; a pair against two single calls; the columns of a replay memory read in place through an unsorted idx with repeats,
NaN where the call must not read and poison around the outputs; the hand-over to torch's Adam and to the device Adam; graph
capture; refusals.  Shapes are the smallest at which the kernels can go wrong.

The actor's float32 gradient is held to the chain cut at the device's own intermediates (offgrad_oracle.case says why): its
action_out inside the actor's forward bound, its dqda_out inside the bound of dq/da at that action taken as exact, its gradient
inside the bound of the actor's backward pass from that dq/da taken as exact -- and inside the end-to-end bound wherever that
covers every row (no ReLU pre-activation of the critic within what the actor's whole worst-case error gives it)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import offgrad_oracle as og                                   # noqa: E402
import optim_oracle as po                                     # noqa: E402

DEV = 'cuda:0'
DT = {'f32': torch.float32, 'f64': torch.float64}
NP = {'f32': np.float32, 'f64': np.float64}
_cache = {}


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _objects(c):
    """(MlpPolicy, [QCritic]) on the device of an oracle case."""
    from rl_on_manifold_amd import MlpPolicy, QCritic
    a = c['actor']
    pol = MlpPolicy(*(_t(a[k]) for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')), obs_shift=_t(a['obs_shift']), obs_scale=_t(a['obs_scale']),
                    activation=a['activation'])
    if c['mean_mode']:
        pol.mean_mode, pol.tensors['act_scale'] = 1, _t(a['act_scale'])
    crs = [QCritic(*(_t(cr[k]) for k in ('W1', 'b1', 'W2', 'b2', 'W2a', 'W3', 'b3')), kind=cr['kind'], act_scale=_t(cr['act_scale']),
                   obs_shift=_t(cr['obs_shift']), obs_scale=_t(cr['obs_scale']), activation=cr['activation']) for cr in c['critics']]
    return pol, crs


def _case(dt, shape, rows, seed, **kw):
    key = (dt, shape, rows, seed, tuple(sorted(kw.items())))
    if key not in _cache:
        c = og.case(seed, *shape, rows, dtype=NP[dt], **kw)
        _cache[key] = (c,) + _objects(c)
    return _cache[key]


def _inside(dt, got, want, what, key='flat', bound='bound', scale='scale'):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    ok, worst = og.inside(got, want, NP[dt], key, bound, scale)
    print('%s %s %s: worst |error| / allowance %.4f' % (what, key, dt, worst))
    assert ok, (what, key, dt, 'worst |error| / allowance %.3f' % worst)


def _critics(dt, c, crs, n_blocks=0, **kw):
    from rl_on_manifold_amd import critic_gradient
    idx = None if c['idx'] is None else _t(c['idx'])
    return critic_gradient(crs, _t(c['obs']), _t(c['action']), _t(c['target']), idx=idx, n_blocks=n_blocks, **kw)


def _actor(dt, c, pol, cr, n_blocks=0, **kw):
    from rl_on_manifold_amd import actor_gradient
    M = c['target'].shape[0]
    aout = torch.full((M, c['k']), float('nan'), dtype=DT[dt], device=DEV)
    dq = torch.full((M, c['k']), float('nan'), dtype=DT[dt], device=DEV)
    idx = None if c['idx'] is None else _t(c['idx'])
    g = actor_gradient(pol, cr, _t(c['obs']), idx=idx, action_out=aout, dqda_out=dq, n_blocks=n_blocks, **kw)
    return g, aout, dq


def _check_critics(dt, c, crs, n_blocks, what):
    gs = _critics(dt, c, crs, n_blocks)
    for j, (g, want) in enumerate(zip(gs, c['want_critic'])):
        _inside(dt, g.flat, want, what + ('critic', j))
        _inside(dt, g.stats, want, what + ('critic', j), 'stats', 'stats_bound', 'stats_scale')
        assert g.stats[1:].eq(0).all()
    return gs


def _check_actor(dt, c, pol, cr, n_blocks, what):
    g, aout, dq = _actor(dt, c, pol, cr, n_blocks)
    want = c['want_actor']
    what = what + ('actor',)
    _inside(dt, aout, want, what, 'a', 'e_a', 'scale_a')
    a_np, dq_np = aout.cpu().numpy().astype(np.float64), dq.cpu().numpy().astype(np.float64)
    at = og.actor_gradient(c['actor'], c['critics'][0], c['obs'], c['mean_mode'], c['idx'], action=a_np)
    assert at['kinks'] == 0
    _inside(dt, dq, at, what + ('at the device action',), 'dqda', 'e_dqda', 'scale_dqda')
    _inside(dt, g.stats, at, what + ('at the device action',), 'stats', 'stats_bound', 'stats_scale')
    frm = og.actor_gradient(c['actor'], c['critics'][0], c['obs'], c['mean_mode'], c['idx'], dqda=dq_np)
    assert frm['kinks'] == 0
    _inside(dt, g.flat, frm, what + ('from the device dq/da',))
    if dt == 'f64' or want['kinks'] == 0:
        _inside(dt, g.flat, want, what + ('end to end',))
        _inside(dt, dq, want, what + ('end to end',), 'dqda', 'e_dqda', 'scale_dqda')
    assert g.stats[1:].eq(0).all()
    return g, aout, dq


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('rows,n_blocks', og.ROW_CASES)
def test_row_counts_and_grids(dt, rows, n_blocks):
    """1 .. 600 rows: a lone row, a part-filled 16-block, a tail wave, 200 rows walked by one and by two workgroups, and 600 by
    one, whose wavefronts walk several rounds.  Two calls with the same grid give the same bits; another grid is inside the
    bound (the order of summation changes)."""
    c, pol, crs = _case(dt, og.ROW_SHAPE, rows, 300 + rows)
    what = (og.ROW_SHAPE, rows, n_blocks)
    gs = _check_critics(dt, c, crs, n_blocks, what)
    ga, aout, dq = _check_actor(dt, c, pol, crs[0], n_blocks, what)
    gs2 = _critics(dt, c, crs, n_blocks)
    ga2, aout2, dq2 = _actor(dt, c, pol, crs[0], n_blocks)
    assert all(torch.equal(a.flat, b.flat) and torch.equal(a.stats, b.stats) for a, b in zip(gs, gs2))
    assert torch.equal(ga.flat, ga2.flat) and torch.equal(ga.stats, ga2.stats) and torch.equal(aout, aout2) and torch.equal(dq, dq2)
    if n_blocks:
        _check_critics(dt, c, crs, 3, what + ('n_blocks = 3',))
        ga3, aout3, dq3 = _check_actor(dt, c, pol, crs[0], 3, what + ('n_blocks = 3',))
        assert torch.equal(aout3, aout) and torch.equal(dq3, dq)           # a row's own values do not depend on the grid


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('mean_mode', og.MEAN_MODES)
@pytest.mark.parametrize('i', range(len(og.SHAPE_CASES)))
def test_shapes(dt, i, mean_mode):
    """Both kinds from CH = 1 to the maximum (DDPG D = 32, k = 8; TD3 n1 = 32), both activations, with and without
    normalisation and act_scale, both mean modes of the actor; 65 rows: a full tile and a tail."""
    c, pol, crs = _case(dt, og.SHAPE_CASES[i], 65, og.SHAPE_SEEDS[i], mean_mode=mean_mode)
    what = (og.SHAPE_CASES[i], 65, mean_mode)
    if mean_mode == 1:
        _check_critics(dt, c, crs, 0, what)
    _check_actor(dt, c, pol, crs[0], 0, what)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_a_pair_is_two_single_calls_bit_for_bit(dt):
    from rl_on_manifold_amd import critic_gradient
    c, pol, crs = _case(dt, og.ROW_SHAPE, 200, 500)
    pair = _critics(dt, c, crs, 2)
    for j in range(2):
        one = critic_gradient(crs[j], _t(c['obs']), _t(c['action']), _t(c['target']), n_blocks=2)
        assert torch.equal(one.flat, pair[j].flat) and torch.equal(one.stats, pair[j].stats)
    assert not torch.equal(pair[0].flat, pair[1].flat)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_memory_columns_in_place_through_idx(dt):
    """A 300-row ReplayMemory whose reward, next_obs and flag columns hold NaN, as do the rows that idx does not name; idx is
    unsorted with repeats; flat, stats, action_out and dqda_out lie inside poisoned buffers.  Inside the oracle's bound, bit-equal
    to the call on contiguous gathered copies, the poison intact, and with out= a second call allocates nothing."""
    from rl_on_manifold_amd import ReplayMemory, actor_gradient, critic_gradient
    N, M = 300, 130
    c, pol, crs = _case(dt, og.ROW_SHAPE, N, 900, n_idx=M)
    D, k = c['D'], c['k']
    nan = lambda *s: torch.full(s, float('nan'), dtype=DT[dt], device=DEV)          # noqa: E731
    idx = _t(c['idx'])
    assert len(set(c['idx'].tolist())) < M and not np.all(np.diff(c['idx']) >= 0)
    obs, act = _t(c['obs']), _t(c['action'])
    named = torch.zeros(N, dtype=torch.bool, device=DEV)
    named[idx] = True
    obs[~named], act[~named] = float('nan'), float('nan')
    assert int((~named).sum()) > 0
    mem = ReplayMemory(N, D, k, dtype=DT[dt], device=DEV)
    mem.add_fields(obs, act, nan(N), nan(N, D), nan(N), nan(N))
    target = _t(c['target'])
    # ---- the critics
    gs = mem.critic_gradient(crs, idx, target)
    for j, (g, want) in enumerate(zip(gs, c['want_critic'])):
        _inside(dt, g.flat, want, ('memory', 'critic', j))
    cols = mem.columns(idx)
    ref = critic_gradient(crs, cols['obs'].contiguous(), cols['action'].contiguous(), target)
    assert all(torch.equal(a.flat, b.flat) and torch.equal(a.stats, b.stats) for a, b in zip(gs, ref))
    # ---- the actor, its outputs inside padded and poisoned buffers
    abuf, qbuf = torch.full((M, k + 3), -7.0, dtype=DT[dt], device=DEV), torch.full((M, k + 2), -7.0, dtype=DT[dt], device=DEV)
    ga = mem.actor_gradient(pol, crs[0], idx, action_out=abuf[:, 2:2 + k], dqda_out=qbuf[:, 1:1 + k])
    ra, rq = torch.empty((M, k), dtype=DT[dt], device=DEV), torch.empty((M, k), dtype=DT[dt], device=DEV)
    rg = actor_gradient(pol, crs[0], cols['obs'].contiguous(), action_out=ra, dqda_out=rq)
    assert torch.equal(ga.flat, rg.flat) and torch.equal(ga.stats, rg.stats)
    assert torch.equal(abuf[:, 2:2 + k], ra) and torch.equal(qbuf[:, 1:1 + k], rq)
    assert (abuf[:, :2] == -7.0).all() and (abuf[:, 2 + k:] == -7.0).all() and (qbuf[:, :1] == -7.0).all() and (qbuf[:, 1 + k:] == -7.0).all()
    frm = og.actor_gradient(c['actor'], c['critics'][0], c['obs'], c['mean_mode'], c['idx'], dqda=rq.cpu().numpy().astype(np.float64))
    _inside(dt, ga.flat, frm, ('memory', 'actor'))
    # ---- poison around flat and stats: the views of an out= whose buffers lie inside larger ones
    for g in list(gs) + [ga]:
        n = g.flat.numel()
        big, bst = torch.full((n + 64,), -7.0, dtype=DT[dt], device=DEV), torch.full((12,), -7.0, dtype=DT[dt], device=DEV)
        want_flat, want_stats = g.flat.clone(), g.stats.clone()
        g.flat, g.stats = big[32:32 + n], bst[4:8]
        if g is ga:
            mem.actor_gradient(pol, crs[0], idx, out=ga)
        g._poison = (big, bst, want_flat, want_stats)
    mem.critic_gradient(crs, idx, target, out=gs)
    for g in list(gs) + [ga]:
        big, bst, want_flat, want_stats = g._poison
        n = want_flat.numel()
        assert torch.equal(big[32:32 + n], want_flat) and torch.equal(bst[4:8], want_stats)
        assert (big[:32] == -7.0).all() and (big[32 + n:] == -7.0).all() and (bst[:4] == -7.0).all() and (bst[8:] == -7.0).all()
    # ---- out= reuse allocates nothing
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    mem.critic_gradient(crs, idx, target, out=gs)
    mem.actor_gradient(pol, crs[0], idx, out=ga, action_out=abuf[:, 2:2 + k], dqda_out=qbuf[:, 1:1 + k])
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    st = mem.storage
    assert all(torch.isnan(st[:, mem.fields[n]]).all() for n in ('reward', 'next_obs', 'absorbing', 'last'))


class _CriticNet(torch.nn.Module):
    def __init__(self, cr):
        super().__init__()
        n1, k = cr['W1'].shape[1], cr['W2a'].shape[1]
        self._h1, self._h2_s, self._h2_a, self._h3 = (torch.nn.Linear(n1, 64), torch.nn.Linear(64, 64), torch.nn.Linear(k, 64, bias=False),
                                                      torch.nn.Linear(64, 1))
        with torch.no_grad():
            for lay, W, b in ((self._h1, 'W1', 'b1'), (self._h2_s, 'W2', 'b2'), (self._h3, 'W3', 'b3'), (self._h2_a, 'W2a', None)):
                lay.weight.copy_(torch.from_numpy(cr[W]))
                if b:
                    lay.bias.copy_(torch.from_numpy(cr[b]))


def test_hand_over_to_torch_adam_and_to_the_device_adam():
    """QGradients.to_module makes torch.optim.Adam.step() work on a module of the reference's layer names; the device Adam of
    optim.py accepts the actor's Gradients for a group without log_std, and the stepped parameters are those of
    tests/optim_oracle.py applied to g.flat read back, inside that module's own float32 bound."""
    from rl_on_manifold_amd import Adam, MlpPolicy, QCritic
    c, pol, crs = _case('f32', og.ROW_SHAPE, 200, 500)
    net = _CriticNet(c['critics'][0]).to(DEV)
    cr = QCritic.from_module(net, c['D'])
    cr.tensors.update(act_scale=_t(c['critics'][0]['act_scale']), obs_shift=_t(c['critics'][0]['obs_shift']),
                      obs_scale=_t(c['critics'][0]['obs_scale']))
    g = _critics('f32', c, cr)
    _inside('f32', g.flat, c['want_critic'][0], ('from_module',))
    g.to_module(net)
    opt = torch.optim.Adam(net.parameters(), lr=3e-4)
    before = [p.detach().clone() for p in net.parameters()]
    opt.step()
    assert all(p.grad is not None and not torch.equal(p, b) for p, b in zip(net.parameters(), before))
    assert net._h2_a.weight.grad.data_ptr() == g.W2a.data_ptr()
    # ---- the actor: a fresh policy whose tensors the device Adam steps in place
    a = c['actor']
    mine = MlpPolicy(*(_t(a[k]).clone() for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')), obs_shift=_t(a['obs_shift']),
                     obs_scale=_t(a['obs_scale']), activation=a['activation'])
    mine.mean_mode, mine.tensors['act_scale'] = 1, _t(a['act_scale'])
    ga, _, _ = _actor('f32', c, mine, crs[0])
    adam = Adam([{'net': mine}], lr=po.LR)
    p0 = np.concatenate([a[k].reshape(-1) for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')])
    grad = ga.flat.cpu().numpy()
    adam.step(ga)
    got = np.concatenate([mine.tensors[k].cpu().numpy().reshape(-1) for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')]).astype(np.float64)
    zero = np.zeros_like(p0)
    want = po.step64(p0, grad, zero, zero, po.fresh_head())
    bound = po.bound32(p0, grad, zero, zero, po.fresh_head())
    assert (np.abs(got - want['p']) <= bound['p']).all() and not np.array_equal(got, p0.astype(np.float64))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_graph_capture_of_both_calls(dt):
    """Both calls with out=: a linear chain on one stream.  The replay gives the bits of the eager call, on inputs that changed
    after the capture."""
    from rl_on_manifold_amd import actor_gradient, critic_gradient
    c, pol, crs = _case(dt, og.ROW_SHAPE, 200, 500)
    obs, act, tgt = _t(c['obs']), _t(c['action']), _t(c['target'])
    gs = critic_gradient(crs, obs, act, tgt)
    aout, dq = torch.empty((200, c['k']), dtype=DT[dt], device=DEV), torch.empty((200, c['k']), dtype=DT[dt], device=DEV)
    ga = actor_gradient(pol, crs[0], obs, action_out=aout, dqda_out=dq)

    def step():
        critic_gradient(crs, obs, act, tgt, out=gs)
        actor_gradient(pol, crs[0], obs, out=ga, action_out=aout, dqda_out=dq)

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    outs = lambda: [t.clone() for t in (gs[0].flat, gs[1].flat, gs[0].stats, ga.flat, ga.stats, aout, dq)]          # noqa: E731
    first = outs()
    obs.mul_(0.5)
    tgt.add_(0.25)
    step()
    eager = outs()
    for t in (gs[0].flat, gs[1].flat, ga.flat, aout, dq):
        t.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    replayed = outs()
    assert all(torch.equal(a, b) for a, b in zip(eager, replayed))
    assert not torch.equal(first[0], eager[0]) and not torch.equal(first[3], eager[3])


def test_refusals():
    from rl_on_manifold_amd import MlpPolicy, QCritic, actor_gradient, critic_gradient
    c, pol, crs = _case('f32', og.ROW_SHAPE, 16, 316)
    obs, act, tgt = _t(c['obs']), _t(c['action']), _t(c['target'])
    wide = og.oo.case(seed=1, rows=4, **dict(zip(og.SHAPE_KEYS, (og.TD3, 25, 8, 'relu', False, False))))
    w = wide['critics'][0]
    wcr = QCritic(*(_t(w[k]) for k in ('W1', 'b1', 'W2', 'b2', 'W2a', 'W3', 'b3')), kind='td3')
    with pytest.raises(ValueError, match='n1 = 33'):
        critic_gradient(wcr, _t(wide['next_obs']), _t(wide['action']), torch.zeros(4, device=DEV))
    lin = lambda o, i: (torch.zeros(o, i, device=DEV), torch.zeros(o, device=DEV))          # noqa: E731
    small = MlpPolicy(*lin(64, c['D']), *lin(64, 64), *lin(c['k'] - 1, 64))
    with pytest.raises(ValueError, match='the actor maps 18 to 6'):
        actor_gradient(small, crs[0], obs)
    with pytest.raises(ValueError, match='critic must be a QCritic'):
        actor_gradient(pol, pol, obs)
    with pytest.raises(ValueError, match='one QCritic or a pair'):
        critic_gradient(pol, obs, act, tgt)
    with pytest.raises(ValueError, match='target must be a tensor of shape'):
        critic_gradient(crs, obs, act, tgt[:5])
    g = critic_gradient(crs[0], obs, act, tgt)
    with pytest.raises(ValueError, match='out must be the QGradients'):
        critic_gradient(crs, obs, act, tgt, out=g)
