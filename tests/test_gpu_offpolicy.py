"""GPU tests of libatacom_offpolicy.so (rl_on_manifold_amd/offpolicy.py): the critic's Q-value and the fused TD target against
the float64 oracle (tests/offpolicy_oracle.py), float32 inside its derived bound on EVERY sample and float64 to 1e-12 of the
output's scale; row counts around the 16-row block and the 64-row tile, one and several rounds of phases per workgroup; every
CH = ceil(n1 / 4) path of both critic kinds; the target's modes; the columns of a replay memory read in place through an
unsorted idx with repeats, NaN where the call must not read and poison around the outputs; the replay memory against plain
indexing; the soft update bit for bit against numpy; graph capture.  Shapes are the smallest at which the kernels can go wrong."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import offpolicy_oracle as oo                                 # noqa: E402

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
    """(case, policy, critics, the oracle's target, the oracle's q of the recorded actions), computed once."""
    key = (dt, shape, rows, seed, tuple(sorted(kw.items())))
    if key not in _cache:
        c = oo.case(seed=seed, rows=rows, dtype=NP[dt], **dict(zip(oo.SHAPE_KEYS, shape)), **kw)
        pol, crs = _objects(c)
        _cache[key] = (c, pol, crs, oo.case_target(c), oo.critic_q(c['critics'][0], c['next_obs'], c['action']))
    return _cache[key]


def _inside(dt, got, want, e32, scale, what):
    """float32: |error| <= the oracle's bound; float64: <= 1e-12 scale + 1e-14, on every sample."""
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), what
    bound = e32 if dt == 'f32' else 1e-12 * scale + 1e-14
    err = np.abs(got - want)
    worst = float((err / bound).max())
    print('%s %s: worst |error| / bound %.4f, worst |error| %.3g' % (what, dt, worst, err.max()))
    assert (err <= bound).all(), (what, dt, 'worst |error| / bound %.3f on %d of %d samples' % (worst, int((err > bound).sum()), err.size))


def _target(c, pol, crs, n_blocks=0, **kw):
    from rl_on_manifold_amd import td_target
    return td_target(pol, crs, _t(c['next_obs']), _t(c['reward']), _t(c['absorbing']), c['gamma'], eps=_t(c['eps']),
                     noise_std=c['noise_std'], noise_clip=c['noise_clip'], low=_t(c['low']), high=_t(c['high']), n_blocks=n_blocks, **kw)


def _check(dt, shape, rows, seed, n_blocks=0, **kw):
    """q_values and td_target of a case against the oracle -> (q, y, a'')."""
    from rl_on_manifold_amd import q_values
    c, pol, crs, ref, (q_ref, e_q, s_q) = _case(dt, shape, rows, seed, **kw)
    q = q_values(crs[0], _t(c['next_obs']), _t(c['action']), n_blocks=n_blocks)
    _inside(dt, q, q_ref, e_q, s_q, (shape, rows, n_blocks, 'q'))
    aout = torch.full((rows, shape[2]), float('nan'), dtype=DT[dt], device=DEV)
    y = _target(c, pol, crs, n_blocks, action_out=aout)
    _inside(dt, y, ref['y'], ref['e_y'], ref['scale_y'], (shape, rows, n_blocks, 'y'))
    _inside(dt, aout, ref['a'], ref['e_a'], ref['scale_a'], (shape, rows, n_blocks, 'action_out'))
    # the critic half from the device's own a'': the sharper float32 bound (offpolicy_oracle.target_from_action)
    y2, e2 = oo.target_from_action(c['critics'], c['next_obs'], aout.cpu().numpy(), c['reward'], c['absorbing'], c['gamma'], NP[dt])
    _inside(dt, y, y2, e2, ref['scale_y'], (shape, rows, n_blocks, 'y from the device action'))
    return q, y, aout


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('rows,n_blocks', oo.ROW_CASES)
def test_row_counts_and_grids(dt, rows, n_blocks):
    """1 .. 600 rows: a lone row, a part-filled 16-block, a tail wave, 200 rows walked by one and by two workgroups, and 600 by
    one, whose wavefronts walk up to three rounds of the three phases.  An explicit n_blocks gives the bits of the automatic one."""
    q, y, a = _check(dt, oo.ROW_SHAPE, rows, 7, n_blocks)
    if n_blocks:
        q0, y0, a0 = _check(dt, oo.ROW_SHAPE, rows, 7, 0)
        assert torch.equal(q, q0) and torch.equal(y, y0) and torch.equal(a, a0)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('i', range(len(oo.SHAPE_CASES)))
def test_shapes(dt, i):
    """Both kinds from CH = 1 to the maximum (DDPG D = 32, k = 8; TD3 n1 = 32), both activations, with and without
    normalisation and act_scale; 65 rows: a full tile and a tail."""
    _check(dt, oo.SHAPE_CASES[i], 65, oo.SHAPE_SEEDS[i])


def test_a_first_layer_wider_than_32_is_refused():
    from rl_on_manifold_amd import AtacomError, q_values
    c = oo.case(seed=1, rows=4, **dict(zip(oo.SHAPE_KEYS, (oo.TD3, 25, 8, 'relu', False, False))))
    _, crs = _objects(c)
    with pytest.raises(AtacomError, match='n1 = n_obs \\+ n_act = 33'):
        q_values(crs[0], _t(c['next_obs']), _t(c['action']))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('name,n_critics,eps,bounds,mean_mode', oo.MODE_CASES)
def test_target_modes(dt, name, n_critics, eps, bounds, mean_mode):
    """DDPG (one critic, no noise, no bounds), TD3 (two critics, clipped noise, bounds), an actor without the squash; asking for
    action_out leaves y's bits."""
    kw = dict(n_critics=n_critics, with_eps=eps, with_bounds=bounds, mean_mode=mean_mode)
    _, y, _ = _check(dt, oo.ROW_SHAPE, 200, 7, **kw)
    c, pol, crs = _case(dt, oo.ROW_SHAPE, 200, 7, **kw)[:3]
    assert torch.equal(_target(c, pol, crs), y)
    if name == 'td3':
        oo.assert_regimes(c)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_memory_columns_in_place_through_idx(dt):
    """Every input is a column of a [40, F] storage in which every column the call must not read holds NaN -- obs, action and
    last for the target; reward, next_obs, absorbing and last for the Q-value -- so a kernel that read a wrong column would
    return NaN; idx is unsorted with repeats; the outputs are strided rows of poisoned buffers.  Bit-equal to the call on
    contiguous gathered copies, nothing outside the views changes, and row r of eps belongs to row r of the call."""
    from rl_on_manifold_amd import ReplayMemory, q_values, td_target
    shape, N, M = (oo.TD3, 4, 2, 'relu', True, True), 40, 70
    c, pol, crs = _case(dt, shape, N, 11)[:3]
    nan = lambda *s: torch.full(s, float('nan'), dtype=DT[dt], device=DEV)          # noqa: E731
    poisoned = lambda mem, names: all(torch.isnan(mem.storage[:, mem.fields[n]]).all() for n in names)      # noqa: E731
    rng = np.random.default_rng(0)
    idx = _t(rng.integers(0, N, M))
    idx[:3] = idx[5]
    eps = _t(rng.uniform(-4, 4, (M, 2)).astype(NP[dt]))
    kw = dict(eps=eps, noise_std=0.2, noise_clip=0.5, low=_t(c['low']), high=_t(c['high']))
    # ---- the target reads next_obs, reward and absorbing: obs, action and last are NaN
    mem = ReplayMemory(N, 4, 2, dtype=DT[dt], device=DEV)
    mem.add_fields(nan(N, 4), nan(N, 2), _t(c['reward']), _t(c['next_obs']), _t(c['absorbing']), nan(N))
    assert mem.size == N and mem.head == 0 and poisoned(mem, ('obs', 'action', 'last'))
    # contiguous gathered copies
    g = {k: v.contiguous() for k, v in mem.columns(idx).items()}
    a_ref = torch.empty((M, 2), dtype=DT[dt], device=DEV)
    y_ref = td_target(pol, crs, g['next_obs'], g['reward'], g['absorbing'], 0.99, action_out=a_ref, **kw)
    # in place, into padded and poisoned outputs
    ybuf, abuf = torch.full((M, 3), -7.0, dtype=DT[dt], device=DEV), torch.full((M, 5), -7.0, dtype=DT[dt], device=DEV)
    y = mem.td_target(pol, crs, idx, 0.99, out=ybuf[:, 1], action_out=abuf[:, 2:4], **kw)
    assert torch.equal(y, y_ref) and torch.equal(abuf[:, 2:4], a_ref)
    assert (ybuf[:, [0, 2]] == -7.0).all() and (abuf[:, [0, 1, 4]] == -7.0).all()
    assert torch.isfinite(y).all() and torch.isfinite(a_ref).all()
    # eps follows r: permuting idx alone changes which noise a memory row meets
    perm = torch.flip(torch.arange(M, device=DEV), [0])
    y_perm = mem.td_target(pol, crs, idx[perm].contiguous(), 0.99, eps=eps[perm].contiguous(), **{k: v for k, v in kw.items() if k != 'eps'})
    assert torch.equal(y_perm, y[perm])
    # ReplayMemory.td_target(idx) is td_target on columns(idx)
    g = mem.columns(idx)
    assert torch.equal(mem.td_target(pol, crs, idx, 0.99), td_target(pol, crs, g['next_obs'], g['reward'], g['absorbing'], 0.99))
    assert poisoned(mem, ('obs', 'action', 'last'))
    # ---- the Q-value reads obs and action (next_obs of the case serves as obs): reward, next_obs, absorbing and last are NaN
    mem = ReplayMemory(N, 4, 2, dtype=DT[dt], device=DEV)
    mem.add_fields(_t(c['next_obs']), _t(c['action']), nan(N), nan(N, 4), nan(N), nan(N))
    assert poisoned(mem, ('reward', 'next_obs', 'absorbing', 'last'))
    qbuf = torch.full((M, 2), -7.0, dtype=DT[dt], device=DEV)
    q = mem.q_values(crs[0], idx, out=qbuf[:, 0])
    g = mem.columns(idx)
    assert torch.equal(q, q_values(crs[0], g['obs'].contiguous(), g['action'].contiguous())) and (qbuf[:, 1] == -7.0).all()
    assert torch.isfinite(q).all()


# ------------------------------------------------------------------------------------------------------------ replay memory
def _records(T, B, Bm, D, k, seed, dtype=torch.float32):
    """Full records [T, Bm, F] with NaN in the padding rows, and the unpacked fields of the real rows."""
    from rl_on_manifold_amd import RecordLayout
    lay = RecordLayout([B], D, k)
    g = torch.Generator().manual_seed(seed)
    rec = torch.randn(T, Bm, lay.F, generator=g).to(dtype)
    rec[..., lay.fields['absorbing']] = (torch.rand(T, Bm, generator=g) < 0.3).to(dtype)
    rec[..., lay.fields['last']] = (torch.rand(T, Bm, generator=g) < 0.3).to(dtype)
    rec[:, B:] = float('nan')
    return lay, rec.to(DEV)


def _restate(store, head, rows):
    """Plain indexing: row j of a collection -> slot (head + j) mod capacity, in order (a later row wins)."""
    cap = store.shape[0]
    for j in range(rows.shape[0]):
        store[(head + j) % cap] = rows[j]
    return (head + rows.shape[0]) % cap


def test_replay_memory_is_plain_indexing():
    from rl_on_manifold_amd import ReplayMemory
    T, B, Bm, D, k = 3, 5, 8, 4, 2
    lay, rec = _records(T, B, Bm, D, k, 1)
    rows = rec[:, :B].reshape(-1, lay.F)
    # capacity 32, head = 29: wrap
    mem = ReplayMemory(32, D, k, device=DEV)
    want, head = torch.zeros(32, lay.F, device=DEV), 0
    for _ in range(2):
        mem.add(lay, rec)
        head = _restate(want, head, rows)
    assert mem.head == head == 30 and mem.size == 30
    mem.head = head = 29
    mem.add(lay, rec)
    head = _restate(want, head, rows)
    assert mem.head == head == 12 and mem.size == 32 and torch.equal(mem.storage, want) and not torch.isnan(mem.storage).any()
    assert mem.initialized(32) and not mem.initialized(33)
    # capacity 15: exact
    mem = ReplayMemory(15, D, k, device=DEV)
    mem.add(lay, rec.unsqueeze(0))                                   # gathered [W = 1, T, Bm, F]
    assert mem.head == 0 and mem.size == 15 and torch.equal(mem.storage, rows)
    # capacity 7: only the last 7 rows, at the slots the full walk leaves them in; then a wrap
    mem = ReplayMemory(7, D, k, device=DEV)
    want, head = torch.zeros(7, lay.F, device=DEV), 0
    for _ in range(2):
        mem.add(lay, rec)
        head = _restate(want, head, rows)
        assert mem.head == head and mem.size == 7 and torch.equal(mem.storage, want)
    idx = mem.sample(1000, generator=torch.Generator(device=DEV).manual_seed(0))
    assert idx.dtype == torch.int64 and idx.device.type == 'cuda' and int(idx.min()) == 0 and int(idx.max()) == 6
    mem = ReplayMemory(32, D, k, device=DEV)
    mem.add(lay, rec)
    idx = mem.sample(1000)
    assert int(idx.min()) >= 0 and int(idx.max()) < 15
    cols = mem.columns()
    assert cols['obs'].shape == (15, D) and cols['obs'].data_ptr() == mem.storage.data_ptr()            # views
    assert torch.equal(mem.columns(idx[:9])['next_obs'], mem.storage[idx[:9]][:, lay.fields['next_obs']])


def test_replay_memory_from_compact_records():
    """Synthetic exception rows, one of them at a truncated row, and one real collection of an auto-resetting environment: the
    memory holds what CompactRecordLayout.unpack rebuilds."""
    from rl_on_manifold_amd import BatchedAtacomEnv, CompactRecordLayout, ReplayMemory
    T, B, Bm, D, k = 3, 5, 8, 4, 2
    lay = CompactRecordLayout([B], D, k, T)
    g = torch.Generator().manual_seed(2)
    rec = torch.randn(T + 1, Bm, lay.Fc, generator=g)
    rec[..., lay.compact_fields['absorbing']] = 0.0
    rec[..., lay.compact_fields['last']] = 0.0
    rec[0, 1, lay.compact_fields['last']] = 1.0                                              # truncated, not absorbing
    rec[1, 3, lay.compact_fields['last']] = rec[1, 3, lay.compact_fields['absorbing']] = 1.0
    rec[:, B:] = float('nan')
    ends = torch.cat([torch.tensor([[0.0, 1.0], [1.0, 3.0], [9.0, 9.0]]), torch.randn(3, D, generator=g)], 1)      # the third is not valid
    rec, ends = rec.to(DEV), ends.to(DEV)
    mem = ReplayMemory(32, D, k, device=DEV)
    mem.add_compact(lay, rec, ends, 2)
    d = lay.unpack(rec, ends, 2)
    for name, ix in mem.fields.items():
        want = d[name][:, :B].reshape((T * B,) + tuple(d[name].shape[2:])).to(torch.float32)
        assert torch.equal(mem.storage[:T * B][:, ix], want), name
    assert torch.equal(mem.storage[0 * B + 1, lay.fields['next_obs']], ends[0, 2:]) and torch.equal(mem.storage[1 * B + 3, lay.fields['next_obs']], ends[1, 2:])
    assert mem.size == T * B and not torch.isnan(mem.storage).any()
    # a real collection: short episodes, so that ends occur before the last step
    Tr, Br = 8, 6
    env = BatchedAtacomEnv('planar', Br, device=DEV, dtype=torch.float32, horizon=3, auto_reset=True)
    acts = torch.randn(Tr, Br, env.dims['null'], generator=torch.Generator().manual_seed(3)).to(DEV) * 0.3
    rec, ends, n = env.rollout_compact(actions=acts, batch_stride=Br + 2)
    assert n > 0
    layr = CompactRecordLayout([Br], env.obs_dim, env.dims['null'], Tr)
    mem = ReplayMemory(64, env.obs_dim, env.dims['null'], device=DEV)
    mem.add_compact(layr, rec, ends, n)
    d = layr.unpack(rec, ends, n)
    for name, ix in mem.fields.items():
        want = d[name][:, :Br].reshape((Tr * Br,) + tuple(d[name].shape[2:])).to(torch.float32)
        assert torch.equal(mem.storage[:Tr * Br][:, ix], want), name
    env.close()


# -------------------------------------------------------------------------------------------------------------- soft update
def _pairs(dt, cases, seed=0):
    out = []
    for j, (n_in, n_out, n_act) in enumerate(cases):
        t, w = oo.pair_case(seed + j, n_in, n_out, n_act, NP[dt])
        out.append((t, w, tuple(_t(a) for a in t), tuple(_t(a) for a in w)))
    return out


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_soft_update_is_the_numpy_expression_bit_for_bit(dt):
    from rl_on_manifold_amd import soft_update
    tau = 0.005
    pairs = _pairs(dt, oo.PAIR_CASES)
    # all four in one launch
    soft_update([p[2] for p in pairs], [p[3] for p in pairs], tau)
    for t, w, td, wd in pairs:
        for a, b, got, on in zip(t, w, td, wd):
            assert np.array_equal(got.cpu().numpy().view(np.uint8), oo.soft_update(a, b, tau).view(np.uint8))
            assert np.array_equal(on.cpu().numpy(), b)                                        # online untouched
    # four single launches give the same bits; a plain pair and a critic pair alone
    singles = _pairs(dt, oo.PAIR_CASES)
    for p in singles:
        soft_update(p[2], p[3], tau)
    for p, s in zip(pairs, singles):
        assert all(torch.equal(a, b) for a, b in zip(p[2], s[2]))
    # tau = 0 leaves the target's bits, tau = 1 copies the online bits
    for tau01 in (0.0, 1.0):
        t, w, td, wd = _pairs(dt, oo.PAIR_CASES[1:2], seed=5)[0]
        soft_update(td, wd, tau01)
        for a, b, got in zip(t, w, td):
            assert np.array_equal(got.cpu().numpy().view(np.uint8), (b if tau01 else a).view(np.uint8))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_soft_update_repeated_a_thousand_times(dt):
    from rl_on_manifold_amd import soft_update
    t, w, td, wd = _pairs(dt, [(4, 1, 2)], seed=9)[0]
    for _ in range(1000):
        soft_update(td, wd, 1e-3)
    for a, b, got in zip(t, w, td):
        want = a
        for _ in range(1000):
            want = oo.soft_update(want, b, 1e-3)
        assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8))


def test_soft_update_takes_policy_and_critic_objects_and_refuses_overlap():
    from rl_on_manifold_amd import AtacomError, soft_update
    c = oo.case(seed=3, rows=4, **dict(zip(oo.SHAPE_KEYS, oo.ROW_SHAPE)))
    pol, crs = _objects(c)
    pol_t, crs_t = _objects(oo.case(seed=4, rows=4, **dict(zip(oo.SHAPE_KEYS, oo.ROW_SHAPE))))
    before = pol_t.tensors['W1'].clone()
    soft_update([pol_t] + crs_t, [pol] + crs, 0.25)
    want = oo.soft_update(before.cpu().numpy(), pol.tensors['W1'].cpu().numpy(), 0.25)
    assert np.array_equal(pol_t.tensors['W1'].cpu().numpy(), want)
    want = oo.soft_update(oo.case(seed=4, rows=4, **dict(zip(oo.SHAPE_KEYS, oo.ROW_SHAPE)))['critics'][1]['W2a'], c['critics'][1]['W2a'], 0.25)
    assert np.array_equal(crs_t[1].tensors['W2a'].cpu().numpy(), want)
    with pytest.raises(AtacomError, match='overlaps'):
        soft_update(crs_t[0], crs_t[0], 0.5)


def test_td_target_and_soft_update_in_a_graph():
    """td_target followed by soft_update of the target networks, captured on one stream and replayed twice with changed inputs:
    the replays equal the eager calls."""
    from rl_on_manifold_amd import soft_update, td_target
    shape = dict(zip(oo.SHAPE_KEYS, oo.ROW_SHAPE))
    c = oo.case(seed=7, rows=200, **shape)
    pol, crs = _objects(c)                                           # the targets: fresh objects, this test moves them
    pol_on, crs_on = _objects(oo.case(seed=8, rows=200, **shape))
    x0, r0 = _t(c['next_obs']), _t(c['reward'])
    x, r, ab, eps, low, high = x0.clone(), r0.clone(), _t(c['absorbing']), _t(c['eps']), _t(c['low']), _t(c['high'])
    y = torch.empty(200, device=DEV)
    targets = [pol] + crs
    names = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'W2a')
    saved = [{k: o.tensors[k].clone() for k in names if k in o.tensors} for o in targets]

    def step():
        td_target(pol, crs, x, r, ab, 0.99, eps=eps, noise_std=0.2, noise_clip=0.5, low=low, high=high, out=y)
        soft_update(targets, [pol_on] + crs_on, 0.01)

    def restore():
        for o, s in zip(targets, saved):
            for k, t in s.items():
                o.tensors[k].copy_(t)
        x.copy_(x0)
        r.copy_(r0)

    def run(fn):
        out = []
        for rep in range(2):
            x.add_(0.1 * (rep + 1))
            r.mul_(-1.0)
            fn()
            out.append((y.clone(), pol.tensors['W3'].clone(), crs[1].tensors['W2a'].clone()))
        return out

    step()                                                           # warm-up before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    restore()
    eager = run(step)
    restore()
    replayed = run(graph.replay)
    torch.cuda.synchronize()
    for e, g in zip(eager, replayed):
        assert all(torch.equal(a, b) for a, b in zip(e, g))
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[0][2], saved[2]['W2a'])
