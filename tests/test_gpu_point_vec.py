"""GPU tests of the collision-avoidance task driven step by step without the host in the loop (libatacom_point_vec.so):
the masked step through BatchedPointReachEnv.step(mask=...) and VectorizedPointReachEnv, the checkpoint through snapshot() /
restore(), and GraphedRollout on the task.

Every bound is EQUALITY (torch.equal, == on the logs): the comparator is the plain step or rollout of the same build
(libatacom_point.so) on a twin engine of the same configuration, seed and inputs.  A masked-in lane runs the source of
k_point_step, the generator is keyed by the environment's own counters, and the statistics are accumulated per environment
in the order of its own steps, so nothing here has a tolerance.

Shapes.  B = 333 environments are two workgroups of 256, the second with one full wave and one of 13 live lanes.  Horizon 5
with auto_reset: 12 steps cross two resets inside the kernel.  All inputs are seeded on the CPU."""
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
DT = {'f32': torch.float32, 'f64': torch.float64}
B, H, STEPS = 333, 5, 12
CONFIGS = [(n, dt, rw) for n in (2, 4) for dt in ('f32', 'f64') for rw in (True, False)]
IDS = ['n%d-%s-%s' % (n, dt, 'walk' if rw else 'circle') for n, dt, rw in CONFIGS]
config = pytest.mark.parametrize('n,dt,rw', CONFIGS, ids=IDS)
supplied_draws = pytest.mark.parametrize('supplied', [False, True], ids=['generator', 'draws'])


def _env(n, dt, rw, seed=6, batch=B, horizon=H, reset=True):
    from rl_on_manifold_amd import BatchedPointReachEnv
    env = BatchedPointReachEnv(batch, n_objects=n, random_walk=rw, horizon=horizon, seed=seed, auto_reset=True, device=DEV,
                               dtype=DT[dt])
    if reset:
        env.reset()
    return env


def _inputs(n, dt, supplied, steps=STEPS, batch=B, seed=0):
    """actions [steps, batch, 2] in (-1.2, 1.2) and, when supplied, random-walk draws [steps, batch, n, 2] in (-1, 1)"""
    g = torch.Generator().manual_seed(seed)
    acts = (torch.rand((steps, batch, 2), dtype=torch.float64, generator=g) * 2.4 - 1.2).to(DT[dt]).to(DEV)
    draws = (torch.rand((steps, batch, n, 2), dtype=torch.float64, generator=g) * 2 - 1).to(DT[dt]).to(DEV) if supplied else None
    return acts, draws


def _partial_mask(batch=B, seed=11):
    return (torch.rand((batch,), generator=torch.Generator().manual_seed(seed)) < 0.6).to(DEV)


def _same(a, b, rows=slice(None)):
    """two results of step(): observation, reward and both flags"""
    return (torch.equal(a[0][rows], b[0][rows]) and torch.equal(a[1][rows], b[1][rows]) and torch.equal(a[2][rows], b[2][rows])
            and torch.equal(a[3]['last'][rows], b[3]['last'][rows]))


def _row(d, t):
    return None if d is None else d[t]


@config
@supplied_draws
def test_a_mask_of_ones_is_the_plain_step(n, dt, rw, supplied):
    masked, plain = _env(n, dt, rw), _env(n, dt, rw)
    acts, draws = _inputs(n, dt, supplied)
    ones = torch.ones(B, dtype=torch.uint8, device=DEV)
    lasts = 0
    for t in range(STEPS):
        got, want = masked.step(acts[t], draws=_row(draws, t), mask=ones), plain.step(acts[t], draws=_row(draws, t))
        assert _same(got, want), t
        assert torch.equal(masked.get_state(), plain.get_state()), t
        lasts += int(got[3]['last'].sum())
    assert lasts == 2 * B                                            # horizon 5: steps 5 and 10 ended an episode everywhere
    assert masked.get_constraints_logs(clear=False) == plain.get_constraints_logs(clear=False)


@config
@supplied_draws
def test_a_fixed_partial_mask(n, dt, rw, supplied):
    """Masked-in rows are the unmasked twin's, bit for bit, across two auto-resets; masked-out rows do not move, report their
    current observation, and their action and draw rows -- NaN here -- are not read."""
    env, twin = _env(n, dt, rw), _env(n, dt, rw)
    mask = _partial_mask()
    out = ~mask
    assert 0.4 * B < int(mask.sum()) < 0.8 * B
    acts, draws = _inputs(n, dt, supplied)
    nobody = torch.zeros(B, dtype=torch.uint8, device=DEV)
    for t in range(STEPS):
        a, d = acts[t].clone(), None if draws is None else draws[t].clone()
        a[out] = float('nan')
        if d is not None:
            d[out] = float('nan')
        st0, obs0 = env.get_state(), env.reset(mask=nobody)
        got, want = env.step(a, draws=d, mask=mask), twin.step(acts[t], draws=_row(draws, t))
        assert _same(got, want, mask), t
        st1 = env.get_state()
        assert torch.equal(st1[mask], twin.get_state()[mask]), t
        assert torch.equal(st1[out], st0[out]), t
        assert torch.equal(got[0][out], obs0[out]) and not torch.isnan(got[0]).any(), t
        assert (got[1][out] == 0).all() and not got[2][out].any() and not got[3]['last'][out].any(), t
    assert not torch.isnan(env.get_state()).any()
    assert int(env.get_state()[mask][:, -2].min()) == 3              # episodes started: the first reset and two in the kernel


@config
@supplied_draws
def test_varying_masks_count_every_environments_own_steps(n, dt, rw, supplied):
    """24 calls, every environment active in exactly 12 of them, environment b receiving row j of the inputs at ITS j-th active
    call: its outputs there are row [j, b] of a twin's 12-step rollout, and at the end the two engines are equal -- state,
    counters and the constraint log, to which each environment added the same terms in the same order."""
    env, twin = _env(n, dt, rw), _env(n, dt, rw)
    acts, draws = _inputs(n, dt, supplied)
    g = torch.Generator().manual_seed(5)
    calls = 2 * STEPS
    active = torch.zeros((calls, B), dtype=torch.bool)
    for b in range(B):
        active[torch.randperm(calls, generator=g)[:STEPS], b] = True
    assert (active.sum(0) == STEPS).all() and 0 < int(active.sum(1).min()) and int(active.sum(1).max()) < B
    own = (torch.cumsum(active.long(), 0) - 1).clamp_(min=0).to(DEV)          # [calls, B]: the environment's own step index
    active = active.to(DEV)
    cols = torch.arange(B, device=DEV)
    ref = twin.rollout(acts, draws=draws)
    got = {k: torch.full_like(ref[k], 77) for k in ('next_obs', 'reward', 'absorbing', 'last')}
    for c in range(calls):
        m, j = active[c], own[c]
        a = acts[j, cols].clone()
        a[~m] = float('nan')
        d = None
        if draws is not None:
            d = draws[j, cols].clone()
            d[~m] = float('nan')
        obs, r, ab, info = env.step(a, draws=d, mask=m)
        got['next_obs'][j[m], cols[m]] = obs[m]
        got['reward'][j[m], cols[m]] = r[m]
        got['absorbing'][j[m], cols[m]] = ab[m].to(torch.uint8)
        got['last'][j[m], cols[m]] = info['last'][m].to(torch.uint8)
    for k in got:
        assert torch.equal(got[k], ref[k]), k
    assert int(ref['last'].sum()) == 2 * B
    assert torch.equal(env.get_state(), twin.get_state())
    assert env.get_constraints_logs(clear=False) == twin.get_constraints_logs(clear=False)


def _run(env, acts, draws, first=0, steps=7):
    """`steps` steps from row `first` of the inputs -> their outputs, stacked"""
    outs = [env.step(acts[first + t], draws=_row(draws, first + t)) for t in range(steps)]
    return (torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs]), torch.stack([o[2] for o in outs]),
            {'last': torch.stack([o[3]['last'] for o in outs])})


@config
def test_snapshot_and_restore(n, dt, rw):
    """restore(snapshot()) puts back what set_state(get_state()) cannot -- the constraint log -- and the generator key."""
    env = _env(n, dt, rw)
    acts, _ = _inputs(n, dt, False)
    _run(env, acts, None, 0, 3)                                      # a log that is not empty, an episode under way
    image, st0, logs0 = env.snapshot(), env.get_state(), env.get_constraints_logs(clear=False)
    first = _run(env, acts, None, 3)
    st1, logs1 = env.get_state(), env.get_constraints_logs(clear=False)
    assert logs1 != logs0 and not torch.equal(st1, st0)
    # the state row alone: the log stays where the seven steps left it
    env.set_state(st0)
    assert torch.equal(env.get_state(), st0) and env.get_constraints_logs(clear=False) == logs1
    env.set_state(st1)
    # the image: everything
    env.restore(image)
    assert torch.equal(env.get_state(), st0) and env.get_constraints_logs(clear=False) == logs0
    assert _same(_run(env, acts, None, 3), first)
    assert torch.equal(env.get_state(), st1) and env.get_constraints_logs(clear=False) == logs1
    # into a handle created with another seed: it adopts the key and continues identically (resets in the kernel included)
    other = _env(n, dt, rw, seed=41, reset=False)
    other.restore(image)
    assert other.cfg.seed == env.cfg.seed == 6
    assert torch.equal(other.get_state(), st0) and other.get_constraints_logs(clear=False) == logs0
    assert _same(_run(other, acts, None, 3), first)
    assert torch.equal(other.get_state(), st1) and other.get_constraints_logs(clear=False) == logs1
    assert int(first[3]['last'].sum()) >= B                          # steps 3..9 cross the horizon of 5


@config
def test_restore_refuses_an_image_of_another_handle_and_writes_nothing(n, dt, rw):
    from rl_on_manifold_amd import AtacomError
    env, control = _env(n, dt, rw), _env(n, dt, rw)
    acts, _ = _inputs(n, dt, False)
    for e in (env, control):
        _run(e, acts, None, 0, 3)
    corrupt = env.snapshot().clone()
    corrupt[4:8] = torch.tensor([99, 0, 0, 0], dtype=torch.uint8, device=DEV)         # the format number
    not_an_image = torch.zeros_like(corrupt)
    images = [('n_objects', 'image n_objects = %d, handle %d' % (6 - n, n), _env(6 - n, dt, rw, seed=9).snapshot()),
              ('dtype', 'image dtype = ', _env(n, 'f64' if dt == 'f32' else 'f32', rw, seed=9).snapshot()),
              ('batch', 'image batch = %d, handle %d' % (B - 1, B), _env(n, dt, rw, seed=9, batch=B - 1).snapshot()),
              ('format', 'image format = 99', corrupt), ('magic', 'bad magic', not_an_image)]
    for t, (field, text, image) in enumerate(images):
        with pytest.raises(AtacomError, match=field) as err:
            env.restore(image)
        assert text in str(err.value), (field, str(err.value))
        assert env.cfg.seed == 6
        assert torch.equal(env.get_state(), control.get_state()), field
        assert env.get_constraints_logs(clear=False) == control.get_constraints_logs(clear=False), field
        assert _same(env.step(acts[3 + t]), control.step(acts[3 + t])), field         # the generator key is the old one too
    with pytest.raises(ValueError):
        env.restore(env.snapshot()[:-16].clone())                    # a valid header on a buffer that is cut short
    with pytest.raises(ValueError):
        env.restore(env.snapshot().cpu())
    assert torch.equal(env.get_state(), control.get_state())


def test_a_masked_step_and_a_snapshot_are_capturable():
    """No host synchronisation in step_all or snapshot: each is captured in a (linear) HIP graph and replayed."""
    from rl_on_manifold_amd import VectorizedPointReachEnv
    N = 64
    venv, twin = (VectorizedPointReachEnv(N, horizon=50, seed=2, device=DEV) for _ in range(2))
    assert venv.number == N and venv.info.horizon == 50 and venv.engine.batch == N
    m = torch.ones(N, dtype=torch.bool)
    m[::3] = False
    m = m.to(DEV)
    act = torch.full((N, 2), 0.25, device=DEV)
    for v in (venv, twin):
        obs, info = v.reset_all()
        assert tuple(obs.shape) == (N, 20) and info == {}
        v.step_all(m, act)                                           # warm-up outside the capture
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        captured = venv.step_all(m, act)
    before = venv.engine.get_state().clone()
    assert torch.equal(before, twin.engine.get_state())              # the capture ran nothing
    for rep in range(2):
        gr.replay()
        torch.cuda.synchronize()
        want = twin.step_all(m, act)
        assert _same(captured, want), rep
    after = venv.engine.get_state()
    assert torch.equal(after, twin.engine.get_state())
    assert torch.equal(after[::3], before[::3])
    assert (after[1::3] != before[1::3]).any(dim=1).all() and (after[2::3] != before[2::3]).any(dim=1).all()
    assert venv.get_constraints_logs() == twin.get_constraints_logs()
    # the checkpoint: captured once, every replay saves the state of that moment
    eng = venv.engine
    image = torch.empty_like(eng.snapshot())
    torch.cuda.synchronize()
    gs = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gs):
        eng.snapshot(out=image)
    for rep in range(2):
        venv.step_all(m, act)
        kept, logs = eng.get_state().clone(), eng.get_constraints_logs(clear=False)
        gs.replay()
        venv.step_all(None, act)
        assert not torch.equal(eng.get_state(), kept)
        eng.restore(image)
        assert torch.equal(eng.get_state(), kept) and eng.get_constraints_logs(clear=False) == logs, rep


@config
def test_graphed_rollout_on_the_task(n, dt, rw):
    """GraphedRollout: observe -> torch policy -> step, T times in one HIP graph.  With a deterministic policy that depends on
    the observation it reproduces `rollout()` of a twin fed the actions it chose (auto-resets included) and the twin's
    constraint log, replay after replay; building it leaves the engine where it was."""
    from rl_on_manifold_amd import GraphedRollout
    Bg, T = 300, 14
    env, twin = _env(n, dt, rw, batch=Bg, horizon=6), _env(n, dt, rw, batch=Bg, horizon=6)
    D = env.obs_dim
    W = (torch.randn((D, 2), dtype=torch.float64, generator=torch.Generator().manual_seed(7)) * 0.5).to(DT[dt]).to(DEV)

    def policy(obs):                       # any capturable torch code
        return torch.tanh((obs * 0.1) @ W) * 1.2

    st, logs = env.get_state(), env.get_constraints_logs(clear=False)
    loop = GraphedRollout(env, policy, T)
    assert torch.equal(env.get_state(), st)
    got = env.get_constraints_logs(clear=False)
    assert got[1:] == logs[1:] and (got[0] == logs[0] or (got[0] != got[0] and logs[0] != logs[0]))   # an empty log's mean is nan
    start, twin_start = env.snapshot(), twin.snapshot()
    for rep in range(2):
        env.restore(start)
        twin.restore(twin_start)
        data = loop.replay()
        torch.cuda.synchronize()
        acts = data['action'].clone()
        ref = twin.rollout(acts)
        for key in ('obs', 'next_obs', 'reward', 'last', 'absorbing'):
            assert torch.equal(data[key], ref[key]), (rep, key)
        assert torch.allclose(acts, policy(data['obs'].reshape(T * Bg, D)).reshape(T, Bg, 2), atol=1e-6)
        assert data['last'][5].all() and data['last'][11].all() and int(data['last'].sum()) == 2 * Bg
        assert not torch.equal(data['obs'][6], data['next_obs'][5])              # the reset state, not the terminal one
        assert torch.equal(env.get_state(), twin.get_state()), rep
        assert env.get_constraints_logs(clear=False) == twin.get_constraints_logs(clear=False), rep


def test_mask_normalisation_and_argument_checks():
    from rl_on_manifold_amd import VectorizedPointReachEnv
    N = 70
    keep = torch.rand((N,), generator=torch.Generator().manual_seed(3)) < 0.5
    masks = {'bool': keep.to(DEV), 'uint8': keep.to(torch.uint8).to(DEV), 'int64': (keep.long() * 5).to(DEV),
             'host bool': keep, 'list': keep.tolist()}
    act = (torch.rand((N, 2), generator=torch.Generator().manual_seed(4)) * 2 - 1).to(DEV)
    results = {}
    for kind, m in masks.items():
        v = VectorizedPointReachEnv(N, n_objects=2, horizon=9, seed=1, device=DEV)
        v.reset_all()
        for _ in range(3):
            out = v.step_all(m, act)
        results[kind] = (out, v.engine.get_state())
    for kind, (out, st) in results.items():
        assert _same(out, results['bool'][0]) and torch.equal(st, results['bool'][1]), kind
    # a partial reset_all: the masked-out environments keep their state
    before = v.engine.get_state().clone()
    obs, _ = v.reset_all(masks['int64'])
    after = v.engine.get_state()
    kd = keep.to(DEV)
    assert torch.equal(after[~kd], before[~kd]) and (after[kd][:, -3] == 0).all() and (before[kd][:, -3] == 3).all()
    assert torch.equal(obs, after[:, :v.engine.obs_dim])
    for bad in (torch.ones(N + 1, dtype=torch.bool, device=DEV), torch.ones((N, 1), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            v.step_all(bad, act)
        with pytest.raises(ValueError):
            v.engine.step(act, mask=bad)
    # step_into reads raw pointers: a strided, host or bool mask raises instead of being misread
    eng = v.engine
    good = dict(actions=act, obs=torch.empty((N, eng.obs_dim), device=DEV), reward=torch.empty((N,), device=DEV),
                absorbing=torch.empty((N,), device=DEV, dtype=torch.uint8), last=torch.empty((N,), device=DEV, dtype=torch.uint8))
    eng.step_into(mask=masks['uint8'], **good)
    eng.step_into(mask=masks['uint8'], **good)                       # second call: the cached fast path
    for bad in (torch.ones(2 * N, dtype=torch.uint8, device=DEV)[::2], torch.ones(N, dtype=torch.uint8), masks['bool'],
                torch.ones(N - 1, dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError):
            eng.step_into(mask=bad, **good)
    # ... and with a mask it makes the step that step() makes
    st = eng.snapshot()
    eng.step_into(mask=masks['uint8'], **good)
    after_into = eng.get_state()
    eng.restore(st)
    out = eng.step(act, mask=masks['uint8'])
    assert torch.equal(out[0], good['obs']) and torch.equal(out[1], good['reward']) and torch.equal(eng.get_state(), after_into)
    assert torch.equal(out[3]['last'].view(torch.uint8), good['last'])
