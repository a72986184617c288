"""Row N4 on the GPU: rigid-body dynamics of the iiwa + striker chain (inverse dynamics / mass matrix / forward
dynamics primitives, golden set G11 = the reference's URDF) and the opt-in rigid-body env step against the oracle."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import atacom_scalar as osc          # noqa: E402
from oracle import atacom_batched as ob          # noqa: E402
from oracle import dynamics as D                 # noqa: E402

DEV = 'cuda:0'
DT = {'f64': torch.float64, 'f32': torch.float32}
IIWA_INIT_Q = np.array([0.0, 0.7135214629060707, 0.0, -0.5024756033561426, 0.0, 1.9256631778550268])


@pytest.mark.parametrize('dt', ['f64', 'f32'])
def test_inverse_dynamics_and_mass_matrix_against_the_reference_urdf(golden, dt):
    """tau = M ddq + C dq + g and M(q) of the nine-joint chain vs the reference's URDF evaluated link by link (G11).
    float64 1e-10; float32 2e-4 abs on torques of up to ~150 Nm (relative 1e-6), 1e-5 on M entries (composite inertias
    are accumulated about the world origin: m |c|^2 ~ 40 kg m^2 terms cancel down to entries <= ~6 kg m^2)."""
    from rl_on_manifold_amd import inverse_dynamics
    g = golden('iiwa_urdf')
    t = lambda a: torch.tensor(a, device=DEV, dtype=DT[dt])                   # noqa: E731
    tau, M = inverse_dynamics(t(g['dyn_q']), t(g['dyn_dq']), t(g['dyn_ddq']), want_mass_matrix=True)
    tau, M = tau.cpu().numpy().astype(np.float64), M.cpu().numpy().astype(np.float64)
    tol_tau, tol_M = (1e-10, 1e-10) if dt == 'f64' else (2e-4, 1e-5)
    assert np.abs(tau - g['dyn_tau']).max() < tol_tau
    assert np.abs(M - g['dyn_M']).max() < tol_M
    assert np.abs(M - np.swapaxes(M, 1, 2)).max() == 0.0                      # symmetric by construction
    assert np.linalg.eigvalsh(M).min() > 1e-4                                 # positive definite
    grav = inverse_dynamics(t(g['dyn_q']), t(0 * g['dyn_dq']), t(0 * g['dyn_ddq'])).cpu().numpy()
    assert np.abs(grav - g['dyn_gravity']).max() < tol_tau


@pytest.mark.parametrize('dt', ['f64', 'f32'])
def test_inverse_then_forward_dynamics_is_the_identity(dt):
    """ID o FD = identity on the controlled joints (servo joints at rest, damping off) -- the assumption the default
    kinematic mode makes is exact here; with damping on, the acceleration drops by M_aa^-1 D dq."""
    from rl_on_manifold_amd import inverse_dynamics, forward_dynamics
    rng = np.random.default_rng(4)
    n = 1000
    q = rng.uniform(-1.5, 1.5, (n, 9)); dq = rng.uniform(-1.5, 1.5, (n, 9)); dq[:, 6:] = 0
    dd = np.concatenate([rng.uniform(-10, 10, (n, 6)), np.zeros((n, 3))], 1)
    t = lambda a: torch.tensor(a, device=DEV, dtype=DT[dt])                   # noqa: E731
    tau = inverse_dynamics(t(q), t(dq), t(dd))
    back = forward_dynamics(t(q), t(dq), tau[:, :6].contiguous(), None, damping=False).cpu().numpy()
    assert np.abs(back - dd[:, :6]).max() < (1e-9 if dt == 'f64' else 2e-2)    # float32: cond(M_aa) ~ 1e4 on 10 rad/s^2
    damped = forward_dynamics(t(q), t(dq), tau[:, :6].contiguous(), None, damping=True).cpu().numpy()
    ref = D.forward_dynamics(q, dq, tau.cpu().numpy().astype(np.float64)[:, :6], np.zeros((n, 3)))
    assert np.abs(damped - ref).max() < (1e-8 if dt == 'f64' else 2e-2)
    assert np.abs(damped - back).max() > 1e-2                                 # the damping really acts
    # prescribed servo accelerations couple into the arm
    aux = rng.uniform(-20, 20, (n, 3))
    coupled = forward_dynamics(t(q), t(dq), tau[:, :6].contiguous(), t(aux), damping=True).cpu().numpy()
    ref = D.forward_dynamics(q, dq, tau.cpu().numpy().astype(np.float64)[:, :6], aux)
    assert np.abs(coupled - ref).max() < (1e-8 if dt == 'f64' else 2e-2)


def test_passive_dynamics_energy_budget():
    """Energy drift is bounded and of integrator order: the undriven, undamped chain (tau = 0) integrated with the engine's
    semi-implicit Euler conserves E = T + V up to an error that halves with the step; with the URDF damping the energy
    only goes down."""
    from rl_on_manifold_amd import forward_dynamics
    rng = np.random.default_rng(7)
    n = 256
    q = np.concatenate([IIWA_INIT_Q + rng.normal(0, 0.2, (n, 6)), np.zeros((n, 3))], 1)
    dq = np.concatenate([rng.normal(0, 0.3, (n, 6)), np.zeros((n, 3))], 1)

    def run(h, steps, damping):
        qq, dd = q.copy(), dq.copy()
        e0 = sum(D.energy(qq, dd))
        worst = np.zeros(n)
        for _ in range(steps):
            acc = forward_dynamics(torch.tensor(qq, device=DEV), torch.tensor(dd, device=DEV),
                                   torch.zeros((n, 6), device=DEV, dtype=torch.float64), None, damping=damping).cpu().numpy()
            dd[:, :6] += acc * h
            qq[:, :6] += dd[:, :6] * h
            worst = np.maximum(worst, np.abs(sum(D.energy(qq, dd)) - e0))
        return e0, sum(D.energy(qq, dd)), worst

    e0, e1, drift = run(1.0 / 240.0, 30, False)              # 1/8 s of free fall
    _, _, drift_half = run(1.0 / 480.0, 60, False)
    scale = np.abs(e0).max()
    assert np.median(drift) < 5e-3 * scale and drift.max() < 0.05 * scale
    assert np.median(drift_half / np.maximum(drift, 1e-12)) < 0.65          # first order in the step
    e0, e1, _ = run(1.0 / 240.0, 30, True)
    assert (e1 <= e0 + 1e-3 * scale).all() and (e1 < e0 - 1e-5).mean() > 0.9


def _aux(o):
    return np.concatenate([o.qx, o.dqx], 1)


def _rigid_body_env_step(dt, lanes, mode, T):
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_parity import _full_state
    from parity_tools import SensitivityRecorder
    from rl_on_manifold_amd import BatchedAtacomEnv
    spec = osc.iiwa_spec(dynamics_mode={'rigid_body': 1, 'rigid_body_ff': 2}[mode])
    B = 256
    env = BatchedAtacomEnv('iiwa', B, device=DEV, dtype=DT[dt], lanes_per_env=lanes, dynamics_mode=mode)
    # the rigid-body kernels exist per lane and per quad: a wider request maps down, and the handle says so
    assert env.lanes_per_env == env.rollout_lanes_per_env == min(lanes, 4)
    rng = np.random.default_rng(3)
    o = ob.BatchedAtacomEnv(spec, B, init_q=IIWA_INIT_Q + rng.normal(0, 0.05, (B, 6)))

    def outputs(p, inputs):
        oo, orr, oab, _ = p.step(inputs[0])
        return np.concatenate([oo, p.s, p.qx, p.dqx, orr[:, None]], 1)

    rec = SensitivityRecorder(outputs, seed=2, state_fields=('q', 'dq', 's', 'puck', 'qx', 'dqx'))
    moved = 0.0
    for t in range(T):
        a = rng.uniform(-1.2, 1.2, (B, 5))
        env.set_state(_full_state(env, o))
        env.set_aux_state(_aux(o))
        obs, r, ab, _ = env.step(a)
        nq, ng = 6, 11
        s_dev = env.get_state().cpu().numpy()[:, 2 * nq:2 * nq + ng]
        dev = np.concatenate([obs.cpu().numpy(), s_dev, env.get_aux_state().cpu().numpy(), r.cpu().numpy()[:, None]], 1)
        if dt == 'f32':
            rec.record(o, (a,), dev)
        oo, orr, oab, _ = o.step(a)
        if dt == 'f64':
            ref = np.concatenate([oo, o.s, o.qx, o.dqx, orr[:, None]], 1)
            assert np.abs(dev - ref).max() < 1e-8, np.abs(dev - ref).max()
        moved = max(moved, np.abs(o.qx).max())
    assert moved > 1e-3                                  # the servo joints really move
    if dt == 'f32':
        print(rec.finish('rigid-body step lanes %d' % lanes))
    # and the mode is not a no-op: the kinematic engine lands elsewhere
    if mode != 'rigid_body':
        return
    kin = BatchedAtacomEnv('iiwa', B, device=DEV, dtype=DT[dt], lanes_per_env=lanes)
    kin.set_state(_full_state(kin, o)); env.set_state(_full_state(env, o)); env.set_aux_state(_aux(o))
    a = rng.uniform(-1, 1, (B, 5))
    d = (kin.step(a)[0] - env.step(a)[0]).abs().max().item()
    assert d > 1e-4


@pytest.mark.mapping(name='iiwa', dyn=True)
@pytest.mark.parametrize('mode', ['rigid_body', 'rigid_body_ff'])
@pytest.mark.parametrize('lanes', [1, 4])
@pytest.mark.parametrize('dt', ['f64', 'f32'])
def test_rigid_body_env_step_against_oracle(dt, lanes, mode):
    """dynamics_mode = 'rigid_body' / 'rigid_body_ff': the whole env step (ATACOM projection, inverse dynamics, servo joints,
    hybrid forward dynamics, integration) vs the oracle, teacher-forced incl. the servo-joint state, on both mappings the mode
    has.  Of the step's saturations these closed-loop states reach the servo velocity set-point clip only: the motor limit,
    its floor and the arm effort limits never bind here (largest |tau| 140 Nm against 320) -- tests/test_gpu_rigid_limits.py
    runs the states where they do.  float64: 256 x 30 states at 1e-8.  float32: 256 x 8 states by the sensitivity rule (its host side -- the
    oracle's rigid-body step under perturbations -- is what takes the time: the 30-step form is the `slow` test below)."""
    _rigid_body_env_step(dt, lanes, mode, 30 if dt == 'f64' else 8)


@pytest.mark.slow
@pytest.mark.parametrize('mode', ['rigid_body', 'rigid_body_ff'])
@pytest.mark.parametrize('lanes', [1, 4, 8])
def test_rigid_body_env_step_against_oracle_soak(lanes, mode):
    """The float32 form of the test above on 256 x 30 states per case (35 - 55 s each, all of it the oracle), incl. a request
    for 8 lanes (runs the quad)."""
    _rigid_body_env_step('f32', lanes, mode, 30)


def test_rigid_body_rollout_equals_steps_and_keeps_the_constraints():
    """k_rollout in rigid-body mode == the same steps one launch at a time; ATACOM still holds the constraints."""
    from rl_on_manifold_amd import BatchedAtacomEnv
    B, T = 512, 60
    g = torch.Generator(device=DEV).manual_seed(0)
    acts = torch.rand((T, B, 5), device=DEV, generator=g) * 2 - 1
    e1 = BatchedAtacomEnv('iiwa', B, device=DEV, dynamics_mode='rigid_body', auto_reset=True, horizon=25)
    e2 = BatchedAtacomEnv('iiwa', B, device=DEV, dynamics_mode='rigid_body', auto_reset=True, horizon=25)
    out = e1.rollout(acts)
    for t in range(T):
        obs, r, ab, info = e2.step(acts[t])
        assert torch.allclose(obs, out['next_obs'][t], atol=2e-5) and torch.equal(info['last'], out['last'][t].bool())
    assert torch.allclose(e1.get_aux_state(), e2.get_aux_state(), atol=2e-5)
    c_avg, c_max, c_dq = e1.get_constraints_logs()
    assert c_max < 0.02 and c_dq < 0.0
    assert e1.lanes_per_env == 4 and e1.rollout_lanes_per_env == 4          # B = 512 would pick 8 lanes: clamped, and said so
    with pytest.raises(Exception):
        BatchedAtacomEnv('planar', 8, device=DEV, dynamics_mode='rigid_body')


def _config4_free_run(mode, B, T, seed):
    """Free-running rigid-body engine and oracle from the feasible initial states of BASELINE config 4."""
    import bench
    from rl_on_manifold_amd import BatchedAtacomEnv
    gen = torch.Generator(device=DEV); gen.manual_seed(seed)
    init = bench.feasible_init('iiwa', B, torch.device(DEV), gen)[0]
    acts = torch.rand((T, B, 5), device=DEV, generator=gen) * 2 - 1
    env = BatchedAtacomEnv('iiwa', B, device=DEV, dynamics_mode=mode, auto_reset=True)
    env.reset(state=init)
    out = env.rollout(acts)
    q6_min = float(out['next_obs'][:, :, 11].abs().min())
    dev = env.get_constraints_logs()
    i64 = init.double().cpu().numpy()
    spec = osc.iiwa_spec(dynamics_mode={'rigid_body': 1, 'rigid_body_ff': 2}[mode])
    o = ob.BatchedAtacomEnv(spec, B, init_q=i64[:, :6], init_dq=i64[:, 6:12], init_puck=i64[:, 12:18])
    a64 = acts.double().cpu().numpy()
    for t in range(T):
        _, _, ab, _ = o.step(a64[t])
        last = ab | (o.t >= o.spec.horizon)
        if last.any():
            o.reset(last)
    return dev, o.get_constraints_logs(), q6_min


def test_rigid_body_free_running_velocity_guarantee():
    """Where the rigid-body mode breaks ATACOM's velocity guarantee, and the mode that keeps it.
    1024 config-4 environments x 120 steps, free-running, HIP float32 and oracle float64 on identical input; the run
    reaches |q6| < 0.1, where joints 5 and 7 align and the reference's joint-7 set-point (env_single.py:137-170) flips by
    pi / 2 from sub-step to sub-step: the servo then swings at +-1.5 v_max, 1700 rad/s^2, and the reaction M_57 dds throws
    joint 5 about -- the URDF effort limits (40 Nm against ~7 Nm needed) do not bind.
      rigid_body    : the reference's inverse dynamics (zeros for the servo joints): c_dq_max > 0 is the MODEL's, the same
                      in both precisions, and bounded by the 1.5 v_max velocity clamp;
      rigid_body_ff : servo accelerations fed forward: c_dq_max <= 1e-3."""
    B, T = 1024, 120
    (d1, o1, q6a), (d2, o2, q6b) = _config4_free_run('rigid_body', B, T, 7), _config4_free_run('rigid_body_ff', B, T, 7)
    print('rigid_body    device %s oracle %s min|q6| %.3f' % (np.round(d1, 4), np.round(o1, 4), q6a))
    print('rigid_body_ff device %s oracle %s min|q6| %.3f' % (np.round(d2, 4), np.round(o2, 4), q6b))
    assert q6a < 0.1 and q6b < 0.1
    for d, o in ((d1, o1), (d2, o2)):
        assert o[1] / 1.5 <= d[1] <= 1.5 * o[1] and abs(d[0] - o[0]) <= 0.15 * o[0], (d, o)
    vmax = osc.iiwa_spec().vel_max.max()
    assert d1[2] <= 0.5 * vmax + 1e-3 and o1[2] <= 0.5 * vmax + 1e-9             # the 1.5 x clamp
    assert d2[2] <= 1e-3 and o2[2] <= 1e-3, (d2, o2)


def test_policy_rollout_in_rigid_body_mode(golden):
    """Rows N2 + N4 together: the actor network evaluated inside the rigid-body rollout kernel (lane and quad mappings)
    == the host evaluating the same network step by step on the rigid-body step kernel."""
    from rl_on_manifold_amd import BatchedAtacomEnv, MlpPolicy
    B, T = 160, 10
    gw = torch.Generator().manual_seed(1)
    W = [torch.randn(64, 18, generator=gw) * 0.2, torch.randn(64, generator=gw) * 0.1, torch.randn(64, 64, generator=gw) * 0.1,
         torch.randn(64, generator=gw) * 0.1, torch.randn(5, 64, generator=gw) * 0.1, torch.zeros(5)]
    pol = MlpPolicy(*W, std=torch.full((5,), 0.3))
    Wd = [w.to(DEV) for w in W]
    for lanes in (1, 4):
        env = BatchedAtacomEnv('iiwa', B, device=DEV, dynamics_mode='rigid_body', lanes_per_env=lanes)
        g = torch.Generator(device=DEV).manual_seed(4)
        eps = torch.randn((T, B, 5), device=DEV, generator=g)
        st, aux = env.get_state().clone(), env.get_aux_state().clone()
        out = env.rollout_policy(pol, T, noise=eps)
        assert torch.isfinite(out['reward']).all()
        env.set_state(st); env.set_aux_state(aux)
        for t in range(T):
            h = torch.relu(out['obs'][t] @ Wd[0].T + Wd[1])             # the network on the kernel's own observation
            h = torch.relu(h @ Wd[2].T + Wd[3])
            a = h @ Wd[4].T + Wd[5] + 0.3 * eps[t]
            assert torch.allclose(a, out['action'][t], atol=2e-4), (lanes, t)
            obs, r, ab, info = env.step(out['action'][t])
            # (the two kernels order the solver's arithmetic differently and the closed loop amplifies rounding, DESIGN.md
            # section 2: free-running agreement in the bulk, not in every environment)
            d = (obs - out['next_obs'][t]).abs().amax(1)
            assert float(d.median()) < 2e-5 and float((d < 2e-3).float().mean()) > 0.97, (lanes, t, float(d.max()))
        assert float(env.get_aux_state().abs().max()) > 1e-4
