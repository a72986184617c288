"""GPU tests of the collision-avoidance task collected with the actor network in the kernel (libatacom_point_policy.so,
k_point_rollout_mlp) through BatchedPointReachEnv.rollout_policy / rollout_packed, the C ABI and RolloutCollector.

Stated bounds
  env part      : EQUALITY.  The actions the fused kernel recorded, fed to rollout() (k_point_rollout) on a twin env, give
                  bit-equal obs, next_obs, reward, last, state rows and constraint logs, float32 and float64: the validated
                  accuracy of k_point_rollout carries over without a new tolerance.
  network, f64  : 1e-8 on every sample against the restatement (tests/point_policy_oracle.py) evaluated on the recorded
                  observations; the fixture of the reference's own networks replayed teacher-forced at 1e-8.
  network, f32  : per step, against the float64 restatement on the recorded float32 observation: err <= 4 sens + 5e-6
                  (tests/parity_tools.py: C_SENS, FLOOR; sens = the restatement's response to float32-sized perturbations of
                  observation, noise and weights, QUICK_SCALES), no sample's bound may be vacuous (> 1e-2).
  structure     : equalities (T x 1 step == 1 x T steps, packed == arrays, padding untouched, collector == rollout_policy).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_policy_oracle as ppo                                   # noqa: E402
from parity_tools import C_SENS, FLOOR, QUICK_SCALES, VACUOUS       # noqa: E402

DEV = 'cuda:0'
DT = {'f64': torch.float64, 'f32': torch.float32}
F64_BOUND = 1e-8
KINDS = ('gauss', 'gauss_tanh', 'sac', 'td3', 'ddpg')              # PPO / TRPO (both activations), SAC, TD3, DDPG
KEYS = ('obs', 'next_obs', 'reward', 'last')
H, T = 9, 25                                                        # every environment auto-resets twice
LOG_STD = (-0.1, 0.2)                                               # narrowed so that SAC's clamp is exercised
X0 = np.array([0.15, -0.1])
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'point_policy.npz')


class _Net:
    """A module with the reference actors' attribute names; weights of the size torch.nn.Linear initialises, the output
    layer widened so that tanh / the clip leave their linear range."""

    def __init__(self, n_in, seed, out_gain=1.0):
        g = torch.Generator().manual_seed(seed)
        self._h1, self._h2, self._h3 = (torch.nn.Linear(a, b, dtype=torch.float64) for a, b in ((n_in, 64), (64, 64), (64, 2)))
        with torch.no_grad():
            for lin in (self._h1, self._h2, self._h3):
                k = 1.0 / np.sqrt(lin.weight.shape[1])
                lin.weight.copy_((torch.rand(lin.weight.shape, generator=g, dtype=torch.float64) * 2 - 1) * k)
                lin.bias.copy_((torch.rand(lin.bias.shape, generator=g, dtype=torch.float64) * 2 - 1) * k)
            self._h3.weight.mul_(out_gain)
        self._action_scaling = torch.tensor([1.0, 0.8], dtype=torch.float64)
        self.W = [t.detach().numpy().copy() for lin in (self._h1, self._h2, self._h3) for t in (lin.weight, lin.bias)]


def _pair(kind, n):
    """(device MlpPolicy, restated policy) of one agent of examples/collision_avoidance_exp.py at the task's bounds."""
    from rl_on_manifold_amd import MlpPolicy
    n_in = 4 * (1 + n)
    lo, hi = np.full(n_in, ppo.OBS_LOW), np.full(n_in, ppo.OBS_HIGH)
    net = _Net(n_in, 100 + n, out_gain=6.0)
    kw = dict(obs_low=lo, obs_high=hi)
    if kind in ('gauss', 'gauss_tanh'):
        act = 'tanh' if kind == 'gauss_tanh' else 'relu'
        dev = MlpPolicy.from_module(net, std=torch.full((2,), ppo.PPO_STD, dtype=torch.float64), activation=act, **kw)
        ora = ppo.make_policy('ppo', net.W)
        ora.act = np.tanh if act == 'tanh' else ora.act
    elif kind == 'sac':
        sg = _Net(n_in, 200 + n, out_gain=8.0)
        dev = MlpPolicy.from_sac(net, sg, log_std_min=LOG_STD[0], log_std_max=LOG_STD[1], **kw)
        ora = ppo.make_policy('sac', net.W, sigma_W=sg.W)
        ora.log_std_min, ora.log_std_max = LOG_STD
    elif kind == 'td3':
        dev = MlpPolicy.from_td3(net, ppo.TD3_SIGMA, low=-0.7, high=0.6, **kw)
        ora = ppo.make_policy('td3', net.W, act_scale=net._action_scaling.numpy(), low=-0.7, high=0.6)
    else:
        dev = MlpPolicy.from_ddpg(net, np.ones(1) * ppo.DDPG_SIGMA, ppo.THETA, ppo.OU_DT, x0=X0, **kw)
        ora = ppo.make_policy('ddpg', net.W, act_scale=net._action_scaling.numpy(), x0=X0)
    return dev, ora


def _env(B, n, rw, dt, **kw):
    from rl_on_manifold_amd import BatchedPointReachEnv
    kw.setdefault('horizon', H)
    kw.setdefault('seed', 6)
    return BatchedPointReachEnv(B, n_objects=n, random_walk=rw, device=DEV, dtype=DT[dt], **kw)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _inputs(B, n, dt, supplied, seed=0, steps=T):
    g = torch.Generator(device=DEV).manual_seed(seed)
    noise = torch.randn((steps, B, 2), device=DEV, dtype=DT[dt], generator=g)
    draws = (torch.rand((steps, B, n, 2), device=DEV, dtype=DT[dt], generator=g) * 2 - 1) if supplied else None
    return noise, draws


def _restated_actions(ora, obs, noise, horizon=H):
    """The restatement evaluated open loop on recorded observations [T, B, D]; the environments were reset before the call,
    so the episode step counter at step t is t mod horizon.  -> actions [T, B, 2], OU state after the call (or None)."""
    ora.x = None
    B = obs.shape[1]
    acts = [ppo.draw(ora, obs[t], noise[t], np.full(B, t % horizon)) for t in range(obs.shape[0])]
    return np.stack(acts), getattr(ora, 'x', None)


def _assert_env_part_equal(out, env, twin, draws):
    ref = twin.rollout(out['action'], draws=draws)
    for k in KEYS:
        assert torch.equal(out[k], ref[k]), k
    assert out['absorbing'].sum().item() == 0
    assert torch.equal(env.get_state(), twin.get_state())
    assert env.get_constraints_logs() == twin.get_constraints_logs()


# ---------------------------------------------------------------------------------------------------- 7. env part
@pytest.mark.parametrize('supplied', [False, True])
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('rw', [True, False])
@pytest.mark.parametrize('n', [2, 4])
def test_env_part_is_k_point_rollout_bit_for_bit(n, rw, kind, dt, supplied):
    B = 300
    env, twin = _env(B, n, rw, dt), _env(B, n, rw, dt)
    assert torch.equal(env.reset(), twin.reset())
    dev, _ = _pair(kind, n)
    noise, draws = _inputs(B, n, dt, supplied)
    out = env.rollout_policy(dev, T, noise=noise, draws=draws)
    assert torch.isfinite(out['action']).all().item()
    assert out['last'].sum().item() == B * (T // H)                  # two in-kernel resets per environment
    _assert_env_part_equal(out, env, twin, draws)


@pytest.mark.parametrize('B', [1, 63, 257, 1000])
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_ragged_batches_env_part_and_packed_records(B, dt):
    n = 4
    env, twin, penv = (_env(B, n, True, dt) for _ in range(3))
    for e in (env, twin, penv):
        e.reset()
    dev, _ = _pair('sac', n)
    noise, draws = _inputs(B, n, dt, True, seed=B)
    out = env.rollout_policy(dev, T, noise=noise, draws=draws)
    _assert_env_part_equal(out, env, twin, draws)
    rec = penv.rollout_packed(policy=dev, n_steps=T, noise=noise, draws=draws, batch_stride=B + 3)
    assert rec.shape == (T, B + 3, penv.record_dim) and not rec[:, B:].any().item()
    u = penv.unpack_records(rec[:, :B])
    for k in ('obs', 'action', 'reward', 'next_obs'):
        assert torch.equal(u[k], out[k]), k
    assert torch.equal(u['last'], out['last'].bool()) and not u['absorbing'].any().item()
    assert torch.equal(penv.get_state(), env.get_state())


# ---------------------------------------------------------------------------------------------------- 8. network, float64
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('rw', [True, False])
@pytest.mark.parametrize('n', [2, 4])
def test_float64_actions_against_the_restatement(n, rw, kind):
    B = 256
    env = _env(B, n, rw, 'f64')
    env.reset()
    dev, ora = _pair(kind, n)
    noise, _ = _inputs(B, n, 'f64', False, seed=3)
    out = env.rollout_policy(dev, T, noise=noise)
    ref, x = _restated_actions(ora, _np(out['obs']), _np(noise))
    err = np.abs(_np(out['action']) - ref)
    print('float64 %s n=%d random_walk=%s: worst |action - restatement| = %.3e over %d samples' % (kind, n, rw, err.max(), err.size))
    assert err.max() <= F64_BOUND, (err.max(), np.unravel_index(err.argmax(), err.shape))
    a = _np(out['action'])
    if kind == 'td3':                                                # 10: the clipped action is the one recorded
        assert a.min() >= -0.7 and a.max() <= 0.6 and (a == -0.7).any() and (a == 0.6).any()
    if kind == 'sac':                                                # 10: squash, and the clamp was reached on both sides
        assert np.abs(a).max() <= 1.0
        W1, b1, W2, b2, W3, b3 = ora.sigma_weights
        xx = (_np(out['obs']) - ora.shift) * ora.scale
        ls = np.maximum(np.maximum(xx @ W1.T + b1, 0) @ W2.T + b2, 0) @ W3.T + b3
        assert (ls < LOG_STD[0]).any() and (ls > LOG_STD[1]).any()
    if kind == 'ddpg':                                               # 10: x0 advanced from the last episode start
        assert np.abs(_np(dev.noise_state) - x).max() <= F64_BOUND
        x_ref = np.tile(X0, (B, 1))
        for t in range(T - T % H, T):
            x_ref = x_ref - ppo.THETA * x_ref * ppo.OU_DT + ppo.DDPG_SIGMA * np.sqrt(ppo.OU_DT) * _np(noise[t])
        assert np.abs(_np(dev.noise_state) - x_ref).max() <= F64_BOUND


@pytest.mark.parametrize('n', [2, 4])
def test_float64_replays_the_reference_fixture(n):
    """Every recorded step of the reference's own networks driving PointReachAtacom as one batch: set_state, one fused
    step with the recorded noise and draws, against the reference's action, next state, slack and reward."""
    from rl_on_manifold_amd import MlpPolicy
    import point_reach_oracle as pro
    G = np.load(GOLDEN)
    for kind in ('ppo', 'sac', 'td3', 'ddpg'):
        p = 'n%d_%s_' % (n, kind)
        S = int(G[p + 'state0'].shape[0])
        nets = []
        for tag in (['mu', 'sigma'] if kind == 'sac' else ['mu']):
            m = _Net(4 * (1 + n), 0)
            with torch.no_grad():
                for i, lin in enumerate((m._h1, m._h2, m._h3)):
                    lin.weight.copy_(torch.tensor(G['%s%s_W%d' % (p, tag, i + 1)]))
                    lin.bias.copy_(torch.tensor(G['%s%s_b%d' % (p, tag, i + 1)]))
            m._action_scaling = torch.tensor(G[p + 'action_scaling']) if (p + 'action_scaling') in G else m._action_scaling
            nets.append(m)
        lo, hi = np.full(4 * (1 + n), ppo.OBS_LOW), np.full(4 * (1 + n), ppo.OBS_HIGH)
        if kind == 'ppo':
            dev = MlpPolicy.from_module(nets[0], std=torch.full((2,), ppo.PPO_STD, dtype=torch.float64), obs_low=lo, obs_high=hi)
        elif kind == 'sac':
            dev = MlpPolicy.from_sac(nets[0], nets[1], obs_low=lo, obs_high=hi)
        elif kind == 'td3':
            dev = MlpPolicy.from_td3(nets[0], ppo.TD3_SIGMA, obs_low=lo, obs_high=hi)
        else:
            dev = MlpPolicy.from_ddpg(nets[0], np.ones(1) * ppo.DDPG_SIGMA, ppo.THETA, ppo.OU_DT, obs_low=lo, obs_high=hi)
        env = _env(S, n, True, 'f64', horizon=1000, auto_reset=False)
        o = pro.PointReachBatched(S, n_objects=n, random_walk=True)
        o.state, o.s = G[p + 'state0'].copy(), G[p + 's0'].copy()
        o.have_centres[:] = True
        o.t = np.arange(S)
        o.time = np.arange(S) * 0.01
        o.episode[:] = 1
        env.set_state(o.get_state())
        if kind == 'ddpg':
            dev.noise_state = torch.tensor(G[p + 'x0'], device=DEV, dtype=torch.float64)
        out = env.rollout_policy(dev, 1, noise=torch.tensor(G[p + 'noise'][None]), draws=torch.tensor(G[p + 'draws'][None]))
        st = _np(env.get_state())
        dev_out = np.concatenate([_np(out['action'][0]), _np(out['next_obs'][0]), st[:, 4 * (1 + n):4 * (1 + n) + n],
                                  _np(out['reward'][0])[:, None]], 1)
        ref = np.concatenate([G[p + 'action'], G[p + 'state1'], G[p + 's1'], G[p + 'reward'][:, None]], 1)
        err = np.abs(dev_out - ref)
        print('fixture n=%d %s: worst |dev - reference| = %.3e' % (n, kind, err.max()))
        assert err.max() <= F64_BOUND, (kind, err.max(), np.unravel_index(err.argmax(), err.shape))


# ---------------------------------------------------------------------------------------------------- 9. network, float32
def _perturbed_policy(ora, sc, rng):
    p = ora.__class__.__new__(ora.__class__)
    p.__dict__.update(ora.__dict__)
    for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
        w = getattr(ora, k)
        setattr(p, k, w * (1.0 + sc * rng.choice([-1.0, 1.0], w.shape)))
    if getattr(ora, 'sigma_weights', None) is not None:
        p.sigma_weights = [w * (1.0 + sc * rng.choice([-1.0, 1.0], w.shape)) for w in ora.sigma_weights]
    return p


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', [2, 4])
def test_float32_actions_every_sample_explained(n, kind):
    B = 512
    env = _env(B, n, True, 'f32')
    env.reset()
    dev, ora = _pair(kind, n)
    noise, _ = _inputs(B, n, 'f32', False, seed=4)
    out = env.rollout_policy(dev, T, noise=noise)
    obs, eps = _np(out['obs']), _np(noise)
    ref, _ = _restated_actions(ora, obs, eps)
    err = (np.abs(_np(out['action']) - ref) / np.maximum(1.0, np.abs(ref))).max(2)
    rng = np.random.default_rng(8)
    sens = np.zeros_like(err)
    for sc in QUICK_SCALES:
        for _ in range(2):
            p = _perturbed_policy(ora, sc, rng)
            po = obs * (1.0 + sc * rng.choice([-1.0, 1.0], obs.shape))
            pe = eps * (1.0 + sc * rng.choice([-1.0, 1.0], eps.shape))
            out_p, _ = _restated_actions(p, po, pe)
            sens = np.maximum(sens, (np.abs(out_p - ref) / np.maximum(1.0, np.abs(ref))).max(2))
    bound = C_SENS * sens + FLOOR
    print('float32 %s n=%d: %d samples, err median %.2e / p99.9 %.2e / max %.2e; err / (C sens + floor) max %.2f; bound max %.2e'
          % (kind, n, err.size, np.median(err), np.quantile(err, 0.999), err.max(), (err / bound).max(), bound.max()))
    assert bound.max() <= VACUOUS, bound.max()                      # no sample's bound may be vacuous
    assert (err <= bound).all(), (err.max(), np.unravel_index((err / bound).argmax(), err.shape))


# ---------------------------------------------------------------------------------------------------- 11. structure
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['sac', 'ddpg', 'td3'])
def test_one_call_of_T_steps_equals_T_calls_of_one(kind, dt):
    B, n = 300, 4
    a, b = _env(B, n, True, dt), _env(B, n, True, dt)
    a.reset(), b.reset()
    pa, _ = _pair(kind, n)
    pb, _ = _pair(kind, n)
    noise, draws = _inputs(B, n, dt, True, seed=5)
    out = a.rollout_policy(pa, T, noise=noise, draws=draws)
    for t in range(T):
        o = b.rollout_policy(pb, 1, noise=noise[t:t + 1], draws=draws[t:t + 1])
        for k in KEYS + ('action',):
            assert torch.equal(o[k][0], out[k][t]), (k, t)
    assert torch.equal(a.get_state(), b.get_state())
    assert a.get_constraints_logs() == b.get_constraints_logs()
    if kind == 'ddpg':
        assert torch.equal(pa.noise_state, pb.noise_state)


# ---------------------------------------------------------------------------------------------------- 12. packed records
@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', [2, 4])
def test_packed_records_equal_the_arrays(n, kind, dt):
    B = 200
    a, b = _env(B, n, True, dt), _env(B, n, True, dt)
    a.reset(), b.reset()
    pa, _ = _pair(kind, n)
    pb, _ = _pair(kind, n)
    noise, _ = _inputs(B, n, dt, False, seed=6)
    out = a.rollout_policy(pa, T, noise=noise)
    rec = b.rollout_packed(policy=pb, n_steps=T, noise=noise)
    assert rec.shape == (T, B, 2 * 4 * (1 + n) + 5)
    u = b.unpack_records(rec)
    for k in ('obs', 'action', 'reward', 'next_obs'):
        assert torch.equal(u[k], out[k]), k
    assert torch.equal(u['last'], out['last'].bool())
    assert torch.equal(a.get_state(), b.get_state())
    # pre-generated actions through the same kernel: the records of rollout()
    c, d = _env(B, n, True, dt), _env(B, n, True, dt)
    c.reset(), d.reset()
    ref = c.rollout(out['action'])
    u = d.unpack_records(d.rollout_packed(actions=out['action']))
    for k in ('obs', 'action', 'reward', 'next_obs'):
        assert torch.equal(u[k], ref[k] if k != 'action' else out['action']), k
    assert torch.equal(c.get_state(), d.get_state()) and c.get_constraints_logs() == d.get_constraints_logs()


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_c_abi_never_writes_the_padding_rows(dt):
    from rl_on_manifold_amd import _lib_point_policy
    from rl_on_manifold_amd.engine import _ptr
    B, n, ld = 70, 2, 77
    env = _env(B, n, True, dt)
    env.reset()
    pol, _ = _pair('td3', n)
    rec = torch.full((T, ld, env.record_dim), -777.0, device=DEV, dtype=DT[dt])
    net = pol.as_struct(env)
    lib = _lib_point_policy.load()
    _lib_point_policy.check(lib.atacom_point_policy_rollout_packed(env._h, T, None, C.byref(net), None, None, _ptr(rec), ld,
                                                                   env._stream()))
    assert (rec[:, B:] == -777.0).all().item() and not (rec[:, :B] == -777.0).any().item()
    # refusals at the ABI: both / neither of actions and net, a stride below the batch
    assert lib.atacom_point_policy_rollout_packed(env._h, T, None, None, None, None, _ptr(rec), ld, None) == _lib_point_policy.E_INVALID
    assert lib.atacom_point_policy_rollout_packed(env._h, T, None, C.byref(net), None, None, _ptr(rec), B - 1, None) == _lib_point_policy.E_INVALID
    assert 'record_batch_stride = %d' % (B - 1) in lib.atacom_point_policy_last_error().decode()
    # a network of the other obstacle count is refused with the value named
    other, _ = _pair('td3', 4)
    from rl_on_manifold_amd import AtacomError
    with pytest.raises(AtacomError, match='n_in = 20'):
        env.rollout_policy(other, 2)


# ---------------------------------------------------------------------------------------------------- 13. collector
@pytest.mark.parametrize('kind', ['gauss', 'ddpg'])
def test_rollout_collector_collects_the_task_fused(kind):
    from rl_on_manifold_amd import RolloutCollector
    B, n = 300, 4
    a, b = _env(B, n, True, 'f32'), _env(B, n, True, 'f32')
    a.reset(), b.reset()
    pa, _ = _pair(kind, n)
    pb, _ = _pair(kind, n)
    noise, _ = _inputs(B, n, 'f32', False, seed=7)
    out = a.rollout_policy(pa, T, noise=noise)
    col = RolloutCollector(b)
    data = col.time_major(col.collect(T, policy=pb, noise=noise))
    for k in ('obs', 'action', 'reward', 'next_obs'):
        assert torch.equal(data[k], out[k]), k
    assert torch.equal(data['last'], out['last'].bool())
    assert torch.equal(a.get_state(), b.get_state())
