"""The runs behind tests/golden/lane_group_identity.npz: what the lane-group kernels (2, 4 and 8 lanes per environment)
return on seeded free-running episodes, recorded once (profiles/tools/gen_lane_group_identity_golden.py, on the commit
before the butterfly sums of csrc/atacom_quad.h were handed to the compiler) and compared bit for bit ever since
(tests/test_gpu_lane_group_identity.py).

20 iiwa environments (not a multiple of the 8 environments a wave holds on 8 lanes) and 12 planar ones, seeded initial
states and actions, 130 steps with the horizon's reset at 120 in them."""
import numpy as np

T, HORIZON = 130, 120
CHECK = (1, 2, 119, 120, 121, 130)            # steps (1-based) whose returns are recorded
BATCH = {'iiwa': 20, 'planar': 12}
# (environment, dtype, lanes per environment, also through the T-step kernel)
CASES = [(name, 'f32', lanes, lanes == 8) for name in ('iiwa', 'planar') for lanes in (8, 4, 2)] + [('iiwa', 'f64', 8, False)]


def case_id(name, dt, lanes):
    return '%s_%s_l%d' % (name, dt, lanes)


def _inputs(env, name):
    """Seeded initial states [B, init_state_dim] around the reset pose and actions [T, B, k] (host, float64)."""
    B, nq, ng = env.batch, env.dims['q'], env.dims['g']
    rng = np.random.default_rng(20260 + len(name))
    full = env.get_state().cpu().numpy().astype(np.float64)
    init = np.zeros((B, env.init_state_dim))
    init[:, :nq] = full[:, :nq] + rng.normal(0, 0.05, (B, nq))
    init[:, nq:2 * nq] = rng.normal(0, 0.02, (B, nq))
    if env.init_state_dim > 2 * nq:
        init[:, 2 * nq:] = full[:, 2 * nq + ng:2 * nq + ng + env.init_state_dim - 2 * nq]
    acts = rng.uniform(-1.2, 1.2, (T, B, env.dims['null']))
    return init, acts


def run_case(name, dt, lanes, with_rollout, device='cuda:0'):
    """{key: numpy array} of one case; keys are prefixed with the case id."""
    import torch
    from rl_on_manifold_amd import BatchedAtacomEnv
    dtype = {'f32': torch.float32, 'f64': torch.float64}[dt]
    env = BatchedAtacomEnv(name, BATCH[name], device=device, dtype=dtype, auto_reset=True, horizon=HORIZON, lanes_per_env=lanes)
    assert env.lanes_per_env == lanes, (env.lanes_per_env, lanes)
    init, acts = _inputs(env, name)
    init_t = torch.as_tensor(init, dtype=dtype, device=device)
    acts_t = torch.as_tensor(acts, dtype=dtype, device=device)
    cid, out = case_id(name, dt, lanes), {}

    def put(key, t):
        out['%s/%s' % (cid, key)] = t.detach().cpu().numpy().copy()

    env.reset(state=init_t)
    env.get_constraints_logs()
    for t in range(T):
        obs, reward, absorbing, info = env.step(acts_t[t])
        if t + 1 in CHECK:
            put('step%d/obs' % (t + 1), obs)
            put('step%d/reward' % (t + 1), reward)
            put('step%d/absorbing' % (t + 1), absorbing.view(torch.uint8))
            put('step%d/last' % (t + 1), info['last'].view(torch.uint8))
    put('state', env.get_state())
    out['%s/stats' % cid] = np.asarray(env.get_constraints_logs(), dtype=np.float64)
    if with_rollout:
        assert env.rollout_lanes_per_env == lanes, (env.rollout_lanes_per_env, lanes)
        env.reset(state=init_t)
        env.get_constraints_logs()
        ro = env.rollout(acts_t)
        idx = torch.as_tensor([c - 1 for c in CHECK], device=device)
        for key in ('obs', 'next_obs', 'reward', 'absorbing', 'last'):
            put('rollout/%s' % key, ro[key][idx])
        put('rollout/state', env.get_state())
        out['%s/rollout/stats' % cid] = np.asarray(env.get_constraints_logs(), dtype=np.float64)
    env.close()
    return out
