"""The runs behind tests/golden/step_params_identity.npz: what the 8-lane float32 iiwa kernels return where a parameter read
behind the sub-step loop decides the result and neither tests/lane_group_identity_cases.py nor
tests/pair_broadcast_identity_cases.py looks: recorded once (profiles/tools/gen_step_params_identity_golden.py, on the commit
before the step kernel began to re-read its parameters from the kernel-argument segment, csrc/atacom_kernels.h: PARAMS_REREAD)
and compared bit for bit ever since (tests/test_gpu_step_params_identity.py).

19 environments (an odd batch), 20 steps with the horizon at 8, so that every environment is reset IN THE KERNEL twice, with
random_init on: the reset re-draws the puck from (seed, environment, episode) -- Params::random_init, ::seed, ::auto_reset and
::horizon behind the loop.  A non-zero action_penalty enters every reward there; the puck model and the termination read the
table, puck, mallet and goal constants there."""
import numpy as np

T, HORIZON = 20, 8
LANES = 8
BATCH = 19
SEED = 4711
ACTION_PENALTY = 0.0375
# step = atacom_step; masked = atacom_step_masked with every third environment sitting out; rollout = the T-step kernel
CASES = ['step', 'masked', 'rollout']
FIELDS = ('obs', 'reward', 'absorbing', 'last')


def case_id(kind):
    return 'iiwa_%s' % kind


def _inputs(env):
    """Seeded initial states [B, init_state_dim] around the reset pose and actions [T, B, k] (host, float64)."""
    B, nq, ng = env.batch, env.dims['q'], env.dims['g']
    rng = np.random.default_rng(20262)
    full = env.get_state().cpu().numpy().astype(np.float64)
    init = np.zeros((B, env.init_state_dim))
    init[:, :nq] = full[:, :nq] + rng.normal(0, 0.05, (B, nq))
    init[:, nq:2 * nq] = rng.normal(0, 0.02, (B, nq))
    init[:, 2 * nq:] = full[:, 2 * nq + ng:2 * nq + ng + env.init_state_dim - 2 * nq]
    acts = rng.uniform(-1.2, 1.2, (T, B, env.dims['null']))
    return init, acts


def run_case(kind, device='cuda:0'):
    """{key: numpy array} of one case; keys are prefixed with the case id."""
    import torch
    from rl_on_manifold_amd import BatchedAtacomEnv
    dtype = torch.float32
    env = BatchedAtacomEnv('iiwa', BATCH, device=device, dtype=dtype, auto_reset=True, horizon=HORIZON, lanes_per_env=LANES,
                           random_init=True, seed=SEED, action_penalty=ACTION_PENALTY)
    assert env.lanes_per_env == LANES and env.rollout_lanes_per_env == LANES, (env.lanes_per_env, env.rollout_lanes_per_env)
    init, acts = _inputs(env)
    init_t = torch.as_tensor(init, dtype=dtype, device=device)
    acts_t = torch.as_tensor(acts, dtype=dtype, device=device)
    cid, out = case_id(kind), {}

    def put(key, t):
        out['%s/%s' % (cid, key)] = t.detach().cpu().numpy().copy()

    env.reset(state=init_t)                 # an explicit state wins over the draw: the in-kernel resets are the ones that draw
    env.get_constraints_logs()
    if kind == 'rollout':
        ro = env.rollout(acts_t)
        for key in FIELDS:
            put(key, ro[key])
    else:
        mask = torch.as_tensor(np.arange(BATCH) % 3 != 0, device=device) if kind == 'masked' else None
        rows = {k: [] for k in FIELDS}
        for t in range(T):
            obs, reward, absorbing, info = env.step(acts_t[t], mask=mask)
            for k, v in zip(FIELDS, (obs, reward, absorbing, info['last'])):
                rows[k].append(v.view(torch.uint8) if v.dtype == torch.bool else v)
        for k, v in rows.items():
            put(k, torch.stack(v))
    put('state', env.get_state())
    out['%s/stats' % cid] = np.asarray(env.get_constraints_logs(), dtype=np.float64)
    env.close()
    return out
