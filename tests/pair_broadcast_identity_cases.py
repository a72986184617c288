"""The runs behind tests/golden/pair_broadcast_identity.npz: what the 8-lane float32 kernels return where
tests/lane_group_identity_cases.py does not reach, recorded once (profiles/tools/gen_pair_broadcast_identity_golden.py, on
the commit before the 8-lane broadcasts of csrc/atacom_quad.h became row-wide 64-bit DPP moves) and compared bit for bit
ever since (tests/test_gpu_pair_broadcast_identity.py).

A row-wide broadcast serves the two 8-lane groups of a 16-lane DPP row with one instruction, so the batches are ODD: 19 iiwa
and 11 planar environments leave the last row with one live group and one group whose lanes are switched off.  12 steps with
the horizon's reset at 8 in them."""
import numpy as np

T, HORIZON = 12, 8
LANES = 8
BATCH = {'iiwa': 19, 'planar': 11}
# (case, environment): step = atacom_step + the T-step kernel; masked = atacom_step_masked with every third environment
# sitting out; policy = the 8-lane policy kernel through rollout_packed; rollout = the T-step kernel alone
CASES = [('step', 'iiwa'), ('masked', 'iiwa'), ('policy', 'iiwa'), ('rollout', 'planar')]


def case_id(kind, name):
    return '%s_%s' % (name, kind)


def _inputs(env, name):
    """Seeded initial states [B, init_state_dim] around the reset pose, actions and noise [T, B, k] (host, float64)."""
    B, nq, ng = env.batch, env.dims['q'], env.dims['g']
    rng = np.random.default_rng(20261 + len(name))
    full = env.get_state().cpu().numpy().astype(np.float64)
    init = np.zeros((B, env.init_state_dim))
    init[:, :nq] = full[:, :nq] + rng.normal(0, 0.05, (B, nq))
    init[:, nq:2 * nq] = rng.normal(0, 0.02, (B, nq))
    if env.init_state_dim > 2 * nq:
        init[:, 2 * nq:] = full[:, 2 * nq + ng:2 * nq + ng + env.init_state_dim - 2 * nq]
    acts = rng.uniform(-1.2, 1.2, (T, B, env.dims['null']))
    noise = rng.normal(0, 1, (T, B, env.dims['null']))
    return init, acts, noise


def _policy(D, k):
    import torch
    from rl_on_manifold_amd import MlpPolicy
    g = np.random.default_rng(7)
    t = lambda a: torch.as_tensor(a, dtype=torch.float32)      # noqa: E731
    return MlpPolicy(t(g.normal(0, 0.2, (64, D))), t(g.normal(0, 0.1, 64)), t(g.normal(0, 0.1, (64, 64))),
                     t(g.normal(0, 0.1, 64)), t(g.normal(0, 0.1, (k, 64))), torch.zeros(k), std=torch.full((k,), 0.3))


def run_case(kind, name, device='cuda:0'):
    """{key: numpy array} of one case; keys are prefixed with the case id."""
    import torch
    from rl_on_manifold_amd import BatchedAtacomEnv
    dtype = torch.float32
    env = BatchedAtacomEnv(name, BATCH[name], device=device, dtype=dtype, auto_reset=True, horizon=HORIZON, lanes_per_env=LANES)
    assert env.lanes_per_env == LANES and env.rollout_lanes_per_env == LANES, (env.lanes_per_env, env.rollout_lanes_per_env)
    init, acts, noise = _inputs(env, name)
    init_t = torch.as_tensor(init, dtype=dtype, device=device)
    acts_t = torch.as_tensor(acts, dtype=dtype, device=device)
    cid, out = case_id(kind, name), {}

    def put(key, t):
        out['%s/%s' % (cid, key)] = t.detach().cpu().numpy().copy()

    def finish(prefix=''):
        put(prefix + 'state', env.get_state())
        out['%s/%sstats' % (cid, prefix)] = np.asarray(env.get_constraints_logs(), dtype=np.float64)

    env.reset(state=init_t)
    env.get_constraints_logs()
    if kind in ('step', 'masked'):
        mask = None
        if kind == 'masked':
            mask = torch.as_tensor(np.arange(BATCH[name]) % 3 != 0, device=device)
        rows = {k: [] for k in ('obs', 'reward', 'absorbing', 'last')}
        for t in range(T):
            obs, reward, absorbing, info = env.step(acts_t[t], mask=mask)
            for k, v in zip(('obs', 'reward', 'absorbing', 'last'), (obs, reward, absorbing, info['last'])):
                rows[k].append(v.view(torch.uint8) if v.dtype == torch.bool else v)
        for k, v in rows.items():
            put(k, torch.stack(v))
        finish()
    if kind in ('step', 'rollout'):
        env.reset(state=init_t)
        env.get_constraints_logs()
        ro = env.rollout(acts_t)
        for key in ('obs', 'next_obs', 'reward', 'absorbing', 'last'):
            put('rollout/%s' % key, ro[key])
        finish('rollout/')
    if kind == 'policy':
        assert env.policy_lanes_per_env == LANES, env.policy_lanes_per_env
        noise_t = torch.as_tensor(noise, dtype=dtype, device=device)
        rec = env.rollout_packed(policy=_policy(env.obs_dim, env.dims['null']), n_steps=T, noise=noise_t)
        put('records', rec)
        finish()
    env.close()
    return out
