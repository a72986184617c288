"""The runs behind tests/golden/offgrad_identity.npz and tests/golden/soft_identity.npz: what libatacom_offgrad.so
(critic_gradient, actor_gradient) and libatacom_soft.so (soft_td_target, soft_critic_gradient, soft_actor_gradient) return where
the code they share with libatacom_fit.so and libatacom_trust.so decides the result -- the row access, the transposition
buffers, the backward pass through the 2 x 64 network with and without the critic's second branch W2a, the hand-over between the
wavefronts, the float64 column pairs and the slice sum of the reduction.  Recorded once
(profiles/tools/gen_offpolicy_backward_identity_golden.py, on the commit before the two libraries' own copies of that code gave
way to csrc/mlp/atacom_mlp_backward.h) and compared bit for bit ever since (tests/test_gpu_offpolicy_backward_identity.py).

Rows and grids: a lone row (fifteen dead lanes of its 16-block), 17 (a part-filled second block), 65 (a second wavefront's tile
holding one row), 200 over two workgroups (all four wavefronts hand over, two partials are reduced; here the critics are a pair:
the grid's second dimension and blockIdx.y of the reduction), 600 in one workgroup (every wavefront walks more than one tile with
its accumulators live), and 70 of 200 rows gathered through an unsorted idx with repeats.  Shapes (D, k): (4, 2) is CH = 1 for a
DDPG call (the critic's first layer is D wide) and CH = 2 for TD3 and SAC (D + k), the actor's first layer zero-padded; (18, 5)
is CH = 6 with a part-filled second input tile (NT = 2); (24, 8) is CH = 8 with D + k = 32, both output quads of W3 and all
eight W2a columns live.  Both activations, normalisation and act_scale on and off, both critic kinds and both mean modes of the
DDPG / TD3 actor, every grid given or 0.  Every case runs in float32 and float64.

The golden holds every value of every output (a gradient is over four thousand values, and they do not compress), so the cases
are few: each row count appears once per library, at shapes that between them cover every path above.  With all three calls in
all six cases soft_identity.npz came to 1 129 340 bytes, above the largest fixture of tests/golden/ (and above 1 MiB); the pair is
needed once and is there once, at the smallest shape, so rather than lose a row count the SAC cases of 600 rows and of the
gathered rows leave soft_critic_gradient out and keep the target and both actor gradients.  The row access, the live accumulators
and the gather of a critic kernel are the header's, and k_offgrad_critic takes them through those two cases.

The inputs are those of offgrad_oracle.case and soft_oracle.case, which keep every row off the ReLU kinks, the ties of the two
critics and the clamp edges."""
import numpy as np

DTYPES = ('f32', 'f64')
NP = {'f32': np.float32, 'f64': np.float64}
GATHER = (70, 200)            # rows read, rows there

# (rows, n_blocks, kind, D, k, activation, normalise, act_scale, mean_mode, pair, gather)
OFFGRAD_CASES = [
    (1, 0, 'ddpg', 4, 2, 'relu', True, True, 1, False, False),
    (17, 0, 'td3', 18, 5, 'tanh', False, False, 0, False, False),
    (65, 0, 'td3', 24, 8, 'tanh', True, True, 1, False, False),
    (200, 2, 'td3', 18, 5, 'relu', True, True, 1, True, False),
    (600, 1, 'ddpg', 24, 8, 'relu', False, True, 0, False, False),
    (70, 0, 'td3', 4, 2, 'relu', True, False, 1, False, True),
]
# (rows, n_blocks, D, k, activation, normalise, act_scale and act_shift, critics, gather); critics: how many critics
# soft_critic_gradient takes, 0: the case leaves that call out (the module docstring says why)
SOFT_CASES = [
    (1, 0, 4, 2, 'relu', True, True, 1, False),
    (17, 0, 18, 5, 'tanh', False, False, 1, False),
    (65, 0, 24, 8, 'tanh', True, True, 1, False),
    (200, 2, 4, 2, 'relu', True, True, 2, False),
    (600, 1, 4, 2, 'tanh', False, True, 0, False),
    (70, 0, 4, 2, 'relu', True, False, 0, True),
]
OFFGRAD_FIELDS = ('critic0/flat', 'critic0/stats', 'actor/flat', 'actor/stats', 'actor/action_out', 'actor/dqda_out')
SOFT_FIELDS = ('target/y', 'target/action', 'target/logp', 'actor/mu', 'actor/sigma', 'actor/stats', 'actor/action', 'actor/logp',
               'actor/q', 'actor/dqda')
CRITIC_FIELDS = ('critic0/flat', 'critic0/stats', 'critic1/flat', 'critic1/stats')          # two per critic of soft_critic_gradient
PAIR_FIELDS = CRITIC_FIELDS[2:]                                                             # what a pair adds


def case_id(lib, case):
    return '%s_%s' % (lib, '_'.join(str(c) for c in case))


def fields(lib, case):
    """The outputs of a case, in the order of its keys."""
    if lib == 'offgrad':
        return OFFGRAD_FIELDS + (PAIR_FIELDS if case[-2] else ())
    return SOFT_FIELDS + CRITIC_FIELDS[:2 * case[-2]]


def _t(a, device):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _keyed(lib, case, dt, out):
    return {'%s/%s/%s' % (case_id(lib, case), dt, k): v.detach().cpu().numpy().copy() for k, v in out.items()}


def run_offgrad(case, dt, device='cuda:0'):
    """{key: numpy array} of one case of libatacom_offgrad.so in one dtype; keys are prefixed with the case id and the dtype."""
    import torch
    import offgrad_oracle as og
    from rl_on_manifold_amd import MlpPolicy, QCritic, actor_gradient, critic_gradient
    rows, n_blocks, kind, D, k, activation, normalise, act_scale, mean_mode, pair, gather = case
    c = og.case(3000 + OFFGRAD_CASES.index(case), kind, D, k, activation, normalise, act_scale, GATHER[1] if gather else rows,
                mean_mode=mean_mode, dtype=NP[dt], n_idx=rows if gather else 0)
    t = lambda a: _t(a, device)                                                           # noqa: E731
    a = c['actor']
    pol = MlpPolicy(*(t(a[n]) for n in og.ACTOR_PARAMS), obs_shift=t(a['obs_shift']), obs_scale=t(a['obs_scale']), activation=a['activation'])
    if mean_mode:
        pol.mean_mode, pol.tensors['act_scale'] = 1, t(a['act_scale'])
    crs = [QCritic(*(t(cr[n]) for n in ('W1', 'b1', 'W2', 'b2', 'W2a', 'W3', 'b3')), kind=cr['kind'], act_scale=t(cr['act_scale']),
                   obs_shift=t(cr['obs_shift']), obs_scale=t(cr['obs_scale']), activation=cr['activation']) for cr in c['critics']]
    obs, idx = t(c['obs']), t(c['idx'])
    gs = critic_gradient(crs if pair else crs[0], obs, t(c['action']), t(c['target']), idx=idx, n_blocks=n_blocks)
    aout, dq = (torch.full((rows, k), float('nan'), dtype=obs.dtype, device=device) for _ in range(2))
    ga = actor_gradient(pol, crs[0], obs, idx=idx, action_out=aout, dqda_out=dq, n_blocks=n_blocks)
    out = {'actor/flat': ga.flat, 'actor/stats': ga.stats, 'actor/action_out': aout, 'actor/dqda_out': dq}
    for j, g in enumerate(gs if pair else [gs]):
        out.update({'critic%d/flat' % j: g.flat, 'critic%d/stats' % j: g.stats})
    return _keyed('offgrad', case, dt, out)


def run_soft(case, dt, device='cuda:0'):
    """{key: numpy array} of one case of libatacom_soft.so in one dtype."""
    import torch
    import soft_oracle as so
    from rl_on_manifold_amd import MlpPolicy, SoftCritic, soft_actor_gradient, soft_critic_gradient, soft_td_target
    rows, n_blocks, D, k, activation, normalise, with_act, critics, gather = case
    c = so.case(4000 + SOFT_CASES.index(case), D, k, activation, normalise, with_act, GATHER[1] if gather else rows, dtype=NP[dt],
                n_idx=rows if gather else 0)
    t = lambda a: _t(a, device)                                                           # noqa: E731
    mu, sg = c['policy']['mu'], c['policy']['sigma']
    pol = MlpPolicy(*(t(mu[n]) for n in so.PARAMS), obs_shift=t(mu['obs_shift']), obs_scale=t(mu['obs_scale']), activation=mu['activation'],
                    sigma_weights=[t(sg[n]) for n in so.PARAMS], squash=True, log_std_min=c['policy']['log_std_min'],
                    log_std_max=c['policy']['log_std_max'])
    mk = lambda cr: SoftCritic(*(t(cr[n]) for n in so.PARAMS), n_act=k, obs_shift=t(cr['obs_shift']),          # noqa: E731
                               obs_scale=t(cr['obs_scale']), activation=cr['activation'])
    crs, tgs = [mk(cr) for cr in c['critics']], [mk(cr) for cr in c['targets']]
    obs, eps = t(c['obs']), t(c['eps'])
    la = torch.tensor([c['log_alpha']], dtype=obs.dtype, device=device)
    kw = dict(act_scale=t(c['act_scale']), act_shift=t(c['act_shift']), idx=t(c['idx']), n_blocks=n_blocks)
    nan = lambda *s: torch.full(s, float('nan'), dtype=obs.dtype, device=device)          # noqa: E731
    out = {'target/action': nan(rows, k), 'target/logp': nan(rows), 'actor/action': nan(rows, k), 'actor/logp': nan(rows),
           'actor/q': nan(rows, 2), 'actor/dqda': nan(rows, k)}
    out['target/y'] = soft_td_target(pol, tgs, obs, t(c['reward']), t(c['absorbing']), c['gamma'], la, eps, action_out=out['target/action'],
                                     logp_out=out['target/logp'], **kw)
    if critics:
        gs = soft_critic_gradient(crs if critics == 2 else crs[0], obs, t(c['action']), t(c['target']), idx=kw['idx'], n_blocks=n_blocks)
        for j, g in enumerate(gs if critics == 2 else [gs]):
            out.update({'critic%d/flat' % j: g.flat, 'critic%d/stats' % j: g.stats})
    ga = soft_actor_gradient(pol, crs, obs, eps, la, c['target_entropy'], action_out=out['actor/action'], logp_out=out['actor/logp'],
                             q_out=out['actor/q'], dqda_out=out['actor/dqda'], **kw)
    out.update({'actor/mu': ga.mu.flat, 'actor/sigma': ga.sigma.flat, 'actor/stats': ga.stats})
    return _keyed('soft', case, dt, out)
