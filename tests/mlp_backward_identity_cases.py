"""The runs behind tests/golden/mlp_backward_identity.npz: what libatacom_fit.so (value_gradient, policy_gradient) and
libatacom_trust.so (fisher_vector_product) return where the code the two share decides the result -- the walk over the rows, the
transposition buffers, the backward pass through the 2 x 64 network, the hand-over between the wavefronts and the reduction of
the partials.  Recorded once (profiles/tools/gen_mlp_backward_identity_golden.py, on the commit before that code moved into
csrc/mlp/atacom_mlp_backward.h) and compared bit for bit ever since (tests/test_gpu_mlp_backward_identity.py).

Rows and grids: a lone row (fifteen dead lanes of its 16-block), 17 (a part-filled second block), 65 (a second wavefront's tile
holding one row), 200 over two workgroups (all four wavefronts hand over, two partials are reduced), 600 in one workgroup (every
wavefront walks more than one tile with its accumulators live), and 70 of 200 rows gathered through a shuffled idx with repeats.
Shapes (n_in, n_out): (4, 2) is CH = 1 with one input tile, (18, 5) CH = 5 with a padded last K-step and a part-filled second
input tile, (25, 1) CH = 7, (32, 8) CH = 8 with both tiles and both output quads full; a critic has n_out = 1.  Both activations
and the observation normalisation on and off appear in each library; the product runs with damping 0 and 0.1.  Every grid is
given or 0 (the library's choice depends on the row count only).  Every case runs in float32 and float64.

The golden holds every value of every output, so the cases are few: each row count appears once per library, at shapes that
between them cover every CH path above."""
import numpy as np

DTYPES = ('f32', 'f64')
CLIP = 0.2
GATHER = (70, 200)            # rows read, rows there

# (rows, n_blocks, n_in, n_out, activation, normalise, gather)
_ROWS = [
    (1, 0, 4, 2, 'relu', True, False),
    (17, 0, 18, 5, 'tanh', False, False),
    (65, 0, 25, 1, 'tanh', True, False),
    (200, 2, 18, 5, 'tanh', True, False),
    (600, 1, 32, 8, 'relu', False, False),
    (70, 0, 18, 5, 'relu', True, True),
]
# head, then the above; the critic takes the shapes with n_out = 1
FIT_CASES = [('ppo',) + c if c[3] > 1 else ('value',) + c for c in _ROWS] + [('value', 600, 1, 18, 1, 'relu', False, False)]
# damping, then the above, the row counts met by other shapes and the other normalisation
TRUST_CASES = [
    (0.1, 1, 0, 18, 5, 'tanh', True, False),
    (0.0, 17, 0, 4, 2, 'relu', False, False),
    (0.1, 65, 0, 25, 1, 'tanh', False, False),
    (0.0, 200, 2, 32, 8, 'relu', True, False),
    (0.1, 600, 1, 18, 5, 'relu', True, False),
    (0.0, 70, 0, 18, 5, 'tanh', True, True),
    (0.0, 200, 2, 18, 5, 'tanh', False, False),
]
FIT_FIELDS, TRUST_FIELDS = ('flat', 'stats'), ('product',)


def case_id(lib, case):
    return '%s_%s' % (lib, '_'.join(str(c) for c in case))


def _inputs(seed, rows, n_in, n_out, activation, normalise, gather):
    """Everything a case reads, drawn in float64: the network, std, the rows, idx and, for the policy gradient, logp_old a
    perturbation of the row's own log-probability, so that rows fall on both sides of the clip."""
    rng = np.random.default_rng(seed)
    there = GATHER[1] if gather else rows
    d = dict(W1=rng.normal(0, 1 / np.sqrt(n_in), (64, n_in)), b1=rng.normal(0, 0.1, 64), W2=rng.normal(0, 0.125, (64, 64)),
             b2=rng.normal(0, 0.1, 64), W3=rng.normal(0, 0.125, (n_out, 64)), b3=rng.normal(0, 0.1, n_out),
             std=rng.uniform(0.5, 1.5, n_out), shift=rng.normal(0, 0.5, n_in), scale=rng.uniform(0.5, 2.0, n_in),
             x=rng.normal(0, 1, (there, n_in)), noise=rng.normal(0, 1, (there, n_out)), adv=rng.normal(0, 1, there),
             target=rng.normal(0, 1, there), wobble=rng.normal(0, 0.3, there),
             v=rng.normal(0, 1, 64 * n_in + 64 + 4096 + 64 + 64 * n_out + n_out + n_out))
    if not normalise:
        d['shift'] = d['scale'] = None
    act = np.tanh if activation == 'tanh' else (lambda a: np.maximum(a, 0.0))
    xn = d['x'] if not normalise else (d['x'] - d['shift']) * d['scale']
    mu = act(act(xn @ d['W1'].T + d['b1']) @ d['W2'].T + d['b2']) @ d['W3'].T + d['b3']
    d['action'] = mu + d['std'] * d['noise']
    logp = -0.5 * (d['noise'] ** 2).sum(-1) - np.log(d['std']).sum() - 0.5 * n_out * np.log(2 * np.pi)
    d['logp_old'] = logp + d['wobble']
    d['idx'] = None
    if gather:
        pick = rng.permutation(there)[:rows - 6]
        d['idx'] = np.concatenate([pick, pick[:6]])[rng.permutation(rows)].astype(np.int64)
    return d


def _on_device(d, dt, activation, device):
    import torch
    from rl_on_manifold_amd import MlpPolicy
    dtype = {'f32': torch.float32, 'f64': torch.float64}[dt]

    def t(a):
        return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype if a.dtype != np.int64 else None).to(device)

    pol = MlpPolicy(*(t(d[k]) for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')), std=t(d['std']), obs_shift=t(d['shift']),
                    obs_scale=t(d['scale']), activation=activation)
    return pol, t


def run_fit(case, dt, device='cuda:0'):
    """{key: numpy array} of one case of libatacom_fit.so in one dtype; keys are prefixed with the case id and the dtype."""
    from rl_on_manifold_amd import fit
    head, rows, n_blocks, n_in, n_out, activation, normalise, gather = case
    d = _inputs(1000 + FIT_CASES.index(case), rows, n_in, n_out, activation, normalise, gather)
    pol, t = _on_device(d, dt, activation, device)
    if head == 'value':
        g = fit.value_gradient(pol, t(d['x']), t(d['target']), idx=t(d['idx']), n_blocks=n_blocks)
    else:
        g = fit.policy_gradient(pol, t(d['x']), t(d['action']), t(d['adv']), t(d['logp_old']), clip=CLIP, idx=t(d['idx']),
                                n_blocks=n_blocks)
    cid = case_id('fit', case)
    return {'%s/%s/flat' % (cid, dt): g.flat.cpu().numpy().copy(), '%s/%s/stats' % (cid, dt): g.stats.cpu().numpy().copy()}


def run_trust(case, dt, device='cuda:0'):
    """{key: numpy array} of one case of libatacom_trust.so in one dtype."""
    from rl_on_manifold_amd import trust
    damping, rows, n_blocks, n_in, n_out, activation, normalise, gather = case
    d = _inputs(2000 + TRUST_CASES.index(case), rows, n_in, n_out, activation, normalise, gather)
    pol, t = _on_device(d, dt, activation, device)
    out = trust.fisher_vector_product(pol, t(d['x']), t(d['v']), damping=damping, idx=t(d['idx']), n_blocks=n_blocks)
    return {'%s/%s/product' % (case_id('trust', case), dt): out.cpu().numpy().copy()}
