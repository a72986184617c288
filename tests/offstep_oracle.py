"""The oracle of libatacom_offstep.so (include/atacom_offstep_hip.h): one tracked step -- the Adam step of tests/optim_oracle.py,
then the target's three-operation soft update from the value just written -- restated in numpy float64 (tracked64) and, in the
same order of individually rounded operations, in numpy float32 (tracked32).  A group is ONE flat vector of N values in the order
of its gradient (W1, b1, W2, b2, W3, b3, W2a): the arithmetic is elementwise and the layout is the tests' concern.  A helper
module: it holds no test."""
import numpy as np

from optim_oracle import BETAS, EPS, LR, fresh_head, gradients, step32, step64      # noqa: F401

TAU = 5e-3
# (n_in, n_out, n_act): the smallest and the largest plain network, a point-sized DDPG critic, the largest critic (a TD3 critic
# with D + k = 32 has the same sizes): N = 4353, 6792, 4545, 6849
SHAPES = ((1, 1, 0), (32, 8, 0), (3, 1, 1), (32, 1, 8))


def group_size(n_in, n_out, n_act):
    return 64 * n_in + 64 + 4096 + 64 + 64 * n_out + n_out + 64 * n_act


def segments(n_in, n_out, n_act):
    """[(name, shape)] in the order of the flat vector."""
    out = [('W1', (64, n_in)), ('b1', (64,)), ('W2', (64, 64)), ('b2', (64,)), ('W3', (n_out, 64)), ('b3', (n_out,))]
    return out + ([('W2a', (64, n_act))] if n_act else [])


def follow(p, target, tau, dtype):
    """target <- fl(fl(a * p) + fl(b * target)) with a = (T) tau, b = (T)(1.0 - tau): three individually rounded operations."""
    f = np.dtype(dtype).type
    p, target = np.asarray(p, dtype=f), np.asarray(target, dtype=f)
    a, b = f(tau), f(1.0 - tau)
    x = a * p
    z = b * target
    out = x + z
    assert out.dtype == f
    return out


def _tracked(step, dtype, p, grad, m, v, head, target, lr, scale, betas, eps, tau):
    f = np.dtype(dtype).type
    if grad is None:                                         # not stepped: p, m, v and the head keep their bits
        o = dict(p=np.asarray(p, dtype=f), m=np.asarray(m, dtype=f), v=np.asarray(v, dtype=f), head=head)
    else:
        o = step(p, grad, m, v, head, lr=lr, scale=scale, betas=betas, eps=eps)
    o['target'] = None if target is None else follow(o['p'], target, tau, dtype)
    return o


def tracked64(p, grad, m, v, head, target=None, lr=LR, scale=1.0, betas=BETAS, eps=EPS, tau=TAU):
    """One tracked step in float64 -> dict(p, m, v, head, target (None without one), and step64's intermediates when stepped).
    grad None: the group is not stepped and only its target follows."""
    return _tracked(step64, np.float64, p, grad, m, v, head, target, lr, scale, betas, eps, tau)


def tracked32(p, grad, m, v, head, target=None, lr=LR, scale=1.0, betas=BETAS, eps=EPS, tau=TAU):
    """The same with every elementwise operation an individually rounded float32 one; the head and the scalars are formed in
    float64 and rounded once."""
    return _tracked(step32, np.float32, p, grad, m, v, head, target, lr, scale, betas, eps, tau)


_cases = {}


def case(shape, dtype, steps=3):
    """The inputs of `steps` consecutive tracked steps of one group from a fresh state: dict(p, target in `dtype`, grads [steps, N]
    in `dtype` with magnitudes 1e-12 .. 1e3 and exact zeros).  Made once per (shape, dtype) and never written to."""
    key = (shape, np.dtype(dtype).name, steps)
    if key not in _cases:
        N = group_size(*shape)
        rng = np.random.default_rng(2000 + N)
        c = dict(p=rng.normal(0.0, 0.3, N).astype(dtype), target=rng.normal(0.0, 0.3, N).astype(dtype),
                 grads=np.stack([gradients(rng, N) for _ in range(steps)]).astype(dtype))
        for a in c.values():
            a.setflags(write=False)
        _cases[key] = c
    return _cases[key]
