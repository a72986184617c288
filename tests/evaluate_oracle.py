"""Float64 restatement of what libatacom_evaluate.so computes (include/atacom_evaluate_hip.h; test infrastructure only): the
2 x 64 network with its observation normalisation and the log-probability of a diagonal Gaussian around its output, with the
forward error bound a float32 evaluation is held to, per sample.  A helper module: it holds no test.

PINNED: tests/test_evaluate_oracle.py checks `forward` against torch.nn modules and `log_prob` against
torch.distributions.MultivariateNormal, both in float64, to 1e-12.

The float32 bound (DESIGN.md section 7b has the derivation).  u = 2^-24, gamma(n) = n u / (1 - n u).  With e the bound on the
error of a layer's input h (elementwise, absolute), the pre-activation a = W h + b computed in float32 in ANY order of
summation, fused or not, satisfies

    |a^ - a|  <=  |W| e  +  gamma(n + 1) (|W| (|h| + e) + |b|)            n = the layer's inputs, padded to a multiple of 4

(every product and the bias pass through at most n + 1 roundings; the zeros a matrix-core tile is padded with add none).  The
activations are 1-Lipschitz; max(a, 0) is exact, and the device's tanh (csrc/atacom_linalg.h: num<float>::tanh) adds TANH_ABS =
3e-7 of absolute error.  The input is (x - shift) * scale: two roundings, e = gamma(2) |x_n|.  The output's bound is multiplied
by SAFETY = 2: the one factor that is not derived -- the matrix cores are not documented to round every partial sum of their
4-term dot products to nearest, and an adder that chops has unit roundoff 2 u.

For the log-probability, z = (a - mean) / std carries  dz = (e_mean / std) (1 + gamma(4)) + gamma(4) |z|  (the device spends two
roundings on it, a subtraction and an IEEE division; four also admit an evaluation that recovers std from the covariance, as
torch's MultivariateNormal does), and

    |logp^ - logp|  <=  sum_k (|z_k| dz_k + dz_k^2 / 2)  +  gamma(n_out + 3) (sum_k (|z_k| + dz_k)^2 / 2 + sum_k |log std_k| + n_out log(2 pi) / 2)

where the second term is the rounding of the sum in any order and of its constants in float32 (the device forms the constant in
double and rounds it once, inside this).
"""
import math

import numpy as np

U32 = 2.0 ** -24
TANH_ABS = 3e-7
SAFETY = 2.0
LOG_2PI = math.log(2.0 * math.pi)


def gamma(n, u=U32):
    return n * u / (1.0 - n * u)


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _act(a, activation):
    return np.maximum(a, 0.0) if activation == 'relu' else np.tanh(a)


def forward(net, x):
    """net: dict with W1 [64, n_in], b1, W2, b2, W3 [n_out, 64], b3, optional obs_shift / obs_scale [n_in] (None = identity) and
    activation 'relu' / 'tanh'; x [R, n_in].  -> (y [R, n_out] float64, e32 [R, n_out]: the float32 bound above, scale
    [R, n_out]: |W3| |h2| + |b3|, the magnitude a float64 evaluation is measured against)."""
    x = _f64(x)
    act = net.get('activation', 'relu')
    shift, scale = _f64(net.get('obs_shift')), _f64(net.get('obs_scale'))
    h = (x - (0.0 if shift is None else shift)) * (1.0 if scale is None else scale)
    e = gamma(2) * np.abs(h)
    mag = None
    for li, (Wk, bk) in enumerate((('W1', 'b1'), ('W2', 'b2'), ('W3', 'b3'))):
        W, b = _f64(net[Wk]), _f64(net[bk])
        n = 4 * ((W.shape[1] + 3) // 4)
        a = h @ W.T + b
        mag = np.abs(h) @ np.abs(W).T + np.abs(b)
        e = e @ np.abs(W).T + gamma(n + 1) * ((np.abs(h) + e) @ np.abs(W).T + np.abs(b))
        if li < 2:
            h = _act(a, act)
            if act == 'tanh':
                e = e + TANH_ABS
        else:
            h = a
    return h, SAFETY * e, mag


def log_prob(net, x, action, std):
    """-> (logp [R] float64, e32 [R]: its float32 bound, scale [R]: the magnitude a float64 evaluation is measured against,
    y, e32_y): the diagonal Gaussian N(forward(net, x), diag(std^2)) at `action` [R, n_out]."""
    y, ey, mag = forward(net, x)
    a, s = _f64(action), _f64(std)
    k = s.shape[0]
    z = (a - y) / s
    const = np.abs(np.log(s)).sum() + 0.5 * k * LOG_2PI
    logp = (-0.5 * z * z - np.log(s)).sum(-1) - 0.5 * k * LOG_2PI
    dz = (ey / s) * (1.0 + gamma(4)) + gamma(4) * np.abs(z)
    e = (np.abs(z) * dz + 0.5 * dz * dz).sum(-1) + gamma(k + 3) * ((0.5 * (np.abs(z) + dz) ** 2).sum(-1) + const)
    scale = (np.abs(z) * (mag + np.abs(a)) / s + 0.5 * z * z).sum(-1) + const
    return logp, e, scale, y, ey


def random_net(rng, n_in, n_out, activation='relu', normalise=True, dtype=np.float32):
    """A network of the reference's initialisation scale (uniform +- sqrt(6 / (fan_in + fan_out)), biases of the same order)
    whose values are exactly representable in `dtype`; shift / scale of O(1) when `normalise`."""
    def lin(o, i):
        lim = math.sqrt(6.0 / (i + o))
        return rng.uniform(-lim, lim, (o, i)).astype(dtype), rng.uniform(-0.3, 0.3, o).astype(dtype)
    W1, b1 = lin(64, n_in)
    W2, b2 = lin(64, 64)
    W3, b3 = lin(n_out, 64)
    net = dict(W1=W1, b1=b1, W2=W2, b2=b2, W3=W3, b3=b3, activation=activation, obs_shift=None, obs_scale=None)
    if normalise:
        net['obs_shift'] = rng.uniform(-1.0, 1.0, n_in).astype(dtype)
        net['obs_scale'] = rng.uniform(0.2, 2.0, n_in).astype(dtype)
    return net


# ---- the cases of tests/test_gpu_evaluate.py, shared with tests/test_evaluate_oracle.py (which holds torch's own float32 result
# to the same bound): (n_in, n_out, activation, normalise, rows)
SHAPE_CASES = [(4, 1, 'relu', True, 65), (12, 3, 'tanh', False, 65), (18, 5, 'relu', False, 65), (20, 2, 'tanh', True, 65),
               (25, 1, 'tanh', True, 65), (32, 8, 'relu', True, 65), (32, 8, 'tanh', False, 65)]
# (rows, n_blocks); 600 rows on one workgroup: ten tiles on four wavefronts, so a float32 wavefront walks up to three
ROW_CASES = [(1, 0), (15, 0), (16, 0), (17, 0), (63, 0), (64, 0), (65, 0), (200, 1), (200, 2), (600, 1)]


def case_data(seed, n_in, n_out, activation, normalise, rows, dtype=np.float32):
    """(net, x [rows, n_in], action [rows, n_out], std [n_out]) of a case: observations of O(1), std log-uniform in [1e-2, 2] and
    actions at z = (action - mean) / std spread over [0, 6] with both signs."""
    rng = np.random.default_rng(seed)
    net = random_net(rng, n_in, n_out, activation, normalise, dtype)
    x = rng.normal(0.0, 1.0, (rows, n_in)).astype(dtype)
    std = np.exp(rng.uniform(math.log(1e-2), math.log(2.0), n_out)).astype(dtype)
    y, _, _ = forward(net, x)
    z = rng.uniform(0.0, 6.0, (rows, n_out)) * rng.choice([-1.0, 1.0], (rows, n_out))
    z[0] = 0.0
    action = (y + z * std.astype(np.float64)).astype(dtype)
    return net, x, action, std
