"""Inputs of the tests of libatacom_returns.so, shared by the CPU tests of the oracle (test_returns_oracle.py) and the GPU tests
(test_gpu_returns.py): seeded rewards, values and flag patterns as float64 numpy arrays [W, T, Bm]."""
import numpy as np

PATTERNS = ('no_last', 'last_everywhere', 'last_at_edges', 'consecutive_ends', 'absorbing_with_and_without_last', 'nan_under_absorbing')
GAMMA_LAM = ((0.99, 0.95), (1.0, 1.0), (0.99, 0.0), (0.0, 0.5))


def make_case(T, B, pattern='consecutive_ends', seed=0, W=1, last_rate=0.1):
    """dict(reward, absorbing, last, v, v_next) [W, T, B]; flags as bool.  Rewards carry the occasional large value (the goal
    and penalty rewards of the tasks), values are of the rewards' order."""
    rng = np.random.default_rng([seed, T, B, W, PATTERNS.index(pattern)])
    shape = (W, T, B)
    r = rng.normal(0.0, 1.0, shape) + np.where(rng.random(shape) < 0.02, rng.normal(0.0, 80.0, shape), 0.0)
    v, vn = rng.normal(0.0, 3.0, shape), rng.normal(0.0, 3.0, shape)
    ab, last = np.zeros(shape, bool), np.zeros(shape, bool)
    if pattern == 'last_everywhere':
        last[:] = True
        ab = rng.random(shape) < 0.3
    elif pattern == 'last_at_edges':
        last[:, 0], last[:, -1] = True, True
        ab[:, 0] = rng.random((W, B)) < 0.5
    elif pattern == 'consecutive_ends':
        last = rng.random(shape) < last_rate
        if T > 1:
            last[:, 1:] |= last[:, :-1] & (rng.random((W, T - 1, B)) < 0.5)       # an end right after an end
        ab = last & (rng.random(shape) < 0.5)
    elif pattern == 'absorbing_with_and_without_last':
        last = rng.random(shape) < last_rate
        ab = (last & (rng.random(shape) < 0.5)) | (rng.random(shape) < 0.1)
    elif pattern == 'nan_under_absorbing':
        last = rng.random(shape) < 0.2
        ab = last & (rng.random(shape) < 0.7)
        ab[:, -1] = True
        last[:, -1] = True
        vn = np.where(ab, np.where(rng.random(shape) < 0.5, np.nan, np.inf), vn)
    return dict(reward=r, absorbing=ab, last=last, v=v, v_next=vn)


def ragged_sizes(W, B):
    """Block sizes of a ragged gather padded to B: the first block full, the others one short (e.g. [5, 4, 4])."""
    return [B] + [max(B - 1, 0)] * (W - 1)
