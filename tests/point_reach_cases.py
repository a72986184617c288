"""Constraint-active inputs for the collision-avoidance tests (CPU and GPU): states of the random-walk task in which the
agent sits at, or inside, the boundary d = 0.6 of an obstacle, built on the CPU from the float64 restatement
(tests/point_reach_oracle.py) alone and deterministic in the seed.

The states the task visits from its reset corner (1, 1) keep every obstacle more than 1.4 away for the first hundred
steps: the slack s stays above 1.4, J_c = [J_q | diag(s)] is dominated by its diagonal and the error correction 100 c is
tiny.  Here the agent is PLACED beside obstacle 0 and then runs free for a short prefix, so that s, the velocities and the
obstacles are what the closed loop produces next to the boundary: s below 1e-4 (the slack dynamics ~ 1/s, a nearly
rank-deficient J_c), the cancellation 0.36 - d^2 + s^2 / 2 times 100, a positive constraint log, saturated accelerations.

The lower walls.  The obstacles never leave [2, 10]^2 (base:61) and the agent is placed at most 1.1 from one of them, so
it cannot reach the walls at 0 within the windows the tests run; the walls at 10 it does reach.  The last B // WALL_SHARE
environments therefore start at the lower walls instead (within 0.02 of x = 0 or y = 0, moving towards it, their
obstacles drawn like everyone's and hence at least 1.9 away): the only way the task itself meets those walls.  They skip
the prefix, which would carry them through the wall before the first compared step.

Exact s == 0 and a rank-deficient J_c are not generated: they are not reachable from a reset, and the reference's answer
there is set by an rcond.
"""
import numpy as np

import parity_tools
import point_reach_oracle as pro

WALL_SHARE = 16
# what the GPU tests run (tests/test_gpu_point_reach_active.py) and the CPU tests hold to its purpose
# (tests/test_point_reach_active_oracle.py): one seed per obstacle count, B environments, T teacher-forced steps
B_ACTIVE, T_ACTIVE = 1024, 12
# seeds picked on the census alone (tests/test_point_reach_active_oracle.py): of 31..40 the ones whose smallest |s| is under
# 3e-4 with supplied AND with generator draws (that minimum over 12288 samples is the one figure that moves with the seed)
SEEDS = {2: 35, 4: 35}
FIXTURE_STATES, FIXTURE_SEEDS = 256, {2: 7002, 4: 7004}
MAX_VACUOUS = 0.02          # the ceiling of tests/test_gpu_point_reach.py (held equal to it there), not a new constant


def active_oracle(B, n, seed, prefix=20, gap_lo=1e-3):
    """A PointReachBatched (random walk, no auto-reset) of B constraint-active environments:

      obstacles   positions U(2.5, 9.5)^2, velocities U(-1, 1)
      agent       beside obstacle 0 at distance 0.6 + g, g log-uniform in [gap_lo, 0.5], at a uniform angle; its velocity
                  points at the obstacle (magnitude U(0, 1)) plus U(-0.3, 0.3) jitter per axis
      s           sqrt(max(-2 c, 0)) over all obstacles: the reset formula
      prefix      free steps of the restatement under U(-1, 1) actions and supplied U(-1, 1) draws, which take s off the
                  reset formula and onto what the closed loop produces (with prefix = 0 exact s = 0 appears)
      lower walls the last B // WALL_SHARE environments (module docstring)

    The constraint log is cleared at the end."""
    rng = np.random.default_rng(seed)
    o = pro.PointReachBatched(B, n_objects=n, random_walk=True, seed=seed, auto_reset=False)
    obst = o.state[:, 4:].reshape(B, n, 4)                               # a view
    obst[:, :, 0:2] = rng.uniform(2.5, 9.5, (B, n, 2))
    obst[:, :, 2:4] = rng.uniform(-1.0, 1.0, (B, n, 2))
    g = np.exp(rng.uniform(np.log(gap_lo), np.log(0.5), B))
    ang = rng.uniform(0.0, 2 * np.pi, B)
    u = np.stack([np.cos(ang), np.sin(ang)], 1)
    o.state[:, 0:2] = obst[:, 0, 0:2] + (0.6 + g)[:, None] * u
    o.state[:, 2:4] = -u * rng.uniform(0.0, 1.0, (B, 1)) + rng.uniform(-0.3, 0.3, (B, 2))

    def slack():
        d = o.state[:, None, 0:2] - o._p()
        return np.sqrt(np.maximum(-2 * (pro.RADIUS2 - (d * d).sum(2)), 0.0))

    o.s = slack()
    o.have_centres[:] = True
    o.episode[:] = 1
    for _ in range(prefix):
        o.step(rng.uniform(-1.0, 1.0, (B, 2)), draws=rng.uniform(-1.0, 1.0, (B, n, 2)))
    w = B // WALL_SHARE
    if w:
        axis = np.arange(w) % 2
        q = rng.uniform(0.5, 9.5, (w, 2))
        dq = rng.uniform(-0.3, 0.3, (w, 2))
        q[np.arange(w), axis] = rng.uniform(0.0, 0.02, w)
        dq[np.arange(w), axis] = -rng.uniform(0.2, 1.0, w)
        o.state[B - w:, 0:2], o.state[B - w:, 2:4] = q, dq
        o.s[B - w:] = slack()[B - w:]
    o.get_constraints_logs()
    return o


def forced_inputs(n, seed, T=T_ACTIVE, B=B_ACTIVE):
    """The actions [T, B, 2] in U(-1.2, 1.2) and supplied draws [T, B, n, 2] in U(-1, 1) of a teacher-forced test."""
    rng = np.random.default_rng(seed + 100)
    return rng.uniform(-1.2, 1.2, (T, B, 2)), rng.uniform(-1.0, 1.0, (T, B, n, 2))


def fixture_states(n, seed=None, count=FIXTURE_STATES):
    """(state [count, 4 (1 + n)], s [count, n]): the inputs of tests/golden/point_reach_active.npz.  A pool of
    B_ACTIVE x T_ACTIVE states (active_oracle stepped through forced_inputs, the state before each step) of which a quarter
    are the ones with the smallest |s|, a quarter the ones deepest inside an obstacle, an eighth steps onto or beyond a wall
    (the lower and the upper ones in turn) and the rest evenly spaced over the remainder -- a selection by the
    restatement's own quantities, in a fixed order.  States whose |s| exceeds 100 are not eligible: an environment whose s
    came within 1e-6 of zero has it thrown to 1e4 .. 1e8 by the slack rate 100 c / s (and halved per step from there), and
    the fixture's absolute 1e-12 is below the spacing of float64 at those magnitudes (1.5e-8 at 1e8)."""
    seed = FIXTURE_SEEDS[n] if seed is None else seed
    o = active_oracle(B_ACTIVE, n, seed)
    acts, draws = forced_inputs(n, seed)
    st, ss = [], []
    for t in range(T_ACTIVE):
        st.append(o.state.copy()); ss.append(o.s.copy())
        o.step(acts[t], draws=draws[t])
    st, ss = np.concatenate(st), np.concatenate(ss)
    d = st[:, None, 0:2] - st[:, 4:].reshape(len(st), n, 4)[:, :, 0:2]
    depth = (pro.RADIUS2 - (d * d).sum(2)).max(1)
    qn = st[:, 0:2] + st[:, 2:4] * o.dt
    low, high = np.flatnonzero((qn <= 0).any(1)), np.flatnonzero((qn >= 10).any(1))
    chosen = []
    seen = set(np.flatnonzero(np.abs(ss).max(1) > 100.0).tolist())

    def take(order, k):
        new = [i for i in order if i not in seen][:k]
        chosen.extend(new); seen.update(new)
    take(np.argsort(np.abs(ss).min(1), kind='stable'), count // 4)
    take(np.argsort(-depth, kind='stable'), count // 4)
    take(low, count // 16)
    take(high, count // 16)
    rest = np.array([i for i in range(len(st)) if i not in seen])
    k = count - len(chosen)
    take(rest[(np.arange(k) * len(rest)) // k], k)
    idx = np.array(chosen)
    assert len(idx) == count == len(set(chosen))
    return st[idx].copy(), ss[idx].copy()


def step_outputs(p, inputs):
    """What is compared per sample: the observation after the step, s after the step, the reward."""
    obs, r, _, _ = p.step(inputs[0], draws=inputs[1])
    return np.concatenate([obs, p.s, r[:, None]], 1)


def clip_state(dq0, flip, dq1, boundary=1 - 1e-9, dt=0.01):
    """Per axis (class, a): a = the acceleration after the clip in units of its bound, read off the velocity update with
    the wall flip `flip` undone; class -1 / 0 / +1 = clip low / inactive / high, |a| >= boundary counting as clipped (a
    clipped axis shows |a| = 1 to the rounding of the build: 1e-15 in float64, 1e-5 in float32)."""
    a = (np.where(flip, -dq1, dq1) - dq0) / (pro.ACTION_SCALE * dt)
    return np.where(a >= boundary, 1, np.where(a <= -boundary, -1, 0)), a


def census(o, actions, draws):
    """What the inputs of a teacher-forced test exercise: `o` (left untouched) is stepped through actions [T, B, 2] and
    draws [T, B, n, 2] (None: the generator's); the counts are over the T x B samples (the state BEFORE each step is the
    sample's input)."""
    p = parity_tools.slice_env(o, np.arange(o.B))
    T = len(actions)
    dmin, smin, flips, clips = [], [], np.zeros((2, 2), dtype=np.int64), []
    for t in range(T):
        d = p.state[:, None, 0:2] - p._p()
        dmin.append(np.sqrt((d * d).sum(2)).min(1))
        smin.append(np.abs(p.s).min(1))
        dq0 = p.state[:, 2:4].copy()
        obs, _, _, _ = p.step(actions[t], draws=None if draws is None else draws[t])
        cs, _ = clip_state(dq0, (obs[:, 0:2] <= 0) | (obs[:, 0:2] >= 10), obs[:, 2:4], dt=p.dt)
        clips.append(cs)
        flips[:, 0] += (obs[:, 0:2] <= 0).sum(0)
        flips[:, 1] += (obs[:, 0:2] >= 10).sum(0)
    dmin, smin, clips = np.array(dmin), np.array(smin), np.array(clips)
    log = p.get_constraints_logs()
    return {'samples': dmin.size, 'min_d': float(dmin.min()), 'inside': float((dmin < 0.6).mean()),
            'within_0.8': float((dmin < 0.8).mean()), 'min_abs_s': float(smin.min()),
            'wall_flips': int(flips.sum()), 'wall_flips_axis_low_high': flips.tolist(),
            'clip_low': float((clips == -1).mean()), 'clip_inactive': float((clips == 0).mean()),
            'clip_high': float((clips == 1).mean()), 'log_mean': float(log[0]), 'log_max': float(log[1])}
