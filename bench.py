#!/usr/bin/env python3
"""Headline benchmark: env-steps/sec of the batched ATACOM step (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--env iiwa|planar|circle] [--batch B] [--dump-outputs DIR] [--full]

A "step" is ONE call of the hot path over one batch: `atacom_step` (C ABI, one HIP kernel launch) for
B = 8192 IiwaAirHockey-7H environments per GPU -- action clip/scale, 4 x [constraint Jacobians + FK,
null-space projection, slack integration, truncation, dynamics], reward / termination / observation,
constraint statistics, masked auto-reset at the horizon.  Inputs (actions) are resident in HBM before the
timed region.

N > 1: one process per GPU over RCCL.  `python bench.py --gpus N` spawns the N ranks itself (it re-executes
under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1`); launched under
torchrun by someone else it uses the ranks it was given (and refuses a WORLD_SIZE that contradicts --gpus).
Each rank owns its own 8192-env shard (weak scaling, no collective on the data path).

Timing: short timed blocks for --warmup-seconds from a snapshot of the engine, which is then restored (a GPU fresh from
set-up runs its first steps ~4 % slow, and a process's first timed block pays ~0.1 ms extra; the restore keeps the timed
data independent of how many steps that took), W warm-up steps, then ONE block of exactly K steps, bracketed by
barrier + synchronize on both sides, its time = MAX over ranks: `ms_per_step` = that time / K, `value` = all environments
x K / that time.  A plain run does nothing else: set-up, warm-up, the K timed steps, the outputs (--dump-outputs), the
JSON line.

--dump-outputs DIR: after the timed block, what its LAST step returned to the caller -- obs [B, D], reward [B],
absorbing [B] and last [B] (the flags as 0. / 1.) -- is written as DIR/<name>.npy in the engine's float type (rank 0's
shard).  Inputs (initial states, actions) come from seeded generators, so two runs with the same arguments step the
same data.  Above 64 MB in all, the same seeded sample of environments is kept from every array and its row indices are
written as DIR/sample_rows.npy.

--full adds everything else the benchmark measures: after the headline block, further K-step blocks until >= --min-time
seconds have been timed (`timing`: median, p99, max -- a single 20-step block is 0.6 ms, one scheduler hiccup moves it
by 10 %), and the extra objects below.  --no-cpu-baseline / --no-secondary leave parts of it out.

Prints ONE JSON line (rank 0).  Extra objects (--full):
  roofline      the BINDING roof of the step kernel: fp32 vector ALU (bound "valu_f32": algorithmic FLOPs per launch /
                mean kernel time from HIP events on the launch stream; this workload sits at 130 FLOP/B, far right of
                the ridge -- SURVEY.md section 8d); `traffic` = measured HBM bytes per launch
  roofline_hbm  the HBM view of the same kernel (algorithmic bytes per launch / the same kernel time)
  collection    config 5's collection phase: rollout_packed(120 steps, one launch) + the one all-gather of the
                packed records (ms, bytes, GB/s per rank)
  secondary     circle-4096 and planar-8192 (BASELINE configs 2 and 3) with their own rooflines; the iiwa headline
                workload through the Python step() surface, with the opt-in canonical chart (chart_mode 1, its own
                roofline against ITS algorithmic FLOPs), and in the rigid-body modes (N = 1 only)
  cpu_baseline  the float64 oracle timed on this box's host cores on bounded samples (rank 0, N = 1 only):
                scalar reference-shaped (1 core and all cores) and batched numpy; + the oracle's constraint
                statistics on 256 of the very same initial states and actions next to the device's
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s
VALU_F32_PEAK_TF = 157.3       # MI355X_MICROARCH.md: peak FP32 vector

# algorithmic HBM bytes per env-step, fp32, sub-steps fused (SURVEY.md section 8d / BASELINE.md section 4;
# derivation in DESIGN.md "Measurement"): state read once + written once, action in, obs/reward/flags out.
ALGO_BYTES = {'circle': 60, 'planar': 220, 'iiwa': 400}
SHAPES = {'circle': (2, 3, 1, 2, 1), 'planar': (6, 9, 3, 3, 4), 'iiwa': (12, 17, 5, 6, 4)}   # c, n, k, nq, substeps
WORKLOAD = {'iiwa': 'IiwaAirHockey env 7H', 'planar': 'PlanarAirHockey env H', 'circle': 'CircularMotion env A'}
IIWA_INIT_Q = [0.0, 0.7135214629060707, 0.0, -0.5024756033561426, 0.0, 1.9256631778550268]


def algorithmic_flops(env):
    """FLOPs per env-step of the algorithm the kernel runs (FMA = 2), counted loop by loop
    (rl_on_manifold_amd/csrc/atacom_linalg.h); selects / compares / moves are not counted."""
    M, N, K, nq, sub = SHAPES[env]
    f = 0
    for i in range(M):
        f += 2 * (N - 1 - i) + 12 + (N - 1 - i)                       # norm, larfg, scale v
        if i < M - 1:
            f += (M - 1 - i) * (4 * (N - 1 - i) + 3)                  # G(i) on the rows below
            f += 2 * (M - 2 - i) + 12 + (M - 2 - i)                   # norm, larfg, scale u
            f += (N - 1 - i) * (4 * (M - 2 - i) + 3)                  # H(i) on the columns right
            f += 4 * (M - 2 - i) + 3                                  # H(i) on the rhs
    f += 3 * M                                                        # bidiagonal solve
    f += sum((1 + K) * (4 * (N - 1 - i) + 3) for i in range(M))       # P applied to [x | null]
    f += sum((N - 1 - j) * (1 + 2 * K) + 2 for j in range(K))         # rref, K pivots
    f += 2 * N * K + N                                                # Nc @ alpha - x
    f += 6 * M + 14 * nq                                              # rhs assembly, slack, truncation, integration
    per_sub = f
    return sub * per_sub + sum(once_per_step_flops(env).values())


def once_per_step_flops(env):
    """FLOPs of what an env step does ONCE (not per physics sub-step, with the reference's zero-order hold of q, dq): counted
    operation by operation from rl_on_manifold_amd/csrc/atacom_envs.h (constraint_terms, constraint_fun, bias_mode 0) and
    atacom_kernels.h (env_step: assembly, puck sub-steps, reward, truncation bounds); FMA = 2, add / mul / div / sqrt / rcp = 1,
    sincos / exp = 20 (the convention of algorithmic_flops_dyn); negations, selects, compares, abs / min / max not counted.
    (Rounds 1 - 5 carried an ESTIMATE here -- 2 x 1500 for iiwa: 1.8 kFLOP, 3.4 % of the step, too many.)"""
    M, N, K, nq, sub = SHAPES[env]
    nnz = sum(ROW_NNZ[env])
    sincos, exp = 20, 20
    assembly = 2 * nnz + 2 * nnz + 6 * M                     # J dq, K J, (psi, c0, yb) per row
    trunc = 4 * nq                                            # acc_truncation bounds (atacom.py:117-121)
    action = 3 * K                                            # clip * alpha_max, |alpha|^2
    # puck: per physics sub-step mallet interpolation 5, integration 6, distance 6 + rcp, normal 2, relative velocity 5,
    # impulse 2 + 4, push-out 4, rims 8, hit latch 3 = 46;  reward / termination: 3 + distances 8 + 2 rcp + cosine 5 + exp + 6
    puck = 46 * sub + 3 + 8 + 2 + 5 + exp + 6
    if env == 'circle':
        terms = 4 + 1 + 2 + 5                                 # f, g, J_f, b_f  (circle_atacom.py:47-70)
        post = 0
        other = 5 + 2 * 8 + 5 + exp                           # pre-step log, base integration (circle_base.py:59-63), reward
        return {'constraint_terms': terms, 'assembly': assembly, 'post_step_kinematics': post, 'truncation_bounds': trunc,
                'action': action, 'base_env': other}
    if env == 'planar':
        fk = 3 * sincos + 3 + 6                               # planar_fk: cumulative angles, link vectors
        terms = fk + 6 + 3 + 6 + 12 + 3 + 2 + 9 + 3 + 6       # tip, table rows, J sums, v = J dq, w, w x v, limits, 2 q, 2 dq^2
        post = fk + 6 + 3 + 9
    else:
        chain = 6 * (6 + 9 + 9) + 12                          # iiwa_chain: origin, two rotated axes per joint; link_7 + tip
        fk = 6 * sincos + chain
        jac = 12 * (6 + 6 + 2)                                # jac_col: z x (p - o), tip / link_7 (6 columns) / link_4 (2)
        bias = 2 * (36 + 36 + 9) + (24 + 24 + 9)              # frame_bias mode 0: w, v = J dq, w x v (6-, 6-, 4-joint frames)
        terms = fk + jac + bias + 8 + 18 + 6 + 12             # table / height rows, limits, 2 q, 2 dq^2
        post = fk + 8 + 18
    return {'constraint_terms': terms, 'assembly': assembly, 'post_step_kinematics': post, 'truncation_bounds': trunc,
            'action': action, 'puck_reward_termination': puck}


# structural non-zeros per row of K J (rl_on_manifold_amd/csrc/atacom_envs.h: jac_zero), equality row first
ROW_NNZ = {'circle': [2, 2], 'planar': [3, 3, 3, 1, 1, 1], 'iiwa': [6, 6, 6, 6, 2, 6, 1, 1, 1, 1, 1, 1]}


def algorithmic_flops_canonical(env):
    """FLOPs per env-step of the canonical chart as the kernel runs it (rl_on_manifold_amd/csrc/atacom_chart.h, square-root
    recursion on the extended state N1 = dim_q + 1; FMA = 2; the slack stage counted once -- it runs in 14 % of the iiwa
    sub-steps; stiff-row steps, selects and compares not counted)."""
    M, N, K, nq, sub = SHAPES[env]
    nf = M - (N - nq)
    nnz = ROW_NNZ[env]
    g_rows = nnz[nf:]
    n1 = nq + 1
    f = sum(z * (z + 1) // 2 + 2 * z for z in g_rows)                  # M, b
    f += nq ** 3 // 3 + nq * nq                                       # Cholesky, its inverse
    f += nq * (nq + 1)                                                # x = -Gamma b
    cond = lambda z: z * n1 + n1 + 2 * n1 * n1 + z + n1               # noqa: E731  vector, norm, project, residual, x
    f += cond(nnz[0]) if nf else 0
    f += nq * (n1 + 2 * n1 * n1 + n1)                                 # joint recursion
    f += 3 * n1 * n1 + 2 * sum(g_rows) + 3 * len(g_rows)              # slack stage (B)
    f += 4 * nq + 2 * sum(g_rows) + 3 * len(g_rows)                   # equality row once more, slack velocities
    per_sub = 2 * f + 6 * M + 14 * nq
    return sub * per_sub + sum(once_per_step_flops(env).values())


def algorithmic_flops_dyn():
    """FLOPs the rigid-body mode (row N4, dynamics_mode 1 / 2) adds to one iiwa env-step: per physics sub-step the nine sines /
    cosines, one Newton-Euler pass, the 9 x 6 mass-matrix rows, servo set-points, torque, Cholesky solve -- counted operation
    by operation from rl_on_manifold_amd/csrc/atacom_dynamics_link.h (the LINK-COORDINATE recursions the kernels run since
    round 5; the world-coordinate form of rounds 2 - 4 counted 4545 per sub-step) and atacom_kernels.h:rigid_body_substep
    (FMA = 2, a general cross product = 9, a symmetric 3 x 3 product = 15, sincos / acos = 20, moving a vector across a joint
    = 6, a symmetric tensor = 23; selects, compares, sign flips and moves not counted)."""
    cross, sym, trig, xvec, xsym = 9, 15, 20, 6, 23
    trig9 = 9 * trig
    # Newton-Euler, base to tip: origin acceleration (offset along one axis: 15), three vectors into the child frame, the joint's
    # own terms (6), centre-of-mass acceleration (3 cross products), F = m a (9), N = I al + w x (I w) (2 sym + cross + 3)
    fwd = 8 * 15 + 9 * (3 * xvec + 6 + 3 * cross + 9 + 2 * sym + cross + 3)
    # tip to base: c x F, accumulate (9), two vectors into the parent frame, offset moment (4)
    bwd = 9 * (cross + 9) + 8 * (2 * xvec + 4)
    # composites: first moment + tensor into the parent frame, parallel-axis shift along one axis (12), the body's own (10)
    comp = 8 * (xvec + xsym + 12) + 9 * 10
    # rows: (p, L) walked down the chain, 6 + 7 + 8 transforms for the servo rows and 0 .. 5 for the controlled joints
    rows = (15 + 21) * (2 * xvec + 4)
    axes = 7 * 18                                                         # orientation chain for the servo set-points
    servo = (2 * cross + 12 + 3 + 5 + trig + 6) + (trig + cross + 12) + 3 * 8
    solve = 6 * (2 * 9) + 6 * (2 * 5) + (6 ** 3 // 3 + 2 * 36 + 30) + 12                    # torque, right-hand side, Cholesky
    return SHAPES['iiwa'][4] * (trig9 + fwd + bwd + comp + rows + axes + servo + solve)


# ------------------------------------------------------------------------------------------ rank spawning
def _free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def launch_ranks(n):
    """`python bench.py --gpus N` outside torchrun: re-execute under torch.distributed.run, one rank per GPU."""
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('OMP_NUM_THREADS', '1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=%d' % n,
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


# ------------------------------------------------------------------------------------------ synthetic data
def feasible_init(name, B, dev, gen, sigma=0.05):
    """Initial joint states per SURVEY.md section 8d (configs 3 / 4): q = q_init + N(0, sigma^2), one Newton correction
    step onto the equality constraint (iiwa: tip height z_ee = 0.1505), REJECTED unless every inequality g < 0 and
    |f| < 1e-3 afterwards; dq = 0; puck uniform in the hit range (env_hitting.py:11,24-25).  The constraint values
    come from the library's own `atacom_constraint_terms` primitive (C ABI) -- no oracle here.
    Returns ([B, init_state_dim] rows for reset(state=...), fraction of draws rejected)."""
    import torch
    from rl_on_manifold_amd import constraint_terms
    nq, nf = {'planar': (3, 0), 'iiwa': (6, 1)}[name]
    q0 = torch.tensor({'planar': [-0.9273, 0.9273, 3.141592653589793 / 2], 'iiwa': IIWA_INIT_Q}[name],
                      device=dev, dtype=torch.float32)
    keep, drawn = [], 0
    while sum(k.shape[0] for k in keep) < B:
        if drawn > 200 * B:
            raise RuntimeError('feasible_init: fewer than 0.5 %% of the draws are feasible (%s)' % name)
        n = max(B // 2, 1024)
        q = q0 + sigma * torch.randn((n, nq), device=dev, generator=gen)
        dq = torch.zeros_like(q)
        if nf:
            fun, J, _ = constraint_terms(name, q, dq)
            Jf = J[:, 0, :]
            q = q - Jf * (fun[:, :1] / (Jf * Jf).sum(1, keepdim=True))       # one correction step
        fun, _, _ = constraint_terms(name, q, dq)
        ok = (fun[:, nf:] < 0).all(1)
        if nf:
            ok &= fun[:, 0].abs() < 1e-3
        keep.append(q[ok])
        drawn += n
    q = torch.cat(keep)[:B]
    kept_of = sum(k.shape[0] for k in keep)
    init = torch.zeros((B, 2 * nq + 6), device=dev)
    init[:, :nq] = q
    init[:, 2 * nq + 0] = -0.6 + 0.4 * torch.rand((B,), device=dev, generator=gen)
    init[:, 2 * nq + 1] = -0.4 + 0.8 * torch.rand((B,), device=dev, generator=gen)
    return init, 1.0 - kept_of / drawn


def make_env(name, B, dev, gen, lanes=0, dtype=None, **kw):
    import torch
    from rl_on_manifold_amd import BatchedAtacomEnv
    env = BatchedAtacomEnv(name, B, device=dev, dtype=dtype or torch.float32, auto_reset=True, lanes_per_env=lanes, **kw)
    init, rej = None, 0.0
    if name != 'circle':
        init, rej = feasible_init(name, B, dev, gen)
        env.reset(state=init)
    else:
        # half at the reference's fixed reset point, half random valid states
        # (circle_base.py:36-42: a point on the circle above y = -0.5 with a tangential velocity)
        st = torch.zeros((B, 4), device=dev)
        st[:, 0] = -1.0
        h = B // 2
        y = -0.5 + 1.5 * torch.rand((h,), device=dev, generator=gen)
        sg = torch.where(torch.rand((h,), device=dev, generator=gen) < 0.5, -1.0, 1.0)
        x = torch.sqrt((1 - y * y).clamp_min(0)) * sg
        sp = torch.rand((h,), device=dev, generator=gen) * torch.where(torch.rand((h,), device=dev, generator=gen) < 0.5, -1.0, 1.0)
        st[:h, 0], st[:h, 1], st[:h, 2], st[:h, 3] = x, y, -y * sp, x * sp
        init = st
        env.reset(state=st)
    return env, init, rej


# ------------------------------------------------------------------------------------------ the timed loop
def time_steps(env, actions, K, W, min_time, sync_all, max_over_ranks, max_blocks=20000, repeat=True, outputs=None,
               warmup_s=0.0):
    """W warm-up steps, then blocks of exactly K atacom_step launches; returns (per-block seconds [max over ranks],
    mean kernel ms from HIP events on the launch stream over all timed launches).  repeat=False: the first block alone.
    outputs: a dict that receives host copies of what the first block's last step returned (obs, reward, absorbing, last),
    taken before any further block runs.  warmup_s: before the W steps, run blocks of min(K, 100) steps for at least this
    many seconds from a snapshot of the engine and restore it -- the device and this timing path reach their steady state,
    and the W + K steps that follow step the same data however many steps that took."""
    import numpy as np
    import torch
    B, D = env.batch, env.obs_dim
    dev = env.device
    obs = torch.empty((B, D), device=dev, dtype=env.dtype)
    rew = torch.empty((B,), device=dev, dtype=env.dtype)
    ab = torch.empty((B,), device=dev, dtype=torch.uint8)
    last = torch.empty((B,), device=dev, dtype=torch.uint8)
    n_pool = actions.shape[0]
    # the engine's bound form of step_into: arguments validated once per action slice, then one atacom_step call through
    # the C ABI per step (BatchedAtacomEnv.bind_step; the circle step is bound by the host, not by its 4 us kernel)
    steppers = [env.bind_step(actions[i], obs, rew, ab, last) for i in range(n_pool)]
    it = 0

    def block(n=K):
        nonlocal it
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync_all()                                   # barrier + synchronize
        t0 = time.perf_counter()
        e0.record()
        for _ in range(n):
            steppers[it % n_pool]()
            it += 1
        e1.record()
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        sync_all()                                   # barrier + synchronize on the far side too
        return dt, e0.elapsed_time(e1)

    if warmup_s > 0:
        # through block() itself: the first block of a process pays ~0.1 ms more than the later ones, whatever came before
        image = env.snapshot()
        t0 = time.perf_counter()
        while max_over_ranks([time.perf_counter() - t0])[0] < warmup_s:      # every rank runs as many blocks
            block(min(K, 100))
        env.restore(image)
        del image
    it = 0
    for _ in range(W):
        steppers[it % n_pool]()
        it += 1

    first = block()
    if outputs is not None:
        outputs.update(obs=obs.cpu().numpy(), reward=rew.cpu().numpy(),
                       absorbing=ab.cpu().numpy().astype(np.float32), last=last.cpu().numpy().astype(np.float32))
    # every rank must run the same number of blocks: decide it from the first block's max-over-ranks time
    t_first = max_over_ranks([first[0]])[0]
    n_blocks = int(min(max(3, min_time / max(t_first, 1e-9)), max_blocks)) if repeat else 1
    res = [first] + [block() for _ in range(n_blocks - 1)]
    secs = max_over_ranks([r[0] for r in res])
    kern_ms = float(np.mean([r[1] for r in res])) / K
    return secs, kern_ms


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """Write {name: array [B, ...]} as path/<name>.npy in float32 / float64 (other types become float32).  Above
    DUMP_LIMIT_BYTES in all, the same seeded sample of rows (environments) is kept from every array and the row indices
    are written as sample_rows.npy."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {n: np.ascontiguousarray(a if a.dtype in (np.float32, np.float64) else a.astype(np.float32))
              for n, a in arrays.items()}
    rows = len(next(iter(arrays.values())))
    per_row = sum(a.nbytes for a in arrays.values()) / rows
    if rows * per_row > DUMP_LIMIT_BYTES:
        keep = int(DUMP_LIMIT_BYTES // (per_row + 8))
        idx = np.sort(np.random.default_rng(0).choice(rows, keep, replace=False))
        arrays = {n: a[idx] for n, a in arrays.items()}
        arrays['sample_rows'] = idx.astype(np.float64)
    for n, a in arrays.items():
        np.save(os.path.join(path, n + '.npy'), a)


def graphed_step_us(env, actions, n=20, reps=30):
    """The same step launches replayed from ONE HIP graph (rl_on_manifold_amd.GraphedRollout: observe -> policy -> step,
    n times; here the "policy" hands out the pre-generated actions): what the launch path costs on top of the kernels."""
    import torch
    from rl_on_manifold_amd import GraphedRollout
    it = [0]

    def policy(obs):
        a = actions[it[0] % actions.shape[0]]
        it[0] += 1
        return a

    loop = GraphedRollout(env, policy, n)
    loop.replay()
    torch.cuda.synchronize(env.device)
    t0 = time.perf_counter()
    for _ in range(reps):
        loop.replay()
    torch.cuda.synchronize(env.device)
    return (time.perf_counter() - t0) / (reps * n) * 1e6


VALU_F64_PEAK_TF = 78.6        # AMD's MI355X specification (FP64 vector; MI355X_MICROARCH.md lists no fp64 figure): half the fp32 rate


def roofline_objects(name, B, kern_ms, traffic=None, chart='reference', dyn=False, f64=False):
    """(roofline, roofline_hbm): the binding roof first -- the vector ALU of the compute type -- then the HBM view of the same
    kernel.  `traffic`: the dict of measured_traffic() (or None)."""
    elem = 2 if f64 else 1
    algo_bytes = (ALGO_BYTES[name] + (48 if dyn else 0)) * B * elem   # dyn: + the six servo-joint values read and written
    flops = ((algorithmic_flops_canonical(name) if chart == 'canonical' else algorithmic_flops(name))
             + (algorithmic_flops_dyn() if dyn else 0)) * B
    gbs = algo_bytes / (kern_ms * 1e-3) / 1e9
    tf = flops / (kern_ms * 1e-3) / 1e12
    peak = VALU_F64_PEAK_TF if f64 else VALU_F32_PEAK_TF
    tb = traffic['bytes'] if traffic else None
    tsrc = traffic['source'] if traffic else None
    traw = traffic['raw_counter_bytes'] if traffic else None
    return ({'bound': 'valu_f64' if f64 else 'valu_f32', 'achieved': tf, 'peak': peak, 'unit': 'TFLOP/s',
             'frac': tf / peak, 'traffic': tb, 'traffic_source': tsrc, 'traffic_raw_counter_bytes': traw,
             'algorithmic_flops_per_launch': flops, 'kernel_ms': kern_ms,
             'note': 'the vector ALU is the binding roof (130 FLOP/B, ridge at 20); traffic = HBM bytes per launch from the '
                     'committed counter passes named in traffic_source (2 x FETCH_SIZE + WRITE_SIZE), next to '
                     'roofline_hbm.algorithmic_bytes_per_launch'},
            {'bound': 'hbm', 'achieved': gbs, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': gbs / HBM_PEAK_GBS,
             'traffic': tb, 'traffic_source': tsrc, 'algorithmic_bytes_per_launch': algo_bytes, 'kernel_ms': kern_ms,
             # > 1: bytes that travel without being asked for (the state moves in whole groups of four fields)
             'traffic_over_algorithmic': (tb / algo_bytes) if tb else None})


def committed_kernel_us(csv_name, kernel_substr):
    """Average duration (us) of a kernel from a committed rocprofv3 --stats summary under profiles/ (None if absent)."""
    import csv
    try:
        for r in csv.DictReader(open(os.path.join(ROOT, 'profiles', csv_name))):
            if kernel_substr in r['Name']:
                return float(r['AverageNs']) / 1e3
    except Exception:  # noqa: BLE001
        pass
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=100)
    ap.add_argument('--warmup-seconds', type=float, default=1.0,
                    help='before the --warmup steps, step for this long from a snapshot that is then restored: the device '
                         'reaches its steady state and the timed steps still see the same data on every run')
    ap.add_argument('--env', default='iiwa')
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--lanes', type=int, default=0, help='kernel mapping: 0 = library policy, else lanes per env')
    ap.add_argument('--chart-mode', default='reference', choices=['reference', 'canonical'],
                    help="chart of the HEADLINE engine (default: the reference's; 'canonical' is the opt-in mode, also "
                         "timed as a secondary record of a --full run)")
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help="write what the timed block's last step returned as DIR/<name>.npy (rank 0's shard)")
    ap.add_argument('--full', action='store_true',
                    help='also measure everything beyond the headline: repeated blocks, collection, rooflines, secondary '
                         'and saturation records, CPU baseline')
    ap.add_argument('--min-time', type=float, default=2.0, help='--full: keep timing K-step blocks until this many seconds')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='--full: leave out the CPU baseline')
    ap.add_argument('--no-secondary', action='store_true', help='--full: leave out the secondary and saturation records')
    ap.add_argument('--cpu-seconds', type=float, default=4.0, help='budget of each scalar CPU-baseline leg')
    args = ap.parse_args()

    env_world = os.environ.get('WORLD_SIZE')
    if env_world is None and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))
    world = int(env_world or '1')
    if world != args.gpus:
        sys.exit('bench.py: --gpus %d contradicts WORLD_SIZE=%d of the launcher' % (args.gpus, world))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    # The contract is ONE JSON line on stdout.  Libraries write there too -- RCCL 2.26 prints a five-line version banner
    # through C stdio at communicator creation, and being block-buffered on a pipe it comes out at process exit, AFTER the
    # JSON line.  So: file descriptor 1 is pointed at stderr for the whole run (Python's own prints included) and the
    # JSON line alone goes to a private duplicate of the real stdout.
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), 'w')
    os.dup2(2, 1)
    if world > 1:
        # before the HIP / HSA runtime comes up (first torch.cuda call): the host driver only supports dmabuf IPC
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')

    import numpy as np
    import torch
    import torch.distributed as dist

    # BENCH_DIST_BACKEND=gloo lets the multi-rank control flow be exercised on a box with fewer GPUs than ranks
    # (ranks then share devices); the driver's runs use the default, nccl (= RCCL), one rank per GPU.
    backend = os.environ.get('BENCH_DIST_BACKEND', 'nccl')
    n_dev = torch.cuda.device_count()
    if n_dev == 0:
        sys.exit('bench.py: no ROCm GPU visible (the engine has no CPU path)')
    if backend == 'nccl' and world > n_dev:
        sys.exit('bench.py: --gpus %d but only %d GPU(s) visible; RCCL needs one GPU per rank '
                 '(BENCH_DIST_BACKEND=gloo exercises the multi-rank control flow on fewer GPUs)' % (world, n_dev))
    dev = torch.device('cuda', local_rank % n_dev)
    torch.cuda.set_device(dev)
    if world > 1:
        kw = {'device_id': dev} if backend == 'nccl' else {}
        dist.init_process_group(backend, rank=rank, world_size=world, **kw)
    red_dev = dev if backend == 'nccl' else torch.device('cpu')

    def sync_all():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    def max_over_ranks(vals):
        if world == 1:
            return list(vals)
        t = torch.tensor(list(vals), device=red_dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.cpu().tolist()

    B, K, W = args.batch, args.steps, args.warmup
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + rank)
    env, init, rejected = make_env(args.env, B, dev, gen, args.lanes, chart_mode=args.chart_mode)
    k = env.dims['null']
    n_pool = 64
    actions = torch.rand((n_pool, B, k), device=dev, generator=gen) * 2 - 1

    # ---- headline: ONE block of exactly K steps
    outs = {} if args.dump_outputs and rank == 0 else None
    secs, kern_ms = time_steps(env, actions, K, W, args.min_time, sync_all, max_over_ranks, repeat=args.full, outputs=outs,
                               warmup_s=args.warmup_seconds)
    elapsed = secs[0]
    if outs is not None:
        dump_outputs(args.dump_outputs, outs)

    result = None
    if rank == 0:
        result = {
            'metric': 'env-steps/sec', 'value': world * B * K / elapsed, 'unit': 'env-steps/s', 'n_gpus': world,
            'steps': K, 'warmup': W, 'warmup_seconds': args.warmup_seconds, 'ms_per_step': elapsed / K * 1e3, 'higher_is_better': True, 'scaling': 'weak',
            'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'config': {'workload': WORKLOAD[args.env] + ', batch %d per GPU' % B,
                       'batch_per_gpu': B, 'global_batch': B * world,
                       'lanes_per_env_requested': int(env.cfg.lanes_per_env), 'lanes_per_env': env.lanes_per_env, 'rollout_lanes_per_env': env.rollout_lanes_per_env, 'substeps': int(env.cfg.substeps),
                       'horizon': int(env.cfg.horizon), 'path': 'atacom_step (1 launch / step) via C ABI',
                       'chart_mode': args.chart_mode,
                       'init': 'q_init + N(0, 0.05^2), one correction step, rejected unless all g < 0 and |f| < 1e-3 '
                               '(%.1f %% of draws rejected); puck uniform in the hit range' % (100 * rejected)
                               if args.env != 'circle' else 'half fixed reset point, half random valid states',
                       'parallelism': 'env-shard x%d, no data-path collective' % world},
        }
    if args.full:
        c_avg, c_max, c_dq_max = env.get_constraints_logs()
        if world > 1:
            c_max, c_dq_max = max_over_ranks([c_max, c_dq_max])
        collection, pol_rate = collection_records(env, args.env, world, backend, dev, gen, sync_all, max_over_ranks)
        if rank == 0:
            traffic = (measured_traffic(args.env, args.chart_mode, lanes=env.lanes_per_env)
                       if B == {'circle': 4096}.get(args.env, 8192) else None)
            roof, roof_hbm = roofline_objects(args.env, B, kern_ms, traffic, args.chart_mode)
            med = float(np.median(secs))
            result.update({
                # spread of the K-step blocks next to the headline block (one block in ~3000 took 70 x the
                # median -- a host hiccup, visible here instead of hidden by the median)
                'block_ms_p99': float(np.percentile(secs, 99)) * 1e3, 'block_ms_max': max(secs) * 1e3,
                'timing': {'blocks': len(secs), 'block_steps': K, 'block_ms_median': med * 1e3,
                           'block_ms_min': min(secs) * 1e3, 'block_ms_p99': float(np.percentile(secs, 99)) * 1e3,
                           'block_ms_max': max(secs) * 1e3, 'ms_per_step_median': med / K * 1e3,
                           'timed_seconds_total': float(sum(secs)),
                           'statistic': 'blocks of (max over ranks); the headline is the first block'},
                'max_abs_c': c_max, 'c_avg': c_avg, 'c_dq_max': c_dq_max,
                'collection': collection,
                'policy_rollout_kernel_env_steps_per_s_per_gpu': pol_rate,
                'roofline': roof, 'roofline_hbm': roof_hbm,
            })
        # the engine of the headline run is no longer needed; secondary workloads and the CPU legs are N = 1 extras
        if world == 1 and rank == 0:
            if not args.no_secondary and args.env == 'iiwa' and args.batch == 8192:
                result['secondary'] = secondary_records(dev, gen, K, W, sync_all, max_over_ranks)
                result['saturation'] = saturation_records(dev, gen, K, W, sync_all, max_over_ranks)
            if not args.no_cpu_baseline:
                result['cpu_baseline'] = cpu_baseline(args.env, args.cpu_seconds, dev, init, k)
    if rank == 0:
        json_out.write(json.dumps(result) + '\n')
        json_out.flush()
    json_out.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return result


def collection_records(env, name, world, backend, dev, gen, sync_all, max_over_ranks):
    """Config 5's collection phase on the headline engine: a 120-step rollout (one launch, packed records) + the one
    all-gather, then the same collection with the actor MLP in the kernel.  Returns (collection dict, policy env-steps/s)."""
    import numpy as np
    import torch
    from rl_on_manifold_amd import MlpPolicy
    from rl_on_manifold_amd.rollout import RolloutCollector
    B, k, D = env.batch, env.dims['null'], env.obs_dim
    # ---- collection phase of config 5: 120-step rollout (one launch, packed records) + the one all-gather
    T = 120
    col = RolloutCollector(env)
    racts = torch.rand((T, B, k), device=dev, generator=gen) * 2 - 1
    rec = env.rollout_packed(actions=racts)
    gathered = col.gather(rec)
    sync_all()
    n_rep = 5
    t_roll, t_gath = [], []
    for _ in range(n_rep):
        sync_all()
        t0 = time.perf_counter()
        env.rollout_packed(actions=racts, out=rec)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        gathered = col.gather(rec)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        t_roll.append(t1 - t0)
        t_gath.append(t2 - t1)
    # the same two collections with the first all-gather left in flight while the second rollout runs (collect_async)
    t_pipe = None
    if world > 1:
        rec2 = torch.empty_like(rec)
        out_a = torch.empty((world,) + tuple(rec.shape), device=dev, dtype=rec.dtype)
        t_pipe = []
        for _ in range(3):
            sync_all()
            t0 = time.perf_counter()
            env.rollout_packed(actions=racts, out=rec)
            _, work = col.gather(rec, out=out_a, async_op=True)
            env.rollout_packed(actions=racts, out=rec2)
            work.wait()
            g2 = col.gather(rec2)
            torch.cuda.synchronize(dev)
            t_pipe.append(time.perf_counter() - t0)
        t_pipe = float(np.median(max_over_ranks(t_pipe)))
        del rec2, out_a, g2
    t_roll = float(np.median(max_over_ranks(t_roll)))
    t_gath = float(np.median(max_over_ranks(t_gath)))
    sent = rec.numel() * rec.element_size()
    recv = gathered.numel() * gathered.element_size()
    collection = {'steps': T, 'records': list(gathered.shape), 'rollout_ms': t_roll * 1e3,
                  'rollout_env_steps_per_s_per_gpu': B * T / t_roll,
                  'allgather_ms': t_gath * 1e3 if world > 1 else None,
                  'bytes_sent_per_rank': sent, 'bytes_received_per_rank': recv if world > 1 else 0,
                  'allgather_GBps_per_rank': (recv - sent) / t_gath / 1e9 if world > 1 else None,
                  'collection_env_steps_per_s': world * B * T / (t_roll + (t_gath if world > 1 else 0.0)),
                  'two_collections_overlapped_ms': t_pipe * 1e3 if t_pipe else None,
                  'backend': backend if world > 1 else None}
    del gathered
    if world == 1 and backend == 'nccl':
        collection['rccl_world1_selfgather'] = rccl_selfgather(env, rec, dev)

    # ---- the same collection with the actor MLP (18-64-64-5, random weights) + Gaussian noise inside the kernel (row N2)
    pol_rate = None
    if name != 'circle':
        gw = torch.Generator(device='cpu'); gw.manual_seed(0)
        Wts = [torch.randn(64, D, generator=gw) * 0.2, torch.zeros(64), torch.randn(64, 64, generator=gw) * 0.1,
               torch.zeros(64), torch.randn(k, 64, generator=gw) * 0.1, torch.zeros(k)]
        pol = MlpPolicy(*Wts, std=torch.full((k,), 0.5))
        eps = torch.randn((T, B, k), device=dev, generator=gen)
        env.rollout_packed(policy=pol, n_steps=T, noise=eps, out=rec)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        for _ in range(n_rep):
            env.rollout_packed(policy=pol, n_steps=T, noise=eps, out=rec)
        torch.cuda.synchronize(dev)
        pol_rate = n_rep * T * B / (time.perf_counter() - t2)
    env.get_constraints_logs()

    return collection, pol_rate


def measured_traffic(name, chart='reference', dyn=False, lanes=0, tag=None):
    """HBM bytes per launch of the step kernel at the BASELINE batch, from the committed counter passes (rocprofv3 --pmc
    FETCH_SIZE and --pmc WRITE_SIZE in separate runs of profiles/tools/gpu_pmc_target.py, summarised into profiles/traffic_*.json) --
    NOT measured inside this run: bench.py cannot host the profiler, the line says where the figure comes from
    (`traffic_source`).  Corrected as MI355X_MICROARCH.md prescribes for gfx950: FETCH_SIZE counts a 16 B / lane streaming
    read at half its bytes (128-byte requests tallied at 64), so the fetch side is doubled; WRITE_SIZE is taken as counted.
    Returns {'bytes', 'raw_counter_bytes', 'fetch_kb', 'write_kb', 'source'} or None."""
    # tag: another workload of the same task with a counter pass of its own ('f64': the float64 headline, '65536': the saturation batch)
    suffix = ('_' + tag) if tag else ('_dyn' if dyn else ('_canonical' if chart == 'canonical' else ('_quad' if name == 'iiwa' and lanes == 4 else '')))
    rel = os.path.join('profiles', 'traffic_%s%s.json' % (name, suffix))
    try:
        d = json.load(open(os.path.join(ROOT, rel)))
        fetch_kb, write_kb = float(d['FETCH_SIZE_KB']), float(d['WRITE_SIZE_KB'])
    except Exception:  # noqa: BLE001
        return None
    return {'bytes': (2.0 * fetch_kb + write_kb) * 1024.0, 'raw_counter_bytes': (fetch_kb + write_kb) * 1024.0,
            'fetch_kb': fetch_kb, 'write_kb': write_kb,
            'source': rel + ' (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of an earlier run on this workload, NOT measured in '
                      'this run); FETCH_SIZE x 2 (gfx950 correction of MI355X_MICROARCH.md, HBM section) + WRITE_SIZE'}


def rccl_selfgather(env, rec, dev, reps=5):
    """N = 1 only: the packed record buffer of the collection above through the real RCCL all_gather_into_tensor -- a
    process group of ONE rank, the collector told not to short-circuit.  No xGMI hop, so this is a LOWER bound on what
    the collective adds to a collection (launch, buffer registration, the device-side copy); the N > 1 lines carry the
    measured all-gather.  Never fatal: a box whose RCCL cannot initialise reports the error string instead."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from rl_on_manifold_amd.rollout import RolloutCollector
    if dist.is_initialized():
        return None
    try:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', str(_free_port()))
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
        try:
            col = RolloutCollector(env, force_collective=True)
            g = col.gather(rec)
            torch.cuda.synchronize(dev)
            same = bool(torch.equal(g[0], rec))
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                col.gather(rec)
                torch.cuda.synchronize(dev)
                ts.append(time.perf_counter() - t0)
            nbytes = rec.numel() * rec.element_size()
            ms = float(np.median(ts)) * 1e3
            return {'ms': ms, 'bytes': nbytes, 'GBps': nbytes / ms / 1e6, 'identical': same, 'backend': 'nccl (RCCL)',
                    'note': 'world of one rank, force_collective: lower bound on the collective (no xGMI hop)'}
        finally:
            dist.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        return {'error': '%s: %s' % (type(e).__name__, str(e)[:300])}


def tstep_record(name, B, T, dev, gen, dtype=None, reps=4, init=True):
    """The T-step kernel (atacom_rollout: state in registers, one launch for T steps of B environments) timed with HIP events
    on the launch stream, with BOTH rooflines.  HBM view: the bytes the launch must move -- actions in, (obs, next_obs,
    reward, absorbing, last) out, per (step, environment); the state itself moves once per launch (counted).  Returns a
    record dict.  `init`: the initial states of the bench protocol (make_env) instead of the default reset state."""
    import torch
    from rl_on_manifold_amd import BatchedAtacomEnv
    dtype = dtype or torch.float32
    if init:
        env, _, _ = make_env(name, B, dev, gen, dtype=dtype)
    else:
        env = BatchedAtacomEnv(name, B, device=dev, dtype=dtype, auto_reset=True)
    k = env.dims['null']
    acts = (torch.rand((T, B, k), device=dev, generator=gen) * 2 - 1).to(dtype)
    out = env.rollout(acts)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        env.rollout(acts, out=out)
    e1.record()
    torch.cuda.synchronize(dev)
    ms = e0.elapsed_time(e1) / reps
    c_avg, c_max, c_dq = env.get_constraints_logs()
    esz = acts.element_size()
    io_bytes = acts.numel() * esz + sum(v.numel() * v.element_size() for v in out.values() if torch.is_tensor(v))
    state_bytes = 2 * B * esz * {'circle': 5, 'planar': 21, 'iiwa': 34}[name]         # hot state read + written once per launch
    nbytes = io_bytes + state_bytes
    flops = algorithmic_flops(name) * B * T
    f64 = dtype == torch.float64
    peak = VALU_F64_PEAK_TF if f64 else VALU_F32_PEAK_TF
    tf, gbs = flops / (ms * 1e-3) / 1e12, nbytes / (ms * 1e-3) / 1e9
    valu = {'bound': 'valu_f64' if f64 else 'valu_f32', 'achieved': tf, 'peak': peak, 'unit': 'TFLOP/s', 'frac': tf / peak,
            'algorithmic_flops_per_launch': flops}
    hbm = {'bound': 'hbm', 'achieved': gbs, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': gbs / HBM_PEAK_GBS,
           'algorithmic_bytes_per_launch': nbytes, 'bytes_per_env_step': nbytes / (B * T)}
    binding = hbm if hbm['frac'] > valu['frac'] else valu
    rec = {'workload': '%s, batch %d, T-step kernel (atacom_rollout, %d steps per launch)' % (WORKLOAD[name], B, T),
           'path': 'atacom_rollout (1 launch / %d steps) via C ABI' % T, 'value': B * T / (ms * 1e-3), 'unit': 'env-steps/s',
           'us_per_step': ms / T * 1e3, 'launch_ms': ms, 'launches_timed': reps, 'lanes_per_env': env.rollout_lanes_per_env,
           'max_abs_c': c_max, 'c_avg': c_avg, 'c_dq_max': c_dq, 'roofline': dict(binding, kernel_ms=ms),
           'roofline_other': dict(valu if binding is hbm else hbm, kernel_ms=ms)}
    env.close()
    del out, acts
    return rec


def saturation_records(dev, gen, K, W, sync_all, max_over_ranks):
    """the headline batch (8192 environments) is ONE wavefront per SIMD -- its roofline fraction is the
    occupancy of the configuration, not the quality of the kernels.  These records put the same kernels at batches that fill
    the machine into the driver-run line: config 5's global batch (65536 iiwa environments) on ONE GPU through atacom_step and
    through the T-step kernel, and the planar / circle T-step kernels at their saturation batches (circle is the one
    HBM-bound configuration: its binding roof is `hbm`)."""
    import numpy as np
    import torch
    out = []
    B = 65536
    env, _, rej = make_env('iiwa', B, dev, gen)
    acts = torch.rand((16, B, 5), device=dev, generator=gen) * 2 - 1
    secs, kern_ms = time_steps(env, acts, K, min(W, 5), 0.4, sync_all, max_over_ranks)
    el = float(np.median(secs))
    c_avg, c_max, c_dq = env.get_constraints_logs()
    roof, roof_hbm = roofline_objects('iiwa', B, kern_ms, measured_traffic('iiwa', tag='65536'))
    out.append({'workload': 'IiwaAirHockey env 7H, batch 65536 on ONE GPU (config 5\'s global batch), single steps',
                'path': 'atacom_step (1 launch / step) via C ABI', 'value': B * K / el, 'unit': 'env-steps/s',
                'ms_per_step': el / K * 1e3, 'blocks': len(secs), 'lanes_per_env': env.lanes_per_env,
                'max_abs_c': c_max, 'c_avg': c_avg, 'c_dq_max': c_dq, 'roofline': roof, 'roofline_hbm': roof_hbm})
    env.close()
    del acts
    out.append(tstep_record('iiwa', 65536, 40, dev, gen))
    out.append(tstep_record('planar', 262144, 40, dev, gen))
    out.append(tstep_record('circle', 1048576, 60, dev, gen))
    return out


def secondary_records(dev, gen, K, W, sync_all, max_over_ranks):
    """BASELINE configs 2 and 3 (circle A batch 4096, planar H batch 8192): same timing protocol, shorter."""
    import numpy as np
    import torch
    out = []
    for name, B in (('circle', 4096), ('planar', 8192)):
        env, _, _ = make_env(name, B, dev, gen)
        k = env.dims['null']
        acts = torch.rand((64, B, k), device=dev, generator=gen) * 2 - 1
        secs, kern_ms = time_steps(env, acts, K, W, 0.7, sync_all, max_over_ranks)
        el = float(np.median(secs))
        c_avg, c_max, c_dq = env.get_constraints_logs()
        racts = torch.rand((120, B, k), device=dev, generator=gen) * 2 - 1
        rec = env.rollout_packed(actions=racts)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(5):
            env.rollout_packed(actions=racts, out=rec)
        torch.cuda.synchronize(dev)
        roll = 5 * 120 * B / (time.perf_counter() - t0)
        g_us = graphed_step_us(env, acts)
        roof, roof_hbm = roofline_objects(name, B, kern_ms, measured_traffic(name))
        rec = {'workload': WORKLOAD[name] + ', batch %d' % B, 'value': B * K / el, 'unit': 'env-steps/s',
               'ms_per_step': el / K * 1e3, 'blocks': len(secs), 'max_abs_c': c_max, 'c_avg': c_avg,
               'c_dq_max': c_dq, 'rollout_kernel_env_steps_per_s': roll,
               'hip_graph_20_steps_us_per_step': g_us, 'roofline': roof,
               'roofline_hbm': roof_hbm}
        rec['path'] = 'atacom_step (1 launch / step) via C ABI; rollout_kernel_env_steps_per_s: atacom_rollout_packed, 120 steps / launch'
        if name == 'circle':
            # the T-step kernel is the real path for this task (a single circle step is launch-bound): the same batch through
            # atacom_rollout, HIP-event timed, with its own rooflines
            rec['tstep'] = tstep_record('circle', B, 500, dev, gen)
            # this configuration is bound by the host's launch path, not by the kernel: the fraction above divides by the time
            # between launches; beside it the kernel-only view, from the committed rocprofv3 kernel statistics of this workload
            k_us = committed_kernel_us('r06_rocprofv3_kernel_stats_circle.csv', 'k_step<float, atacom::Circle') or \
                committed_kernel_us('r05_rocprofv3_kernel_stats_circle.csv', 'k_step<float, atacom::Circle')
            rec['launch_bound'] = True
            if k_us:
                rk, _ = roofline_objects(name, B, k_us * 1e-3, measured_traffic(name))
                rec['roofline_kernel_only'] = {'kernel_us_rocprofv3': k_us, 'frac': rk['frac'], 'achieved': rk['achieved'],
                                               'unit': rk['unit'], 'source': 'profiles/r0x_rocprofv3_kernel_stats_circle.csv'}
        out.append(rec)
        env.close()
    # the headline workload in the REFERENCE'S OWN PRECISION (all reference arithmetic is float64 numpy): the same
    # kernels instantiated in double -- the build the parity tests hold to 1e-8 against the oracle on every sample -- timed
    # with the same protocol, priced against the fp64 vector peak (VERDICT r4 missing 3: no float64 timing existed)
    env, _, _ = make_env('iiwa', 8192, dev, gen, dtype=torch.float64)
    acts = torch.rand((64, 8192, 5), device=dev, generator=gen, dtype=torch.float64) * 2 - 1
    secs, kern_ms = time_steps(env, acts, K, W, 0.7, sync_all, max_over_ranks)
    el = float(np.median(secs))
    c_avg, c_max, c_dq = env.get_constraints_logs()
    roof, roof_hbm = roofline_objects('iiwa', 8192, kern_ms, measured_traffic('iiwa', tag='f64'), f64=True)
    out.append({'workload': 'IiwaAirHockey env 7H, batch 8192, float64 (the reference\'s precision)', 'dtype': 'f64',
                'value': 8192 * K / el, 'unit': 'env-steps/s', 'ms_per_step': el / K * 1e3, 'blocks': len(secs),
                'max_abs_c': c_max, 'c_avg': c_avg, 'c_dq_max': c_dq, 'lanes_per_env': env.lanes_per_env,
                'rollout_lanes_per_env': env.rollout_lanes_per_env, 'roofline': roof, 'roofline_hbm': roof_hbm})
    env.close()
    # the iiwa headline workload through the allocating Python surface (step(): clones + bool conversion per call), and
    # in the opt-in rigid-body mode (row N4)
    import rl_on_manifold_amd as pkg
    for label, kw in (('python step() surface', {}),
                      ('canonical chart (chart_mode = 1, opt-in)', {'chart_mode': 'canonical'}),
                      ('rigid-body mode (dynamics_mode = 1)', {'dynamics_mode': 'rigid_body'}),
                      ('rigid-body mode with servo feed-forward (dynamics_mode = 2)', {'dynamics_mode': 'rigid_body_ff'})):
        B = 8192
        env = pkg.BatchedAtacomEnv('iiwa', B, device=dev, dtype=torch.float32, auto_reset=True, **kw)
        init, _ = feasible_init('iiwa', B, dev, gen)
        env.reset(state=init)
        acts = torch.rand((64, B, 5), device=dev, generator=gen) * 2 - 1
        kern_ms = None
        if kw:
            secs, kern_ms = time_steps(env, acts, K, W, 0.7, sync_all, max_over_ranks)
            el = float(np.median(secs))
        else:
            for i in range(W):
                env.step(acts[i % 64])
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            n = max(K, 200)
            for i in range(n):
                env.step(acts[i % 64])
            torch.cuda.synchronize(dev)
            el = (time.perf_counter() - t0) * K / n
        c_avg, c_max, c_dq = env.get_constraints_logs()
        rec = {'workload': 'IiwaAirHockey env 7H, batch 8192, ' + label, 'value': B * K / el, 'unit': 'env-steps/s',
               'ms_per_step': el / K * 1e3, 'max_abs_c': c_max, 'c_avg': c_avg, 'c_dq_max': c_dq,
               'lanes_per_env': env.lanes_per_env, 'rollout_lanes_per_env': env.rollout_lanes_per_env}
        if 'chart_mode' in kw:
            racts = torch.rand((120, B, 5), device=dev, generator=gen) * 2 - 1
            r_ = env.rollout_packed(actions=racts)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(5):
                env.rollout_packed(actions=racts, out=r_)
            torch.cuda.synchronize(dev)
            rec['rollout_kernel_env_steps_per_s'] = 5 * 120 * B / (time.perf_counter() - t0)
            rec['roofline'], rec['roofline_hbm'] = roofline_objects('iiwa', B, kern_ms, measured_traffic('iiwa', 'canonical'),
                                                                    'canonical')
        if 'dynamics_mode' in kw:
            rec['roofline'], rec['roofline_hbm'] = roofline_objects('iiwa', B, kern_ms, measured_traffic('iiwa', dyn=True),
                                                                    dyn=True)
        out.append(rec)
        env.close()
    return out


def usable_cores():
    """Cores this process may actually use: the affinity mask, capped by the cgroup CPU quota (a container that
    sees 256 CPUs but is throttled to 16 cores' worth of time gains nothing from 256 workers)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    for path in ('/sys/fs/cgroup/cpu.max', '/sys/fs/cgroup/cpu/cpu.cfs_quota_us'):
        try:
            txt = open(path).read().split()
            if path.endswith('cpu.max'):
                if txt[0] != 'max':
                    n = min(n, max(1, int(float(txt[0]) / float(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                per = int(open('/sys/fs/cgroup/cpu/cpu.cfs_period_us').read())
                if q > 0:
                    n = min(n, max(1, int(q / per + 0.5)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def cpu_baseline(env_name, budget_s, dev, init, k):
    """The oracle as the CPU baseline ("port"; the reference itself needs Pinocchio / PyBullet / MushroomRL and never
    travels to this box).  Three legs on the host cores of the GPU box:
      R1  scalar, reference algorithmic shape (one LAPACK SVD + one RREF per environment per sub-step), 1 core;
      R1' the same on all cores (independent processes, core count stated);
      R2  batched numpy restatement, 1 process -- run on 256 of the bench's own initial states with a fixed action
          sequence, which also yields the oracle's constraint statistics next to the device's on identical input."""
    import multiprocessing as mp
    import numpy as np
    import torch
    from oracle import cpu_legs
    from rl_on_manifold_amd import BatchedAtacomEnv
    cores = usable_cores()
    one = cpu_legs.scalar_leg((env_name, budget_s, 0))
    ctx = mp.get_context('spawn')
    t0 = time.perf_counter()
    with ctx.Pool(cores) as pool:
        parts = pool.map(cpu_legs.scalar_leg, [(env_name, budget_s, i + 1) for i in range(cores)])
    wall_all = time.perf_counter() - t0
    all_rate = sum(p['steps'] / p['seconds'] for p in parts)
    # ---- R2 + constraint check on identical states / actions
    n_sub, T = 256, 120
    rng = np.random.default_rng(5)
    acts = rng.uniform(-1, 1, (T, n_sub, k))
    sub_init = None if init is None else init[:n_sub].double().cpu().numpy()
    t0 = time.perf_counter()
    ora = cpu_legs.batched_leg(env_name, sub_init, acts)
    dt_b = time.perf_counter() - t0
    denv = BatchedAtacomEnv(env_name, n_sub, device=dev, dtype=torch.float32, auto_reset=True)
    if init is not None:
        denv.reset(state=init[:n_sub])
    denv.rollout(torch.as_tensor(acts, dtype=torch.float32, device=dev))
    d_avg, d_max, d_dq = denv.get_constraints_logs()
    denv.close()
    return {'value': all_rate, 'unit': 'env-steps/s', 'cores': cores, 'kind': 'port',
            'sample': 'float64 numpy/scipy oracle in the reference\'s algorithmic shape (SVD + RREF per env per sub-step), '
                      '%d independent processes x %.0f s of sequential %s env-steps (%.1f s wall incl. process start)'
                      % (cores, budget_s, env_name, wall_all),
            'legs': {'scalar_1_core': {'value': one['steps'] / one['seconds'], 'cores': 1, 'steps': one['steps']},
                     'scalar_all_cores': {'value': all_rate, 'cores': cores, 'steps': int(sum(p['steps'] for p in parts))},
                     'batched_numpy': {'value': n_sub * T / dt_b, 'cores': 1, 'steps': n_sub * T,
                                       'blas_threads': os.environ.get('OMP_NUM_THREADS', 'default')}},
            'constraint_check': {'envs': n_sub, 'steps': T, 'note': 'same initial states and actions, free-running',
                                 'oracle_f64': {'c_avg': ora['c_avg'], 'c_max': ora['c_max'], 'c_dq_max': ora['c_dq_max']},
                                 'device_f32': {'c_avg': d_avg, 'c_max': d_max, 'c_dq_max': d_dq},
                                 'c_max_ratio_device_over_oracle': d_max / ora['c_max'] if ora['c_max'] else None},
            'host_cpus_visible': os.cpu_count(), 'host_cpus_usable': cores}


if __name__ == '__main__':
    main()
