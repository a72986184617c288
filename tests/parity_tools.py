"""How the float32 parity tests decide that an error is *explained* -- with no sample allowed to stay unexplained.

The reference algorithm is discontinuous (rref's 0.05 pivot tolerance, atacom.py:128; contact / rim / latch decisions of
the puck model) and, away from its discontinuities, has a large and strongly state-dependent Lipschitz constant (the
slack dynamics ~ 1/s; four chained sub-steps; a LAPACK null basis that is ill-determined -- amplification up to 1e5 --
whenever joints sit near zero).  A float32 evaluation is a float64 evaluation of slightly perturbed data (backward
stability), so the honest bound on |HIP_f32 - oracle_f64| is the oracle's own response to float32-sized perturbations
of its inputs AND of the matrix J_c it factorises (all entries, structural zeros included):

    sens(x) = max over perturbations d, |d_i| <= eps_rel * |x_i|, of | oracle(x + d) - oracle(x) |

estimated by sampling (a handful of random sign patterns at three magnitudes, 2e-7 ... 4e-6 relative: 2 to 30 float32
ulps).  A sample PASSES if  err <= C * sens + floor.  A sample that does not pass the cheap estimate is re-examined
with many more draws at up to 1.6e-5 relative (a discontinuity just outside the first ball: the tolerance branch one of
the kernel's ~10^4 rounded operations can reach); if the float64 oracle itself then moves by >= err / C it passes,
otherwise the test FAILS.  Nothing is waved through by a percentage: a kernel bug (wrong lane, wrong row, stale
register) produces errors where the oracle is insensitive and is caught on the first sample.

SELF-AUDIT.  Where the oracle itself is that sensitive that C sens + floor exceeds REPRO_ERR, REPRO_GAIN, MAX_UNREPRODUCED = 1e-3, 5.0, 2e-3
VACUOUS = 1e-2 the
bound says nothing about the sample.  `finish` / `assert_matrix_fn_explained` count those samples, print the share and
FAIL when it exceeds a per-test ceiling (default 40 %; the step tests pass what their task was calibrated to --
reference chart: iiwa 35 % (its perturbed reset poses sit inside the rref tolerance regime: the reference itself moves
by > 1e-2 under float32-sized perturbations on a third of them), planar 0.5 %, circle 0; canonical chart: see
tests/test_gpu_chart.py): the rule cannot silently turn vacuous -- a kernel bug confined to ill-conditioned
samples would need that band to grow, or is caught by the float64 build of the SAME kernels, which every step test
runs on the same samples at 1e-8 (no sensitivity allowance there).

And LARGE errors are capped whatever the bound says: a sample whose error exceeds REPRO_ERR = 1e-3 is re-run through the
float64 oracle under float32-sized perturbations of its inputs; unless one of those evaluations lands REPRO_GAIN = 5 x
closer to the device's result than the unperturbed oracle is (the device took the other side of a discontinuity the
perturbations reach) it counts as "not reproduced", and at most MAX_UNREPRODUCED = 0.2 % of a test's samples may be.
Calibration (round 3, 40960 teacher-forced iiwa steps per mapping): 31-37 errors above 1e-3, nearly all of them from
the CONTINUOUS hypersensitivity of the reference's null basis (random perturbations move the oracle as far, but not to the
same point), i.e. 0.09 % -- a kernel defect confined to the ill-conditioned samples would have to hide inside that.

C = 4 and floor = 5e-6 * max(1, |value|) are calibrated on 1.6e5 teacher-forced env steps per environment and kernel
mapping (profiles/r02_parity_sensitivity.md): the largest err / sens seen was 1.7, the 99.9th percentile 0.09, the
median below 0.01 -- the bound is a worst-case (condition-number) bound, the bulk of the errors sits at 1e-6.
"""
import copy

import numpy as np

QUICK_SCALES = (2e-7, 1e-6, 4e-6)
DEEP_SCALES = (1e-6, 4e-6, 1.6e-5)
C_SENS = 4.0
REPRO_ERR, REPRO_GAIN, MAX_UNREPRODUCED = 1e-3, 5.0, 2e-3
VACUOUS = 1e-2               # a bound above this says nothing: such samples are counted and capped (module docstring)
JC_NOISE_FRACTION = 0.25     # J_c entries are perturbed at a quarter of the input scales: 5e-8 ... 1e-6 (1 to 16 float32 ulps)
FLOOR = 5e-6


def slice_env(o, idx):
    """A deep copy of a batched oracle env restricted to the environments `idx`."""
    p = copy.copy(o)
    idx = np.asarray(idx)
    for k, v in o.__dict__.items():
        if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == o.B:
            setattr(p, k, v[idx].copy())
        else:
            setattr(p, k, copy.deepcopy(v))
    p.B = len(idx)
    return p


def perturbed(o, scale, rng, fields=('q', 'dq', 's', 'puck'), jc_noise=True):
    p = slice_env(o, np.arange(o.B))
    for k in ('decision_margin', 'contact_margin', 'cond_number', 'chart_skipped', 'chart_info', 'chart_default'):
        p.__dict__.pop(k, None)
    for f in fields:
        arr = getattr(p, f)
        arr *= 1.0 + scale * rng.choice([-1.0, 1.0], arr.shape)
    # and an unstructured perturbation of J_c itself (structural zeros included) at the same relative size: rounding inside
    # a float32 factorisation is exactly that, and the reference's LAPACK null basis responds to it with an amplification
    # of up to ~1e5 when joints sit near zero (nearly decoupled joint-limit rows: a near-breakdown of the Golub-Kahan
    # recurrence) -- see DESIGN.md section 2 and profiles/r02_parity_sensitivity.md
    if jc_noise:
        p.jc_noise = (scale * JC_NOISE_FRACTION, rng)
    return p


class SensitivityRecorder:
    """Collects, step by step, the device error and the oracle's sensitivity; `finish()` asserts that every sample is
    explained (module docstring).

    step_fn(env_copy, inputs) -> [B, n_out] float64 array of everything that is compared (it may advance env_copy).
    `inputs` is a tuple of float arrays that are perturbed together with the state (actions, noise).

    quick_scales / deep_scales / floor (defaults: the module's constants, the float32 rule) restate the rule for another
    precision: the float64 build on ill-conditioned states is held to  err <= floor + C sens  with the probes scaled down
    to float64-sized perturbations and jc_noise = False (no unstructured noise on J_c: `finish_float64`).
    stacked_draws = True evaluates the draws of one scale as ONE oracle batch (every environment repeated `draws` times)
    instead of one after the other: the same probes, drawn in another order, at a fraction of the cost where the oracle's
    time is per call and not per environment (the deep probe of a few samples: 48 draws per scale).
    repro_scales / repro_draws / repro_structured widen the DRAWS of the reproduction audit of errors above REPRO_ERR (its
    REPRO_* constants stand): other scales than the deep ones, more draws per scale, and every scale also without the
    unstructured J_c noise (J_c's structural zeros kept exact, as a device keeps them) -- tests/arm_limit_cases.py."""

    def __init__(self, step_fn, seed=0, state_fields=('q', 'dq', 's', 'puck'), quick_scales=QUICK_SCALES,
                 deep_scales=DEEP_SCALES, floor=FLOOR, jc_noise=True, stacked_draws=False, repro_scales=None, repro_draws=16,
                 repro_structured=False):
        self.step_fn = step_fn
        self.repro_scales, self.repro_draws, self.repro_structured = repro_scales, repro_draws, repro_structured
        self.quick_scales, self.deep_scales, self.floor, self.jc_noise = quick_scales, deep_scales, floor, jc_noise
        self.stacked = stacked_draws
        self.rng = np.random.default_rng(seed)
        self.fields = state_fields
        self.snaps, self.inputs, self.base, self.err, self.sens, self.where, self.dev = [], [], [], [], [], [], []

    def _stacked(self, o, inputs, draws):
        rep = np.repeat(np.arange(o.B), draws)
        return slice_env(o, rep), tuple(x[rep] for x in inputs), rep

    def _sens(self, o, inputs, base, scales, draws):
        s = np.zeros(o.B)
        if self.stacked:
            big, bin_, rep = self._stacked(o, inputs, draws)
            bb = base[rep]
            for sc in scales:
                p = perturbed(big, sc, self.rng, self.fields, self.jc_noise)
                pin = tuple(x * (1.0 + sc * self.rng.choice([-1.0, 1.0], x.shape)) for x in bin_)
                out = self.step_fn(p, pin)
                r = (np.abs(out - bb) / np.maximum(1.0, np.abs(bb))).max(1)
                s = np.maximum(s, r.reshape(o.B, draws).max(1))
            return s
        for sc in scales:
            for _ in range(draws):
                p = perturbed(o, sc, self.rng, self.fields, self.jc_noise)
                pin = tuple(x * (1.0 + sc * self.rng.choice([-1.0, 1.0], x.shape)) for x in inputs)
                out = self.step_fn(p, pin)
                s = np.maximum(s, (np.abs(out - base) / np.maximum(1.0, np.abs(base))).max(1))
        return s

    def prepare(self, o, inputs, base=None):
        """Oracle side of one sample (independent of the device, so a test parametrised over kernel mappings prepares
        once and compares many times).  Call BEFORE the oracle env `o` is stepped; returns the oracle outputs (`base`: those
        outputs where another recorder of the same step_fn has already computed them)."""
        snap = slice_env(o, np.arange(o.B))
        for k in ('decision_margin', 'contact_margin', 'cond_number', 'chart_skipped', 'chart_info', 'chart_default'):
            snap.__dict__.pop(k, None)
        if base is None:
            base = self.step_fn(slice_env(snap, np.arange(o.B)), inputs)
        self.snaps.append(snap); self.inputs.append(inputs); self.base.append(base)
        self.sens.append(self._sens(snap, inputs, base, self.quick_scales, 2))
        return base

    def compare(self, t, dev_out):
        base = self.base[t]
        rel = np.abs(np.asarray(dev_out, dtype=np.float64) - base) / np.maximum(1.0, np.abs(base))
        e = rel.max(1)
        while len(self.err) <= t:
            self.err.append(None)
            self.where.append(None)
            self.dev.append(None)
        self.err[t], self.where[t] = e, rel.argmax(1)
        self.dev[t] = np.asarray(dev_out, dtype=np.float64)
        return e

    def record(self, o, inputs, dev_out):
        """prepare + compare for tests that run once."""
        base = self.prepare(o, inputs)
        self.compare(len(self.base) - 1, dev_out)
        return base

    def fresh(self):
        """A recorder sharing the prepared oracle data, with an empty error log (one per device configuration)."""
        r = copy.copy(self)
        r.err, r.where, r.dev = [], [], []
        r.sens = [x.copy() for x in self.sens]
        return r

    def head(self, n):
        """fresh() restricted to the first n environments (a ragged device batch out of the same prepared samples)."""
        r = copy.copy(self)
        idx = np.arange(n)
        r.snaps = [slice_env(s, idx) for s in self.snaps]
        r.inputs = [tuple(x[:n] for x in i) for i in self.inputs]
        r.base = [b[:n] for b in self.base]
        r.sens = [s[:n].copy() for s in self.sens]
        r.err, r.where, r.dev = [], [], []
        return r

    def _unreproduced(self, E):
        """samples with E > REPRO_ERR that no perturbed oracle evaluation brings REPRO_GAIN x closer to the device"""
        big = np.argwhere(E > REPRO_ERR)
        out = []
        for t in np.unique(big[:, 0]) if len(big) else []:
            idx = big[big[:, 0] == t, 1]
            sub = slice_env(self.snaps[t], idx)
            sin = tuple(x[idx] for x in self.inputs[t])
            dev = self.dev[t][idx]
            scale = np.maximum(1.0, np.abs(dev))
            best = np.full(len(idx), np.inf)
            n = self.repro_draws
            kinds = (self.jc_noise, False) if self.repro_structured and self.jc_noise else (self.jc_noise,)
            if self.stacked:
                stk, bin_, rep = self._stacked(sub, sin, n)
            for sc in self.deep_scales if self.repro_scales is None else self.repro_scales:
                for jc in kinds:
                    if self.stacked:
                        p = perturbed(stk, sc, self.rng, self.fields, jc)
                        pin = tuple(x * (1.0 + sc * self.rng.choice([-1.0, 1.0], x.shape)) for x in bin_)
                        r = (np.abs(self.step_fn(p, pin) - dev[rep]) / scale[rep]).max(1)
                        best = np.minimum(best, r.reshape(len(idx), n).min(1))
                        continue
                    for _ in range(n):
                        p = perturbed(sub, sc, self.rng, self.fields, jc)
                        pin = tuple(x * (1.0 + sc * self.rng.choice([-1.0, 1.0], x.shape)) for x in sin)
                        o = self.step_fn(p, pin)
                        best = np.minimum(best, (np.abs(o - dev) / scale).max(1))
            for j, b in enumerate(idx):
                if best[j] > E[t, b] / REPRO_GAIN:
                    out.append((int(t), int(b), float(E[t, b]), float(best[j])))
        return out, len(big)

    def _explain(self, limit=None):
        """(E, S, unexplained, n_deep): the errors, the sensitivities after the deep probe of every sample that fails the
        quick estimate, the samples that stay above  C sens + floor  as (t, env, err, sens, where), and how many samples
        needed the deep probe.  limit (CPU self-tests only): deep-probe only the `limit` samples furthest above the quick
        bound -- the others are neither explained nor reported."""
        E, S = np.array(self.err), np.array(self.sens)
        F = self.floor
        bad = np.argwhere(E > C_SENS * S + F)
        if limit is not None and len(bad) > limit:
            over = (E / (C_SENS * S + F))[bad[:, 0], bad[:, 1]]
            bad = bad[np.argsort(-over, kind='stable')[:limit]]
        n_deep = len(bad)
        unexplained = []
        for t in np.unique(bad[:, 0]) if n_deep else []:
            idx = bad[bad[:, 0] == t, 1]
            sub = slice_env(self.snaps[t], idx)
            sin = tuple(x[idx] for x in self.inputs[t])
            s2 = self._sens(sub, sin, self.base[t][idx], self.deep_scales, 48)
            for j, b in enumerate(idx):
                S[t, b] = max(S[t, b], s2[j])
                if E[t, b] > C_SENS * S[t, b] + F:
                    unexplained.append((int(t), int(b), float(E[t, b]), float(S[t, b]), 'output %d' % self.where[t][b]))
        return E, S, unexplained, n_deep

    def finish_float64(self, what='', max_loose=1.0):
        """The float64 rule on ill-conditioned states (a recorder built with float64-sized scales and floor = the suite's
        float64 bound): EVERY sample within  floor + C sens;  the share of samples whose allowance C sens exceeds the floor
        itself (the bound is more than twice the suite's) is capped by max_loose."""
        E, S, unexplained, n_deep = self._explain()
        loose = float(np.mean(C_SENS * S > self.floor))
        summary = ('%s: %d samples, err median %.2e / p99.9 %.2e / max %.2e; err / (%.0e + C sens) max %.2f; largest '
                   'allowance %.2e; %d samples needed the deep probe; C sens > %.0e on %.2f %% of the samples (ceiling %.1f %%)'
                   % (what, E.size, np.median(E), np.quantile(E, 0.999), E.max(), self.floor,
                      (E / (C_SENS * S + self.floor)).max(), (C_SENS * S + self.floor).max(), n_deep, self.floor, 100 * loose,
                      100 * max_loose))
        assert np.isfinite(E).all(), 'non-finite errors: ' + summary
        assert loose <= max_loose, 'the float64 allowance is loose on too many samples: ' + summary
        assert not unexplained, 'UNEXPLAINED float64 errors (t, env, err, sens, where): %s | %s' % (unexplained[:10], summary)
        return summary

    def finish(self, what='', max_vacuous=0.4):
        E, S, unexplained, n_deep = self._explain()
        ratio = E / (C_SENS * S + self.floor)
        self.bound = C_SENS * S + self.floor                  # kept for followed_chart_errors
        vac = float(np.mean(self.bound > VACUOUS))
        summary = ('%s: %d samples, err median %.2e / p99.9 %.2e / max %.2e; err / (C sens + floor) max %.2f; '
                   '%d samples needed the deep probe; bound vacuous (> %.0e) on %.2f %% of the samples (ceiling %.1f %%)'
                   % (what, E.size, np.median(E), np.quantile(E, 0.999), E.max(), ratio.max(), n_deep, VACUOUS, 100 * vac,
                      100 * max_vacuous))
        assert vac <= max_vacuous, 'the sensitivity bound is vacuous on too many samples: ' + summary
        unrep, n_big = self._unreproduced(E)
        summary += '; %d errors > %.0e, %d not reproduced by a perturbed oracle' % (n_big, REPRO_ERR, len(unrep))
        assert len(unrep) <= MAX_UNREPRODUCED * E.size, 'large errors that are no branch of the oracle ' \
            '(t, env, err, closest perturbed oracle): %s | %s' % (unrep[:10], summary)
        assert not unexplained, 'UNEXPLAINED float32 errors (t, env, err, sens, where): %s | %s' % (unexplained[:10], summary)
        assert np.median(E) < 2e-5 and np.quantile(E, 0.99) < 2e-3, summary      # and the bulk is at rounding level
        return summary


def skip_pattern_of_rref(Nr, tol=1e-6):
    """The pivot-or-skip decisions behind an rref'd null basis Nr [B, n, k] (null_space_coordinate.rref, column vectors):
    row j of Nr is the unit vector e_i exactly when column j was the i-th pivot column; a column that was skipped (its
    candidates <= the tolerance, zeroed from row i down) carries zeros in the entries i.. only.  Returns bool [B, n]: True =
    skipped (columns after the last pivot are reported as pivots -- they are never tested)."""
    Nr = np.asarray(Nr, dtype=np.float64)
    B, n, k = Nr.shape
    i = np.zeros(B, dtype=np.int64)
    skip = np.zeros((B, n), dtype=bool)
    eye = np.eye(k)
    for j in range(n):
        active = i < k
        unit = np.abs(Nr[:, j, :] - eye[np.minimum(i, k - 1)]).max(1) < tol
        piv = active & unit
        skip[:, j] = active & ~unit
        i = i + piv
    return skip


def followed_chart_errors(rec, follow_fn, tol=1e-4, only_vacuous=True, decisions=None):
    """VERDICT r3 item 3b.  For the samples whose sensitivity bound says nothing (> VACUOUS), compare the device with the
    float64 oracle FORCED ONTO THE DEVICE'S OWN CHART DECISIONS: follow_fn(Jc [b, c, n]) -> bool [b, n] (the pivot / skip
    pattern the device's float32 rref takes on these matrices, read off atacom_nullspace).  Call after finish().
    Returns (number of such samples, their errors against the following oracle, their errors against the plain oracle).
    decisions (optional dict): filled with 'same' / 'total' -- in how many of the chart evaluations behind
    these samples (one per physics sub-step) the device's whole pivot / skip pattern IS the float64 oracle's own."""
    from oracle import atacom_batched as ob
    E = np.array(rec.err)
    sel = rec.bound > VACUOUS if only_vacuous else np.ones_like(rec.bound, dtype=bool)
    e_follow, e_plain = [], []
    same = total = 0

    def counted(sub):
        k, rtol = sub.spec.n_null, sub.spec.rref_tol

        def f(Jc):
            nonlocal same, total
            dev = follow_fn(Jc)
            _, N = ob.bidiag_solve_null(Jc, np.zeros(Jc.shape[:2]), k)
            own = skip_pattern_of_rref(ob.rref_tol(N, rtol))
            same += int((dev == own).all(1).sum())
            total += len(dev)
            return dev
        return f
    for t in range(E.shape[0]):
        idx = np.nonzero(sel[t])[0]
        if not len(idx):
            continue
        sub = slice_env(rec.snaps[t], idx)
        sub.chart_follow = counted(sub) if decisions is not None else follow_fn
        out = rec.step_fn(sub, tuple(x[idx] for x in rec.inputs[t]))
        dev = rec.dev[t][idx]
        e_follow.append((np.abs(dev - out) / np.maximum(1.0, np.abs(out))).max(1))
        e_plain.append(E[t, idx])
    if decisions is not None:
        decisions['same'], decisions['total'] = same, total
    if not e_follow:
        return 0, np.zeros(0), np.zeros(0)
    return int(sel.sum()), np.concatenate(e_follow), np.concatenate(e_plain)


def assert_matrix_fn_explained(fn, A, dev_out, what='', seed=0, max_vacuous=0.4):
    """The same rule for a stand-alone primitive  out = fn(A)  on a batch of matrices A [n, M, N] (e.g. the chart
    rref(null(A), tol)): every float32 device result within C x (float64 fn's response to float32-sized relative
    perturbations of A) + floor; samples failing the quick estimate get the deep probe; none may stay unexplained."""
    rng = np.random.default_rng(seed)
    base = fn(A).reshape(len(A), -1)
    scale = np.maximum(1.0, np.abs(base))
    err = (np.abs(np.asarray(dev_out, dtype=np.float64).reshape(len(A), -1) - base) / scale).max(1)

    def sens(idx, scales, draws):
        s = np.zeros(len(idx))
        for sc in scales:
            for _ in range(draws):
                Ai = A[idx]
                Ap = Ai * (1.0 + sc * rng.choice([-1.0, 1.0], Ai.shape)) \
                    + JC_NOISE_FRACTION * sc * np.abs(Ai).max((1, 2), keepdims=True) * rng.choice([-1.0, 1.0], Ai.shape)
                out = fn(Ap).reshape(len(idx), -1)
                s = np.maximum(s, (np.abs(out - base[idx]) / scale[idx]).max(1))
        return s

    S = sens(np.arange(len(A)), QUICK_SCALES, 2)
    bad = np.nonzero(err > C_SENS * S + FLOOR)[0]
    if len(bad):
        S[bad] = np.maximum(S[bad], sens(bad, DEEP_SCALES, 48))
    still = bad[err[bad] > C_SENS * S[bad] + FLOOR]
    vac = float(np.mean(C_SENS * S + FLOOR > VACUOUS))
    summary = '%s: %d matrices, err median %.2e max %.2e, %d needed the deep probe, bound vacuous on %.2f %%' % (
        what, len(A), np.median(err), err.max(), len(bad), 100 * vac)
    assert vac <= max_vacuous, 'the sensitivity bound is vacuous on too many samples: ' + summary
    assert len(still) == 0, 'UNEXPLAINED: %s | %s' % ([(int(i), float(err[i]), float(S[i])) for i in still[:10]], summary)
    return summary
