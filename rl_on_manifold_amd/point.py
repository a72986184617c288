"""The collision-avoidance task (the reference's PointReachAtacom,
atacom/environments/collision_avoidance/collision_avoidance_atacom.py:8) on libatacom_point.so.

  BatchedPointReachEnv   B environments on one device, torch tensors in and out, the surface of BatchedAtacomEnv
  PointReachAtacom       batch-1 numpy facade with the reference's constructor, argument for argument

All arithmetic happens in the libraries (hand-written HIP, gfx950); this file only moves pointers.  Collection with an
MlpPolicy (rollout_policy, rollout_packed) runs the fused kernel of libatacom_point_policy.so on the same handle,
rollout_compact the kernel of libatacom_point_compact.so, and the masked step and the checkpoint (step(mask=...), snapshot,
restore) those of libatacom_point_vec.so.

Random numbers.  The reference draws the obstacles' reset positions and random-walk accelerations from numpy's global
generator.  Here a call either receives the draws (`draws=`, the values np.random.uniform returned) or, by default,
the device draws them from the engine's counter-based generator keyed (seed, environment, episode, draw) -- the
distribution of the reference, reproducible, and restated in tests/point_reach_oracle.py.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib_point, _lib_point_compact, _lib_point_policy, _lib_point_vec
from ._device_env import DeviceEnv, _ptr, step_to_host
from .rollout import record_fields
from .spaces import Box, MDPInfo


class BatchedPointReachEnv(DeviceEnv):
    _destroy = 'atacom_point_destroy'

    def __init__(self, batch, n_objects=4, random_walk=True, time_step=0.01, horizon=1000, gamma=0.99, seed=0,
                 auto_reset=True, device='cuda:0', dtype=torch.float32):
        """The state is zero until the first reset(): like the reference's constructor, this one does not reset (the
        circle centres of random_walk=False are those of the FIRST reset, for the life of the object)."""
        lib = _lib_point.load()
        self._init_device(device, dtype, _lib_point.check,
                          ValueError("the engine runs on a ROCm device ('cuda:N'); there is no CPU path"))
        cfg = _lib_point.default_config()
        cfg.batch, cfg.n_objects, cfg.random_walk = int(batch), int(n_objects), int(bool(random_walk))
        cfg.dtype = _lib_point.F32 if dtype == torch.float32 else _lib_point.F64
        cfg.horizon, cfg.auto_reset, cfg.seed = int(horizon), int(bool(auto_reset)), int(seed) & 0x7fffffff
        cfg.dt, cfg.gamma = float(time_step), float(gamma)
        self.cfg, self.batch, self.n_objects, self.random_walk = cfg, int(batch), int(n_objects), bool(random_walk)
        n = self.n_objects
        self.obs_dim, self.state_dim = 4 * (1 + n), 7 * n + 8
        self.dims = {'q': 2, 'f': 0, 'g': n, 'null': 2, 'c': n}
        h = C.c_void_p()
        _lib_point.check(lib.atacom_point_create(C.byref(cfg), self._dev_index, C.byref(h)))
        self._h, self._lib = h, lib
        # collision_avoidance_base.py:12-14
        self._mdp_info = MDPInfo(Box(-np.ones(self.obs_dim) * 10, np.ones(self.obs_dim) * 10), Box(-np.ones(2), np.ones(2)),
                                 cfg.gamma, cfg.horizon)

    # ------------------------------------------------------------------ reference surface
    @property
    def info(self):
        return self._mdp_info

    def seed(self, seed):
        """Re-keys the device generator from the next call on."""
        self.cfg.seed = int(seed) & 0x7fffffff
        _lib_point.check(self._lib.atacom_point_set_seed(self._h, self.cfg.seed))

    def reset(self, mask=None, draws=None):
        """Reset the masked environments (all if mask is None).  draws (optional) [B, n_objects, 2]: the obstacle
        positions, values of U(2, 8).  Returns the observation of every environment."""
        m = None if mask is None else self._as_dev(mask, (self.batch,), torch.uint8)
        d = None if draws is None else self._as_dev(draws, (self.batch, self.n_objects, 2))
        obs = self._empty(self.batch, self.obs_dim)
        _lib_point.check(self._lib.atacom_point_reset(self._h, _ptr(m), _ptr(d), _ptr(obs), self._stream()))
        return obs

    def _vec_lib(self):
        if getattr(self, '_vlib', None) is None:
            self._vlib = _lib_point_vec.load()
        return self._vlib

    def _launch_step(self, actions, draws, obs, reward, absorbing, last, mask):
        """atacom_point_step, or atacom_point_vec_step_masked when there is a mask, on the caller's current stream."""
        if mask is None:
            _lib_point.check(self._lib.atacom_point_step(self._h, _ptr(actions), _ptr(draws), _ptr(obs), _ptr(reward),
                                                         _ptr(absorbing), _ptr(last), self._stream()))
        else:
            _lib_point_vec.check(self._vec_lib().atacom_point_vec_step_masked(
                self._h, _ptr(mask), _ptr(actions), _ptr(draws), _ptr(obs), _ptr(reward), _ptr(absorbing), _ptr(last),
                self._stream()))

    def step(self, actions, draws=None, mask=None):
        """actions [B, 2]; draws (optional) [B, n_objects, 2], values of U(-1, 1) for the random walk; mask (optional, [B] bool
        / uint8): environments with a zero entry sit the call out ON THE DEVICE -- state, counters and statistics untouched, no
        random numbers consumed, obs = their current observation, reward 0, flags False; their action and draw rows are not read.
        -> (obs, reward, absorbing, {'last': ...}) in fresh tensors."""
        B = self.batch
        a = self._as_dev(actions, (B, 2))
        d = None if draws is None else self._as_dev(draws, (B, self.n_objects, 2))
        obs, reward = self._empty(B, self.obs_dim), self._empty(B)
        absorbing, last = self._empty(B, dtype=torch.uint8), self._empty(B, dtype=torch.uint8)
        if mask is not None:
            mask = mask.view(torch.uint8) if (isinstance(mask, torch.Tensor) and mask.dtype == torch.bool
                                              and self._on_my_device(mask) and mask.is_contiguous()) \
                else self._as_dev(mask, (B,), torch.uint8)
            if tuple(mask.shape) != (B,):
                raise ValueError("expected a mask of shape (%d,), got %s" % (B, tuple(mask.shape)))
        self._launch_step(a, d, obs, reward, absorbing, last, mask)
        return obs, reward, absorbing.view(torch.bool), {'last': last.view(torch.bool)}

    def step_into(self, actions, obs, reward, absorbing, last=None, draws=None, mask=None):
        """Allocation-free variant of step(): caller-owned output tensors (uint8 for the flags).  `mask` (uint8 [B], optional):
        environments with a zero byte sit the call out on the device (atacom_point_vec_step_masked)."""
        B = self.batch
        self._check_io(actions, (B, 2), self.dtype, 'actions')
        self._check_io(draws, (B, self.n_objects, 2), self.dtype, 'draws')
        self._check_io(obs, (B, self.obs_dim), self.dtype, 'obs')
        self._check_io(reward, (B,), self.dtype, 'reward')
        self._check_io(absorbing, (B,), torch.uint8, 'absorbing')
        self._check_io(last, (B,), torch.uint8, 'last')
        self._check_io(mask, (B,), torch.uint8, 'mask')
        self._launch_step(actions, draws, obs, reward, absorbing, last, mask)

    def observe_into(self, obs):
        """The observation of the CURRENT state into obs [B, obs_dim]: the masked reset with a mask that selects nobody.
        Enqueue-only (what GraphedRollout captures)."""
        self._check_io(obs, (self.batch, self.obs_dim), self.dtype, 'obs')
        _lib_point.check(self._lib.atacom_point_reset(self._h, _ptr(self._nobody()), None, _ptr(obs), self._stream()))

    def rollout(self, actions, draws=None, want_next_obs=True, out=None):
        """T env steps in one kernel launch.  actions [T, B, 2], draws (optional) [T, B, n_objects, 2]
        -> dict(obs, next_obs, reward, absorbing, last, action), the layout of BatchedAtacomEnv.rollout."""
        T = int(actions.shape[0])
        B = self.batch
        a = self._as_dev(actions, (T, B, 2))
        d = None if draws is None else self._as_dev(draws, (T, B, self.n_objects, 2))
        if out is None:
            out = self._rollout_buffers(T, want_next_obs, with_action=False)
        _lib_point.check(self._lib.atacom_point_rollout(self._h, T, _ptr(a), _ptr(d), _ptr(out['obs']),
                                                        _ptr(out.get('next_obs')), _ptr(out['reward']),
                                                        _ptr(out['absorbing']), _ptr(out['last']), self._stream()))
        out['action'] = a
        return out

    @property
    def record_dim(self):
        """Values of one packed record: [obs | action(2) | reward | next_obs | absorbing | last]."""
        return record_fields(self.obs_dim, 2)[1]

    def _policy_lib(self):
        if getattr(self, '_plib', None) is None:
            self._plib = _lib_point_policy.load()
        return self._plib

    def rollout_policy(self, policy, n_steps, noise=None, draws=None, want_next_obs=True):
        """T = n_steps env steps driven by a policy; returns the dict of rollout(), 'action' being what the policy drew.

        * `policy` is an MlpPolicy (anything with `as_struct`): the FUSED kernel of libatacom_point_policy.so -- actor network
          and exploration evaluated inside the rollout kernel, ONE launch for the whole phase.  `noise` [T, B, 2] standard-normal
          draws supplied by the caller (None = zeros), `draws` [T, B, n_objects, 2] values of U(-1, 1) for the random walk
          (None = the device generator, the keys of rollout()).
        * `policy` is any other callable / module mapping observations [B, obs_dim] to actions [B, 2]: a HOST LOOP of
          policy.forward + step, n_steps launches of each, starting from the current observation (`noise` and `draws` are not
          taken there: the callable owns its exploration)."""
        if hasattr(policy, 'as_struct'):
            T, B = int(n_steps), self.batch
            net = policy.as_struct(self)
            nz = None if noise is None else self._as_dev(noise, (T, B, 2))
            d = None if draws is None else self._as_dev(draws, (T, B, self.n_objects, 2))
            out = self._rollout_buffers(T, want_next_obs)
            _lib_point_policy.check(self._policy_lib().atacom_point_policy_rollout(
                self._h, T, C.byref(net), _ptr(nz), _ptr(d), _ptr(out['obs']), _ptr(out['next_obs']), _ptr(out['action']),
                _ptr(out['reward']), _ptr(out['absorbing']), _ptr(out['last']), self._stream()))
            return out
        if noise is not None or draws is not None:
            raise ValueError("noise / draws go with an MlpPolicy (the fused kernel); a plain callable runs the host loop and "
                             "owns its exploration")
        T, D = int(n_steps), self.obs_dim
        out = self._rollout_buffers(T)
        fwd = policy.forward if hasattr(policy, 'forward') else policy
        obs = self.get_state()[:, :D].contiguous()
        with torch.no_grad():
            for t in range(T):
                out['obs'][t] = obs
                out['action'][t] = fwd(obs).to(self.dtype)
                self.step_into(out['action'][t], out['next_obs'][t], out['reward'][t], out['absorbing'][t], out['last'][t])
                # after an in-kernel reset the next observation is the reset state, not the terminal one
                obs = self.get_state()[:, :D].contiguous() if self.cfg.auto_reset else out['next_obs'][t]
        return out

    def rollout_packed(self, actions=None, policy=None, n_steps=None, noise=None, draws=None, out=None, batch_stride=None):
        """T env steps in one launch, written as ONE packed record per (step, env): records [T, batch_stride, record_dim] =
        [obs | action | reward | next_obs | absorbing | last] -- the layout the sharded collector all-gathers as it is
        (rollout.py), the surface of BatchedAtacomEnv.rollout_packed.  Either `actions` [T, B, 2] or `policy` (an MlpPolicy,
        evaluated inside the kernel; `noise` [T, B, 2] or None) with `n_steps`; `draws` as in rollout_policy.  batch_stride >
        batch pads the env axis (ragged shards); the padding rows are zero (filled at allocation, or here when the caller
        supplies `out`) and never written by the kernel."""
        if actions is None and policy is not None and not hasattr(policy, 'as_struct'):
            raise ValueError("rollout_packed takes an MlpPolicy (as_struct); a plain callable goes through rollout_policy")
        T, a_ptr, net_ref, noise_ptr, _keep = self._source(actions, policy, n_steps, noise)
        ld = self.batch if batch_stride is None else int(batch_stride)
        out = self._packed_out(T, ld, self.record_dim, out)
        d = None if draws is None else self._as_dev(draws, (T, self.batch, self.n_objects, 2))
        _lib_point_policy.check(self._policy_lib().atacom_point_policy_rollout_packed(
            self._h, T, a_ptr, net_ref, noise_ptr, _ptr(d), _ptr(out), ld, self._stream()))
        return out

    def rollout_compact(self, actions=None, policy=None, n_steps=None, noise=None, draws=None, out=None, batch_stride=None,
                        ends_capacity=None):
        """rollout_packed() in the compact record format (atacom_point_compact_rollout), which does not repeat next_obs -- the
        surface of BatchedAtacomEnv.rollout_compact plus `draws`.  Returns (records [T + 1, batch_stride, D + 5], ends [n, D + 2], n):
          records rows 0..T-1 = [obs | action | reward | absorbing | last], row T = [obs after the last step | zeros];
          ends = one row [t, b, terminal obs] per episode end at t < T-1 of an auto-resetting engine, in no particular order.
        rollout.CompactRecordLayout rebuilds the full records' fields from them.  ends_capacity (default (T-1) * batch, the
        worst case) rows are allocated on the device; at the task's horizon of 1000 about batch * T / 1000 are used.  `out` = (records,
        ends) caller buffers of those shapes (ends [ends_capacity, D + 2]); padding rows are zeroed as in rollout_packed.
        Reads the row count back: synchronises the current stream once.  Raises ValueError when the count exceeds the
        capacity -- the rows past it are lost, and the engine has advanced all the same."""
        if actions is None and policy is not None and not hasattr(policy, 'as_struct'):
            raise ValueError("rollout_compact takes an MlpPolicy (as_struct); a plain callable goes through rollout_policy")
        T, a_ptr, net_ref, noise_ptr, _keep = self._source(actions, policy, n_steps, noise)
        d = None if draws is None else self._as_dev(draws, (T, self.batch, self.n_objects, 2))
        lib = _lib_point_compact.load()

        def call(rec, ld, ends, cap, n_ends):
            _lib_point_compact.check(lib.atacom_point_compact_rollout(
                self._h, T, a_ptr, net_ref, noise_ptr, _ptr(d), _ptr(rec), ld, _ptr(ends), cap, _ptr(n_ends), self._stream()))
        return self._rollout_compact(call, T, batch_stride, ends_capacity, out)

    def get_constraints_logs(self, clear=True):
        """(c_avg, c_max, c_dq_max) over every step of every environment since the last clear; c_dq_max is the
        reference's constant 0 (collision_avoidance_atacom.py:40-41)."""
        res = (C.c_double * 3)()
        _lib_point.check(self._lib.atacom_point_get_stats(self._h, C.byref(res), int(clear), self._stream()))
        return float(res[0]), float(res[1]), float(res[2])

    def snapshot(self, out=None):
        """Checkpoint of the WHOLE handle (atacom_point_vec_snapshot_save): the state, the step and episode counters as the
        integers they are, and the constraint statistics, which get_state() leaves out -- an opaque uint8 tensor on the device;
        `restore(image)` followed by the same calls reproduces the run and its get_constraints_logs() bit for bit.  One launch
        on the current stream, no synchronisation: capturable."""
        lib = self._vec_lib()
        n = int(lib.atacom_point_vec_snapshot_bytes(self._h))
        if n < 0:
            _lib_point_vec.check(n)
        if out is None:
            out = torch.empty((n,), device=self.device, dtype=torch.uint8)
        elif out.dtype != torch.uint8 or out.numel() < n or not self._on_my_device(out) or not out.is_contiguous():
            raise ValueError("snapshot buffer must be a contiguous uint8 tensor of >= %d bytes on %s" % (n, self.device))
        _lib_point_vec.check(lib.atacom_point_vec_snapshot_save(self._h, _ptr(out), self._stream()))
        return out

    def restore(self, image):
        """Puts a snapshot() back, the generator key included (`cfg.seed` follows); horizon, time step, obstacle mode and
        auto_reset stay this engine's.  The image's header is read back first (synchronises the current stream) and checked
        against the engine before anything is written: an image of another n_objects, dtype, batch or format raises AtacomError
        naming the field and leaves state, statistics and key as they were."""
        lib = self._vec_lib()
        if not isinstance(image, torch.Tensor) or image.dtype != torch.uint8 or image.numel() < 64 \
                or not self._on_my_device(image) or not image.is_contiguous():
            raise ValueError("snapshot image must be a contiguous uint8 tensor on %s" % (self.device,))
        n = int(lib.atacom_point_vec_snapshot_bytes(self._h))
        if n < 0:
            _lib_point_vec.check(n)
        # an image of another shape is refused here by its header, with the field named, before its size is looked at
        seed = C.c_int32(0)
        _lib_point_vec.check(lib.atacom_point_vec_snapshot_inspect(self._h, _ptr(image), C.byref(seed), self._stream()))
        if image.numel() < n:
            raise ValueError("snapshot image is truncated: %d bytes, %d expected" % (image.numel(), n))
        _lib_point_vec.check(lib.atacom_point_vec_snapshot_restore(self._h, _ptr(image), self._stream()))
        self.cfg.seed = int(seed.value)

    def get_state(self):
        """[B, 7 n + 8] = [observation, s, first-reset centres, _time, steps taken, episodes started, centres set]."""
        st = self._empty(self.batch, self.state_dim)
        _lib_point.check(self._lib.atacom_point_get_state(self._h, _ptr(st), self._stream()))
        return st

    def set_state(self, state):
        st = self._as_dev(state, (self.batch, self.state_dim))
        _lib_point.check(self._lib.atacom_point_set_state(self._h, _ptr(st), self._stream()))


class PointReachAtacom:
    """collision_avoidance_atacom.py:8-17, argument for argument; numpy in, numpy copies out.  The obstacles' draws come
    from the device generator (seed()); `reset(draws=...)` / `step(a, draws=...)` replay recorded ones."""

    def __init__(self, time_step=0.01, horizon=1000, gamma=0.99, n_objects=4, random_walk=False, device='cuda:0',
                 dtype=torch.float32):
        self.time_step, self.n_objects, self.random_walk = time_step, n_objects, random_walk
        # mushroom_rl.Core resets between episodes, so the facade does not reset inside a step
        self._engine = BatchedPointReachEnv(1, n_objects=n_objects, random_walk=random_walk, time_step=time_step,
                                            horizon=horizon, gamma=gamma, auto_reset=False, device=device, dtype=dtype)
        self.dims = self._engine.dims
        self.state = np.zeros(self._engine.obs_dim)

    @property
    def info(self):
        return self._engine.info

    @property
    def s(self):
        n = self.n_objects
        return self._engine.get_state()[0, 4 * (1 + n):4 * (1 + n) + n].cpu().numpy().astype(np.float64)

    def seed(self, seed):
        self._engine.seed(seed)

    def render(self):
        pass

    def stop(self):
        self._engine.stop()

    def reset(self, state=None, draws=None):
        """`state` is accepted and ignored, as in the reference (collision_avoidance_base.py:25-39)."""
        d = None if draws is None else np.asarray(draws, dtype=np.float64).reshape(1, self.n_objects, 2)
        self.state = self._engine.reset(draws=d)[0].cpu().numpy().astype(np.float64)
        return self.state.copy()

    def step(self, action, draws=None):
        d = None if draws is None else np.asarray(draws, dtype=np.float64).reshape(1, self.n_objects, 2)
        self.state, reward, absorbing = step_to_host(self._engine, action, draws=d)
        return self.state.copy(), reward, absorbing, {}

    def get_constraints_logs(self):
        return self._engine.get_constraints_logs()
