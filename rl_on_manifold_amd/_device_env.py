"""What the device-resident batched environments (engine.BatchedAtacomEnv, point.BatchedPointReachEnv) share on the host:
device and dtype, the caller's stream, argument validation, output buffers, the packed-record views and the handle's life.
No numerics and no library names here: a subclass binds its library's checker (`_check`) and names its destroy function.
"""
import ctypes as C

import numpy as np
import torch

from .rollout import compact_record_fields, record_fields, unpack_fields


def _ptr(t):
    # a plain int (or None) converts to void* through the argtypes of the _lib*.py tables; no c_void_p object per call
    return t.data_ptr() if t is not None else None


# torch.cuda.current_stream(device).cuda_stream builds two Python objects per call (~2 us -- more than the circle
# kernel runs); the raw accessor PyTorch keeps for extension launchers returns the hipStream_t as an int directly
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def step_to_host(engine, action, **kw):
    """One step of a batch-1 engine for the numpy facades -> (state, float reward, bool absorbing).  One device -> host
    transfer (and one synchronisation) per step: observation, reward and flag travel together."""
    obs, r, ab, _ = engine.step(np.asarray(action, dtype=np.float64).reshape(1, -1), **kw)
    host = torch.cat([obs[0], r, ab.to(obs.dtype)]).cpu().numpy().astype(np.float64)
    return host[:-2].copy(), float(host[-2]), bool(host[-1] != 0.0)


def device_mask(env_mask, device, n):
    """What the vectorised surfaces (envs.VectorizedAtacomEnv, envs.VectorizedPointReachEnv) make of an `env_mask`: uint8 [n] on
    `device`, or None for "all" -- decided from the argument alone (None), never by looking at the mask's values (that would be
    a device -> host synchronisation per step).  bool is reinterpreted, uint8 taken as it is, anything else compared with 0."""
    if env_mask is None:
        return None
    m = env_mask if isinstance(env_mask, torch.Tensor) else torch.as_tensor(env_mask)
    m = m.to(device=device)
    if m.dtype == torch.bool:
        m = m.contiguous().view(torch.uint8)
    elif m.dtype != torch.uint8:
        m = (m != 0).view(torch.uint8)
    if tuple(m.shape) != (n,):
        raise ValueError("env_mask must have shape (%d,), got %s" % (n, tuple(m.shape)))
    return m.contiguous()


class DeviceEnv:
    """Base of the batched environments.  A subclass calls `_init_device`, then sets `batch`, `obs_dim`, `dims`, `_lib` and
    `_h` (the library and its handle)."""

    _destroy = None                    # name of the library function that frees `_h`
    # how a compact collection that overflowed its exception list is retried (the end of rollout_compact's message)
    _compact_retry = "take a snapshot() before the call to retry it with a larger ends_capacity"

    def _init_device(self, device, dtype, check, not_a_gpu):
        """`check`: the library's return-code checker; `not_a_gpu`: the exception to raise for a device that is no GPU."""
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise not_a_gpu
        # normalised once: torch.device('cuda') != torch.device('cuda:0'), and every comparison below is on self.device
        self._dev_index = dev.index if dev.index is not None else torch.cuda.current_device()
        self.device = torch.device('cuda', self._dev_index)
        if dtype not in (torch.float32, torch.float64):
            raise ValueError('dtype must be torch.float32 or torch.float64')
        self.dtype = dtype
        self._check = check
        self._io_ok = set()
        self._h = None

    def render(self):
        pass

    def stop(self):
        pass

    def _stream(self):
        if _raw_stream is not None:
            return _raw_stream(self._dev_index)
        return torch.cuda.current_stream(self.device).cuda_stream

    def _as_dev(self, x, shape, dtype=None):
        t = torch.as_tensor(x, dtype=dtype or self.dtype, device=self.device)
        if tuple(t.shape) != tuple(shape):
            raise ValueError("expected shape %s, got %s" % (tuple(shape), tuple(t.shape)))
        return t.contiguous()

    def _empty(self, *shape, dtype=None):
        return torch.empty(shape, device=self.device, dtype=dtype or self.dtype)

    def _on_my_device(self, t):
        return t.device.type == 'cuda' and t.device.index == self._dev_index

    def _check_io(self, t, shape, dtype, what):
        """Raw-pointer entry points read whatever they are given: a float64, strided or host tensor would be read as
        garbage.  Validated once per distinct tensor (keyed by storage, shape, dtype), so the steady state of a loop that
        reuses its buffers pays one dict lookup per argument and allocates nothing."""
        if t is None:
            return
        if not isinstance(t, torch.Tensor) or not self._on_my_device(t):
            raise ValueError("%s must be a torch tensor on %s" % (what, self.device))
        key = (what, t.data_ptr(), t.dtype, tuple(t.shape), t.stride())
        if key in self._io_ok:
            return
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor of shape %s (got %s, %s%s)"
                             % (what, dtype, tuple(shape), t.dtype, tuple(t.shape), '' if t.is_contiguous() else ', strided'))
        if len(self._io_ok) > 4096:
            self._io_ok.clear()
        self._io_ok.add(key)

    def _nobody(self):
        """A reset mask that selects nobody: a masked reset with it is "observe the current state" (kept: a captured graph
        reads it at every replay)."""
        if getattr(self, '_nobody_mask', None) is None:
            self._nobody_mask = torch.zeros((self.batch,), device=self.device, dtype=torch.uint8)
        return self._nobody_mask

    def _rollout_buffers(self, T, want_next_obs=True, with_action=True):
        """The time-major output tensors of a T-step collection (flags as uint8)."""
        B, D, e = self.batch, self.obs_dim, self._empty
        out = {'obs': e(T, B, D), 'next_obs': e(T, B, D) if want_next_obs else None, 'reward': e(T, B),
               'absorbing': e(T, B, dtype=torch.uint8), 'last': e(T, B, dtype=torch.uint8)}
        if with_action:
            out['action'] = e(T, B, self.dims['null'])
        return out

    def _packed_out(self, T, ld, F, out, what='out'):
        """The [T, ld, F] buffer of a packed collection: allocated (zeros when ld > batch pads the env axis) or the
        caller's, validated, with its padding rows zeroed -- the kernel never writes them."""
        B = self.batch
        if out is None:
            return (torch.empty if ld == B else torch.zeros)((T, ld, F), device=self.device, dtype=self.dtype)
        if tuple(out.shape) != (T, ld, F) or not out.is_contiguous() or out.dtype != self.dtype \
                or not self._on_my_device(out):
            raise ValueError("%s must be a contiguous [%d, %d, %d] tensor of the engine's dtype on %s"
                             % (what, T, ld, F, self.device))
        if ld > B:
            out[:, B:].zero_()                  # a caller's buffer may hold anything: the padding rows are zero (rollout.py)
        return out

    def _source(self, actions, policy, n_steps, noise):
        """Where a packed collection takes its actions from: `actions` [T, B, k], or `policy` (an MlpPolicy) with `n_steps`
        and optional `noise` [T, B, k].  -> (T, actions pointer, network reference, noise pointer, what must stay alive
        until the launch)."""
        if (actions is None) == (policy is None):
            raise ValueError("give either actions or policy")
        B, k = self.batch, self.dims['null']
        if actions is not None:
            T = int(actions.shape[0])
            a = self._as_dev(actions, (T, B, k))
            return T, _ptr(a), None, None, a
        T = int(n_steps)
        net = policy.as_struct(self)
        nz = None if noise is None else self._as_dev(noise, (T, B, k))
        return T, None, C.byref(net), _ptr(nz), (net, nz)

    def _rollout_compact(self, call, T, batch_stride, ends_capacity, out):
        """The host side of a collection in the compact record format (rollout.CompactRecordLayout): the records and the
        exception rows allocated or validated, `call(records, ld, ends or None, capacity, n_ends)` -- the subclass's library
        call -- issued, and the count read back (ONE synchronisation of the current stream).
        -> (records [T + 1, ld, Fc], ends[:n], n).  Raises ValueError when the count exceeds the capacity."""
        B = self.batch
        _, Fc, E = compact_record_fields(self.obs_dim, self.dims['null'])
        ld = B if batch_stride is None else int(batch_stride)
        cap = max(T - 1, 0) * B if ends_capacity is None else int(ends_capacity)
        if cap < 0:
            raise ValueError("ends_capacity must be >= 0")
        rec, ends = (None, self._empty(cap, E)) if out is None else out
        rec = self._packed_out(T + 1, ld, Fc, rec, 'out[0]')
        if ends.dim() != 2 or ends.shape[0] < cap or ends.shape[1] != E or not ends.is_contiguous() \
                or ends.dtype != self.dtype or not self._on_my_device(ends):
            raise ValueError("out[1] must be a contiguous [>= %d, %d] tensor of the engine's dtype on %s"
                             % (cap, E, self.device))
        n_ends = self._empty(1, dtype=torch.int32)
        call(rec, ld, ends if cap > 0 else None, cap, n_ends)
        n = int(n_ends.item())
        if n > cap:
            raise ValueError("rollout_compact: %d episode-end rows, capacity %d -- the rows past the capacity were not written. "
                             "The engine has advanced: %s" % (n, cap, self._compact_retry))
        return rec, ends[:n], n

    def unpack_records(self, rec):
        """Views into packed records [..., record_dim] (no copy)."""
        return unpack_fields(rec, record_fields(self.obs_dim, self.dims['null'])[0])

    def close(self):
        if getattr(self, '_h', None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
