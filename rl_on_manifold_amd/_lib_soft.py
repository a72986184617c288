"""ctypes binding of libatacom_soft.so (include/atacom_soft_hip.h): the fused soft TD target, the gradients of the two critics and
of the squashed-Gaussian actor, and the Adam step of log_alpha of a SAC update, over a minibatch gathered from a replay memory in
place.  The library has no handle; a call is one argument struct.  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C

from . import _binding
from ._binding import AtacomError, OK, E_INVALID, E_HIP, E_UNSUPPORTED, F32, F64  # noqa: F401
from ._lib import AtacomMlp
from ._lib_evaluate import View

MAX_IN, MAX_ACT, HIDDEN, MAX_BLOCKS, STATS, ALPHA_STATE = 32, 8, 64, 65535, 4, 48


class Critic(C.Structure):
    """atacom_soft_critic"""
    _fields_ = [('n_obs', C.c_int32), ('n_act', C.c_int32), ('activation', C.c_int32), ('reserved', C.c_int32)] + \
               [(k, C.c_void_p) for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'obs_shift', 'obs_scale')]


class TargetArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_blocks', C.c_int32),
                ('n_critics', C.c_int32), ('reserved', C.c_int32), ('n_outer', C.c_int64), ('n_inner', C.c_int64),
                ('policy', AtacomMlp), ('critics', Critic * 2), ('next_obs', View), ('reward', View), ('absorbing', View),
                ('eps', C.c_void_p), ('eps_stride', C.c_int64), ('act_scale', C.c_void_p), ('act_shift', C.c_void_p),
                ('log_alpha', C.c_void_p), ('gamma', C.c_double), ('idx', C.c_void_p), ('n_idx', C.c_int64),
                ('y', C.c_void_p), ('y_stride', C.c_int64), ('action_out', C.c_void_p), ('action_out_stride', C.c_int64),
                ('logp_out', C.c_void_p), ('logp_out_stride', C.c_int64), ('stream', C.c_void_p)]


class CriticArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_blocks', C.c_int32),
                ('n_critics', C.c_int32), ('reserved', C.c_int32), ('n_outer', C.c_int64), ('n_inner', C.c_int64),
                ('critics', Critic * 2), ('obs', View), ('action', View), ('target', C.c_void_p), ('target_stride', C.c_int64),
                ('idx', C.c_void_p), ('n_idx', C.c_int64), ('grad', C.c_void_p * 2), ('stats', C.c_void_p * 2),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('stream', C.c_void_p)]


class ActorArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_blocks', C.c_int32),
                ('n_outer', C.c_int64), ('n_inner', C.c_int64), ('policy', AtacomMlp), ('critics', Critic * 2), ('obs', View),
                ('eps', C.c_void_p), ('eps_stride', C.c_int64), ('act_scale', C.c_void_p), ('act_shift', C.c_void_p),
                ('log_alpha', C.c_void_p), ('target_entropy', C.c_double), ('idx', C.c_void_p), ('n_idx', C.c_int64),
                ('grad_mu', C.c_void_p), ('grad_sigma', C.c_void_p), ('stats', C.c_void_p),
                ('action_out', C.c_void_p), ('action_out_stride', C.c_int64), ('logp_out', C.c_void_p), ('logp_out_stride', C.c_int64),
                ('q_out', C.c_void_p), ('q_out_stride', C.c_int64), ('dqda_out', C.c_void_p), ('dqda_out_stride', C.c_int64),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('stream', C.c_void_p)]


class AlphaArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('reserved', C.c_int32),
                ('log_alpha', C.c_void_p), ('grad', C.c_void_p), ('state', C.c_void_p),
                ('lr', C.c_double), ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double), ('stream', C.c_void_p)]


def new_args(cls):
    return _binding.new_args(cls)


def grad_size(n_in, n_out):
    """The values of a gradient: W1, b1, W2, b2, W3, b3."""
    return 64 * n_in + 64 + 4096 + 64 + 64 * n_out + n_out


_int = C.c_int
# {symbol: (restype, argtypes)}: every function of include/atacom_soft_hip.h
SIGNATURES = {
    'atacom_soft_version': (C.c_char_p, None),
    'atacom_soft_last_error': (C.c_char_p, None),
    'atacom_soft_workspace_size': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    'atacom_soft_target': (_int, [C.POINTER(TargetArgs)]),
    'atacom_soft_critic_gradient': (_int, [C.POINTER(CriticArgs)]),
    'atacom_soft_actor_gradient': (_int, [C.POINTER(ActorArgs)]),
    'atacom_soft_alpha_step': (_int, [C.POINTER(AlphaArgs)]),
}
EXPORTS = list(SIGNATURES)
LIB_PATH, load, check = _binding.library('soft', SIGNATURES)
