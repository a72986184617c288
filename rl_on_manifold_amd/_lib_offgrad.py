"""ctypes binding of libatacom_offgrad.so (include/atacom_offgrad_hip.h): the gradient of the critics' mean-squared TD error and
the deterministic policy gradient of the actor of a DDPG / TD3 update, over a minibatch gathered from a replay memory in place.
The library has no handle; a call is one argument struct.  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C

from . import _binding
from ._binding import AtacomError, OK, E_INVALID, E_HIP, E_UNSUPPORTED, F32, F64  # noqa: F401
from ._lib import AtacomMlp
from ._lib_evaluate import View

DDPG, TD3 = 0, 1
MAX_IN, MAX_ACT, HIDDEN, MAX_BLOCKS, STATS = 32, 8, 64, 65535, 4


class Critic(C.Structure):
    """atacom_offgrad_critic: field for field the Critic of _lib_offpolicy."""
    _fields_ = [('kind', C.c_int32), ('n_obs', C.c_int32), ('n_act', C.c_int32), ('activation', C.c_int32)] + \
               [(k, C.c_void_p) for k in ('W1', 'b1', 'W2', 'b2', 'W2a', 'W3', 'b3', 'obs_shift', 'obs_scale', 'act_scale')]


class CriticArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_blocks', C.c_int32),
                ('n_critics', C.c_int32), ('reserved', C.c_int32), ('n_outer', C.c_int64), ('n_inner', C.c_int64),
                ('critics', Critic * 2), ('obs', View), ('action', View), ('target', C.c_void_p), ('target_stride', C.c_int64),
                ('idx', C.c_void_p), ('n_idx', C.c_int64), ('grad', C.c_void_p * 2), ('stats', C.c_void_p * 2),
                ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('stream', C.c_void_p)]


class ActorArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_blocks', C.c_int32),
                ('n_outer', C.c_int64), ('n_inner', C.c_int64), ('actor', AtacomMlp), ('critic', Critic), ('obs', View),
                ('idx', C.c_void_p), ('n_idx', C.c_int64), ('grad', C.c_void_p), ('stats', C.c_void_p),
                ('action_out', C.c_void_p), ('action_out_stride', C.c_int64), ('dqda_out', C.c_void_p),
                ('dqda_out_stride', C.c_int64), ('workspace', C.c_void_p), ('workspace_bytes', C.c_size_t), ('stream', C.c_void_p)]


def new_args(cls):
    return _binding.new_args(cls)


def grad_size(n_in, n_out, n_act):
    """The values of a gradient: W1, b1, W2, b2, W3, b3 and, for a critic (n_act = k), W2a."""
    return 64 * n_in + 64 + 4096 + 64 + 64 * n_out + n_out + 64 * n_act


_int = C.c_int
# {symbol: (restype, argtypes)}: every function of include/atacom_offgrad_hip.h
SIGNATURES = {
    'atacom_offgrad_version': (C.c_char_p, None),
    'atacom_offgrad_last_error': (C.c_char_p, None),
    'atacom_offgrad_workspace_size': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    'atacom_offgrad_critic_gradient': (_int, [C.POINTER(CriticArgs)]),
    'atacom_offgrad_actor_gradient': (_int, [C.POINTER(ActorArgs)]),
}
EXPORTS = list(SIGNATURES)
LIB_PATH, load, check = _binding.library('offgrad', SIGNATURES)
