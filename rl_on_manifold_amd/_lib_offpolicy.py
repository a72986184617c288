"""ctypes binding of libatacom_offpolicy.so (include/atacom_offpolicy_hip.h): the Q-value of the DDPG / TD3 critic, the fused TD
target of a minibatch gathered from a replay memory in place, and the soft update of the target networks.  The library has no
handle; a call is one argument struct.  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C

from . import _binding
from ._binding import AtacomError, OK, E_INVALID, E_HIP, E_UNSUPPORTED, F32, F64  # noqa: F401
from ._lib import AtacomMlp
from ._lib_evaluate import View

DDPG, TD3 = 0, 1
MAX_IN, MAX_ACT, HIDDEN, MAX_BLOCKS, MAX_PAIRS, TENSORS = 32, 8, 64, 65535, 4, 7
PARAMS = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'W2a')          # the tensor order of a soft-update pair


class Critic(C.Structure):
    _fields_ = [('kind', C.c_int32), ('n_obs', C.c_int32), ('n_act', C.c_int32), ('activation', C.c_int32)] + \
               [(k, C.c_void_p) for k in ('W1', 'b1', 'W2', 'b2', 'W2a', 'W3', 'b3', 'obs_shift', 'obs_scale', 'act_scale')]


class QArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_blocks', C.c_int32),
                ('n_outer', C.c_int64), ('n_inner', C.c_int64), ('critic', Critic), ('obs', View), ('action', View),
                ('idx', C.c_void_p), ('n_idx', C.c_int64), ('q', C.c_void_p), ('q_stride', C.c_int64), ('stream', C.c_void_p)]


class TargetArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_blocks', C.c_int32),
                ('n_critics', C.c_int32), ('reserved', C.c_int32), ('n_outer', C.c_int64), ('n_inner', C.c_int64),
                ('actor', AtacomMlp), ('critics', Critic * 2), ('next_obs', View), ('reward', View), ('absorbing', View),
                ('eps', C.c_void_p), ('eps_stride', C.c_int64), ('noise_std', C.c_double), ('noise_clip', C.c_double),
                ('gamma', C.c_double), ('act_low', C.c_void_p), ('act_high', C.c_void_p), ('idx', C.c_void_p),
                ('n_idx', C.c_int64), ('y', C.c_void_p), ('y_stride', C.c_int64), ('action_out', C.c_void_p),
                ('action_out_stride', C.c_int64), ('stream', C.c_void_p)]


class Pair(C.Structure):
    _fields_ = [('n_in', C.c_int32), ('n_out', C.c_int32), ('n_act', C.c_int32), ('reserved', C.c_int32),
                ('target', C.c_void_p * TENSORS), ('online', C.c_void_p * TENSORS)]


class SoftUpdateArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_pairs', C.c_int32),
                ('tau', C.c_double), ('stream', C.c_void_p), ('pairs', Pair * MAX_PAIRS)]


def new_args(cls):
    return _binding.new_args(cls)


_int = C.c_int
# {symbol: (restype, argtypes)}: every function of include/atacom_offpolicy_hip.h
SIGNATURES = {
    'atacom_offpolicy_version': (C.c_char_p, None),
    'atacom_offpolicy_last_error': (C.c_char_p, None),
    'atacom_offpolicy_q': (_int, [C.POINTER(QArgs)]),
    'atacom_offpolicy_target': (_int, [C.POINTER(TargetArgs)]),
    'atacom_offpolicy_soft_update': (_int, [C.POINTER(SoftUpdateArgs)]),
}
EXPORTS = list(SIGNATURES)
LIB_PATH, load, check = _binding.library('offpolicy', SIGNATURES)
