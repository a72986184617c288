"""ctypes binding of libatacom_offstep.so (include/atacom_offstep_hip.h): one Adam step of up to four parameter groups -- plain
networks or two-branch critics -- and the soft update of their target networks in one launch, with the step count and the powers
of the betas in device memory.  The library has no handle; a call is one argument struct.  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C

from . import _binding
from ._binding import AtacomError, OK, E_INVALID, E_HIP, F32, F64  # noqa: F401

MAX_GROUPS, MAX_IN, MAX_OUT, MAX_ACT, HIDDEN, TENSORS, HEAD = 4, 32, 8, 8, 64, 7, 32
PARAMS = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'W2a')          # the order of a group: that of _lib_offpolicy.PARAMS


class Group(C.Structure):
    _fields_ = [('n_in', C.c_int32), ('n_out', C.c_int32), ('n_act', C.c_int32), ('reserved', C.c_int32)] + \
               [(k, C.c_void_p) for k in PARAMS] + \
               [('target', C.c_void_p * TENSORS), ('grad', C.c_void_p), ('state', C.c_void_p),
                ('lr', C.c_double), ('grad_scale', C.c_double)]


class OffstepArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_groups', C.c_int32),
                ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double), ('tau', C.c_double), ('stream', C.c_void_p),
                ('groups', Group * MAX_GROUPS)]


def new_args(cls=OffstepArgs):
    return _binding.new_args(cls)                     # the one struct of this library is the default


def group_size(n_in, n_out, n_act):
    """N, the parameters of a group: the values of its gradient and of each moment."""
    return 64 * n_in + 64 + 4096 + 64 + 64 * n_out + n_out + 64 * n_act


_int = C.c_int
# {symbol: (restype, argtypes)}: every function of include/atacom_offstep_hip.h
SIGNATURES = {
    'atacom_offstep_version': (C.c_char_p, None),
    'atacom_offstep_last_error': (C.c_char_p, None),
    'atacom_offstep_state_size': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    'atacom_offstep_adam_init': (_int, [C.POINTER(OffstepArgs)]),
    'atacom_offstep_adam_step': (_int, [C.POINTER(OffstepArgs)]),
}
EXPORTS = list(SIGNATURES)
LIB_PATH, load, check = _binding.library('offstep', SIGNATURES)
