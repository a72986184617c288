"""ctypes binding of libatacom_optim.so (include/atacom_optim_hip.h): one Adam step of up to four parameter groups in one
launch, with the step count and the powers of the betas in device memory.  The library has no handle; a call is one argument
struct.  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C

from . import _binding
from ._binding import AtacomError, OK, E_INVALID, E_HIP, E_UNSUPPORTED, F32, F64  # noqa: F401

MAX_GROUPS, MAX_IN, MAX_OUT, HIDDEN, HEAD = 4, 32, 8, 64, 32
PARAMS = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')


class Group(C.Structure):
    _fields_ = [('n_in', C.c_int32), ('n_out', C.c_int32)] + [(k, C.c_void_p) for k in PARAMS] + \
               [('log_std', C.c_void_p), ('std', C.c_void_p), ('grad', C.c_void_p), ('state', C.c_void_p),
                ('lr', C.c_double), ('grad_scale', C.c_double)]


class OptimArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_groups', C.c_int32),
                ('beta1', C.c_double), ('beta2', C.c_double), ('eps', C.c_double), ('stream', C.c_void_p),
                ('groups', Group * MAX_GROUPS)]


def new_args(cls=OptimArgs):
    return _binding.new_args(cls)                     # the one struct of this library is the default


def group_size(n_in, n_out, has_log_std):
    """N, the parameters of a group: the values of its gradient and of each moment."""
    return 64 * n_in + 64 + 4096 + 64 + 64 * n_out + n_out + (n_out if has_log_std else 0)


_int = C.c_int
# {symbol: (restype, argtypes)}: every function of include/atacom_optim_hip.h
SIGNATURES = {
    'atacom_optim_version': (C.c_char_p, None),
    'atacom_optim_last_error': (C.c_char_p, None),
    'atacom_optim_state_size': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    'atacom_optim_adam_init': (_int, [C.POINTER(OptimArgs)]),
    'atacom_optim_adam_step': (_int, [C.POINTER(OptimArgs)]),
}
EXPORTS = list(SIGNATURES)
LIB_PATH, load, check = _binding.library('optim', SIGNATURES)
