"""ctypes binding of libatacom_fit.so (include/atacom_fit_hip.h): the gradient of the value loss of a critic, or of PPO's
clipped surrogate of an actor, over the rows of a finished collection.  The library has no handle; a call is one argument
struct.  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C

from . import _binding
from ._binding import AtacomError, OK, E_INVALID, E_HIP, E_UNSUPPORTED, F32, F64  # noqa: F401
from ._lib import AtacomMlp
from ._lib_evaluate import View

MAX_IN, MAX_OUT, HIDDEN, MAX_BLOCKS, STATS = 32, 8, 64, 65535, 4
VALUE, PPO_CLIP = 0, 1


class FitArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_blocks', C.c_int32),
                ('head', C.c_int32), ('reserved', C.c_int32), ('n_outer', C.c_int64), ('n_inner', C.c_int64), ('net', AtacomMlp),
                ('x', View), ('action', View), ('weight', View), ('logp_old', View), ('idx', C.c_void_p), ('n_idx', C.c_int64),
                ('clip', C.c_double), ('grad', C.c_void_p), ('stats', C.c_void_p), ('workspace', C.c_void_p),
                ('workspace_bytes', C.c_size_t), ('stream', C.c_void_p)]


def new_args(cls=FitArgs):
    return _binding.new_args(cls)                     # the one struct of this library is the default


def grad_size(n_in, n_out, head):
    """The values of `grad`: P, and n_out more (d log std) for the PPO head."""
    return 64 * n_in + 64 + 4096 + 64 + 64 * n_out + n_out + (n_out if head == PPO_CLIP else 0)


_int = C.c_int
# {symbol: (restype, argtypes)}: every function of include/atacom_fit_hip.h
SIGNATURES = {
    'atacom_fit_version': (C.c_char_p, None),
    'atacom_fit_last_error': (C.c_char_p, None),
    'atacom_fit_workspace_size': (C.c_size_t, [C.POINTER(FitArgs)]),
    'atacom_fit_gradient': (_int, [C.POINTER(FitArgs)]),
}
EXPORTS = list(SIGNATURES)
LIB_PATH, load, check = _binding.library('fit', SIGNATURES)
