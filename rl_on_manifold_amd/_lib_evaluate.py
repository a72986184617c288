"""ctypes binding of libatacom_evaluate.so (include/atacom_evaluate_hip.h): a critic or actor network, and the Gaussian
log-probability of recorded actions, over the rows of a finished collection.  The library has no handle; a call is one argument
struct.  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C

from . import _binding
from ._binding import AtacomError, OK, E_INVALID, E_HIP, E_UNSUPPORTED, F32, F64  # noqa: F401
from ._lib import AtacomMlp

MAX_IN, MAX_OUT, HIDDEN, MAX_BLOCKS = 32, 8, 64, 65535


class View(C.Structure):
    _fields_ = [('ptr', C.c_void_p), ('stride_outer', C.c_int64), ('stride_inner', C.c_int64)]


class EvaluateArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_blocks', C.c_int32),
                ('n_outer', C.c_int64), ('n_inner', C.c_int64), ('net', AtacomMlp),
                ('x', View), ('action', View), ('y', View), ('logp', View), ('stream', C.c_void_p)]


def new_args(cls=EvaluateArgs):
    return _binding.new_args(cls)                     # the one call of this library: its struct is the default


_int = C.c_int
# {symbol: (restype, argtypes)}: every function of include/atacom_evaluate_hip.h
SIGNATURES = {
    'atacom_evaluate_version': (C.c_char_p, None),
    'atacom_evaluate_last_error': (C.c_char_p, None),
    'atacom_evaluate_mlp': (_int, [C.POINTER(EvaluateArgs)]),
}
EXPORTS = list(SIGNATURES)
LIB_PATH, load, check = _binding.library('evaluate', SIGNATURES)
