"""ctypes binding of libatacom_evaluate.so (include/atacom_evaluate_hip.h): a critic or actor network, and the Gaussian
log-probability of recorded actions, over the rows of a finished collection.  The library has no handle; a call is one argument
struct.  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C
import os

from . import _binding
from ._binding import AtacomError  # noqa: F401
from ._lib import AtacomMlp

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('ATACOM_EVALUATE_LIB') or os.path.join(HERE, 'libatacom_evaluate.so')

OK, E_INVALID, E_HIP, E_UNSUPPORTED = 0, -1, -2, -3
F32, F64 = 0, 1
MAX_IN, MAX_OUT, HIDDEN, MAX_BLOCKS = 32, 8, 64, 65535


class View(C.Structure):
    _fields_ = [('ptr', C.c_void_p), ('stride_outer', C.c_int64), ('stride_inner', C.c_int64)]


class EvaluateArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_blocks', C.c_int32),
                ('n_outer', C.c_int64), ('n_inner', C.c_int64), ('net', AtacomMlp),
                ('x', View), ('action', View), ('y', View), ('logp', View), ('stream', C.c_void_p)]


def new_args(cls=EvaluateArgs):
    """A zeroed argument struct with its struct_size filled in."""
    a = cls()
    a.struct_size = C.sizeof(cls)
    return a


_int = C.c_int
# {symbol: (restype, argtypes)}: every function of include/atacom_evaluate_hip.h
SIGNATURES = {
    'atacom_evaluate_version': (C.c_char_p, None),
    'atacom_evaluate_last_error': (C.c_char_p, None),
    'atacom_evaluate_mlp': (_int, [C.POINTER(EvaluateArgs)]),
}
EXPORTS = list(SIGNATURES)


def load():
    """Load (once) and return the shared library with argtypes set.  Raises if it is not built."""
    return _binding.load(LIB_PATH, 'libatacom_evaluate.so', SIGNATURES)


check = _binding.checker(load, 'atacom_evaluate_last_error')
