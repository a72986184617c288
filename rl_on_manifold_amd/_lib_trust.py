"""ctypes binding of libatacom_trust.so (include/atacom_trust_hip.h): the product of a policy's Fisher matrix with a vector over
the rows of a finished collection, the repeated stage of a trust-region policy step.  The library has no handle; a call is one
argument struct.  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C

from . import _binding
from ._binding import AtacomError, OK, E_INVALID, E_HIP, E_UNSUPPORTED, F32, F64  # noqa: F401
from ._lib import AtacomMlp
from ._lib_evaluate import View

MAX_IN, MAX_OUT, HIDDEN, MAX_BLOCKS = 32, 8, 64, 65535


class TrustArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('device', C.c_int32), ('dtype', C.c_int32), ('n_blocks', C.c_int32),
                ('n_outer', C.c_int64), ('n_inner', C.c_int64), ('net', AtacomMlp), ('x', View), ('idx', C.c_void_p),
                ('n_idx', C.c_int64), ('v', C.c_void_p), ('damping', C.c_double), ('out', C.c_void_p), ('workspace', C.c_void_p),
                ('workspace_bytes', C.c_size_t), ('stream', C.c_void_p)]


def new_args(cls=TrustArgs):
    return _binding.new_args(cls)                     # the one struct of this library is the default


def net_size(n_in, n_out):
    """P: the values of the network part of a direction."""
    return 64 * n_in + 64 + 4096 + 64 + 64 * n_out + n_out


def size(n_in, n_out):
    """The values of `v` and of `out`: P, and n_out more for log std."""
    return net_size(n_in, n_out) + n_out


_int = C.c_int
# {symbol: (restype, argtypes)}: every function of include/atacom_trust_hip.h
SIGNATURES = {
    'atacom_trust_version': (C.c_char_p, None),
    'atacom_trust_last_error': (C.c_char_p, None),
    'atacom_trust_workspace_size': (C.c_size_t, [C.POINTER(TrustArgs)]),
    'atacom_trust_fvp': (_int, [C.POINTER(TrustArgs)]),
}
EXPORTS = list(SIGNATURES)
LIB_PATH, load, check = _binding.library('trust', SIGNATURES)
