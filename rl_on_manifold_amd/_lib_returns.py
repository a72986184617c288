"""ctypes binding of libatacom_returns.so (include/atacom_returns_hip.h): advantages, their normalisation and episode returns of
a finished collection.  The library has no handle; a call is one argument struct.  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C

from . import _binding
from ._binding import AtacomError, OK, E_INVALID, E_HIP, E_UNSUPPORTED, F32, F64, new_args  # noqa: F401

FLAG_U8, FLAG_VALUE = 0, 1


def workspace_doubles(n_blocks, batch):
    """ATACOM_RETURNS_WORKSPACE_DOUBLES of the header."""
    return 3 * (int(n_blocks) * int(batch) + 256)


class View(C.Structure):
    _fields_ = [('ptr', C.c_void_p), ('stride_t', C.c_int64), ('stride_b', C.c_int64), ('stride_w', C.c_int64)]


class Shape(C.Structure):
    _fields_ = [('device', C.c_int32), ('dtype', C.c_int32), ('flag_dtype', C.c_int32), ('n_steps', C.c_int32),
                ('batch', C.c_int32), ('n_blocks', C.c_int32), ('d_sizes', C.c_void_p)]


class GaeArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('normalize', C.c_int32), ('shape', Shape), ('gamma', C.c_double), ('lam', C.c_double),
                ('reward', View), ('absorbing', View), ('last', View), ('v', View), ('v_next', View), ('ret', View), ('adv', View),
                ('d_workspace', C.c_void_p), ('d_stats', C.c_void_p), ('stream', C.c_void_p)]


class NormalizeArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('reserved', C.c_int32), ('shape', Shape), ('adv', View),
                ('d_workspace', C.c_void_p), ('d_stats', C.c_void_p), ('stream', C.c_void_p)]


class EpisodesArgs(C.Structure):
    _fields_ = [('struct_size', C.c_uint32), ('reserved', C.c_int32), ('shape', Shape), ('gamma', C.c_double),
                ('reward', View), ('last', View), ('d_workspace', C.c_void_p), ('d_result', C.c_void_p), ('stream', C.c_void_p)]


_int = C.c_int
# {symbol: (restype, argtypes)}: every function of include/atacom_returns_hip.h
SIGNATURES = {
    'atacom_returns_version': (C.c_char_p, None),
    'atacom_returns_last_error': (C.c_char_p, None),
    'atacom_returns_gae': (_int, [C.POINTER(GaeArgs)]),
    'atacom_returns_normalize': (_int, [C.POINTER(NormalizeArgs)]),
    'atacom_returns_episodes': (_int, [C.POINTER(EpisodesArgs)]),
}
EXPORTS = list(SIGNATURES)
LIB_PATH, load, check = _binding.library('returns', SIGNATURES)
