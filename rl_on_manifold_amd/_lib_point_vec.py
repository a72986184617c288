"""ctypes binding of libatacom_point_vec.so (include/atacom_point_vec_hip.h): the collision-avoidance task's masked step and
its checkpoint.  It works on the handles of libatacom_point.so (_lib_point).  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C

from . import _binding
from ._binding import AtacomError, OK, E_INVALID, E_HIP, E_UNSUPPORTED  # noqa: F401

_vp, _i32, _i64, _int = C.c_void_p, C.c_int32, C.c_int64, C.c_int
# {symbol: (restype, argtypes)}: every function of include/atacom_point_vec_hip.h
SIGNATURES = {
    'atacom_point_vec_last_error': (C.c_char_p, None),
    'atacom_point_vec_version': (C.c_char_p, None),
    'atacom_point_vec_step_masked': (_int, [_vp] * 9),
    'atacom_point_vec_snapshot_bytes': (_i64, [_vp]),
    'atacom_point_vec_snapshot_save': (_int, [_vp, _vp, _vp]),
    'atacom_point_vec_snapshot_inspect': (_int, [_vp, _vp, C.POINTER(_i32), _vp]),
    'atacom_point_vec_snapshot_restore': (_int, [_vp, _vp, _vp]),
}
EXPORTS = list(SIGNATURES)
LIB_PATH, load, check = _binding.library('point_vec', SIGNATURES)
