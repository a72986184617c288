"""ctypes binding of libatacom_point.so (include/atacom_point_hip.h): the collision-avoidance task.  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C

from . import _binding
from ._binding import AtacomError, OK, E_INVALID, E_HIP, E_UNSUPPORTED, F32, F64  # noqa: F401


class AtacomPointConfig(C.Structure):
    """Mirror of `atacom_point_config` (include/atacom_point_hip.h)."""
    _fields_ = [('struct_size', C.c_int32), ('batch', C.c_int32), ('dtype', C.c_int32), ('n_objects', C.c_int32),
                ('random_walk', C.c_int32), ('horizon', C.c_int32), ('auto_reset', C.c_int32), ('seed', C.c_int32),
                ('dt', C.c_double), ('gamma', C.c_double)]


_vp, _i32, _int, _cfg = C.c_void_p, C.c_int32, C.c_int, C.POINTER(AtacomPointConfig)
# {symbol: (restype, argtypes)}: every function of include/atacom_point_hip.h
SIGNATURES = {
    'atacom_point_last_error': (C.c_char_p, None),
    'atacom_point_version': (C.c_char_p, None),
    'atacom_point_default_config': (_int, [_cfg]),
    'atacom_point_create': (_int, [_cfg, C.c_int, C.POINTER(_vp)]),
    'atacom_point_destroy': (_int, [_vp]),
    'atacom_point_reset': (_int, [_vp, _vp, _vp, _vp, _vp]),
    'atacom_point_step': (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'atacom_point_rollout': (_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'atacom_point_get_stats': (_int, [_vp, C.POINTER(C.c_double * 3), _i32, _vp]),
    'atacom_point_get_state': (_int, [_vp, _vp, _vp]),
    'atacom_point_set_state': (_int, [_vp, _vp, _vp]),
    'atacom_point_set_seed': (_int, [_vp, _i32]),
}
EXPORTS = list(SIGNATURES)
LIB_PATH, load, check = _binding.library('point', SIGNATURES)


def default_config():
    cfg = AtacomPointConfig()
    check(load().atacom_point_default_config(C.byref(cfg)))
    return cfg
