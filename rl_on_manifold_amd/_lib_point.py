"""ctypes binding of libatacom_point.so (include/atacom_point_hip.h): the collision-avoidance task.  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C
import os

from ._lib import AtacomError

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('ATACOM_POINT_LIB') or os.path.join(HERE, 'libatacom_point.so')

F32, F64 = 0, 1
OK, E_INVALID, E_HIP, E_UNSUPPORTED = 0, -1, -2, -3

EXPORTS = ['atacom_point_default_config', 'atacom_point_create', 'atacom_point_destroy', 'atacom_point_reset',
           'atacom_point_step', 'atacom_point_rollout', 'atacom_point_get_stats', 'atacom_point_get_state',
           'atacom_point_set_state', 'atacom_point_set_seed', 'atacom_point_last_error', 'atacom_point_version']


class AtacomPointConfig(C.Structure):
    """Mirror of `atacom_point_config` (include/atacom_point_hip.h)."""
    _fields_ = [('struct_size', C.c_int32), ('batch', C.c_int32), ('dtype', C.c_int32), ('n_objects', C.c_int32),
                ('random_walk', C.c_int32), ('horizon', C.c_int32), ('auto_reset', C.c_int32), ('seed', C.c_int32),
                ('dt', C.c_double), ('gamma', C.c_double)]


_lib = None


def load():
    """Load (once) and return the shared library with argtypes set.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    try:                      # one HIP runtime per process: PyTorch's, when it is there (see _lib.load)
        import torch  # noqa: F401
    except Exception:  # noqa: BLE001
        pass
    if not os.path.exists(LIB_PATH):
        raise AtacomError("libatacom_point.so is not built (%s). Run `python -m rl_on_manifold_amd.build` -- "
                          "there is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int32
    lib.atacom_point_default_config.argtypes = [C.POINTER(AtacomPointConfig)]
    lib.atacom_point_create.argtypes = [C.POINTER(AtacomPointConfig), C.c_int, C.POINTER(vp)]
    lib.atacom_point_destroy.argtypes = [vp]
    lib.atacom_point_reset.argtypes = [vp, vp, vp, vp, vp]
    lib.atacom_point_step.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.atacom_point_rollout.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.atacom_point_get_stats.argtypes = [vp, C.POINTER(C.c_double * 3), i32, vp]
    lib.atacom_point_get_state.argtypes = [vp, vp, vp]
    lib.atacom_point_set_state.argtypes = [vp, vp, vp]
    lib.atacom_point_set_seed.argtypes = [vp, i32]
    lib.atacom_point_last_error.restype = C.c_char_p
    lib.atacom_point_version.restype = C.c_char_p
    for name in EXPORTS:
        if name not in ('atacom_point_last_error', 'atacom_point_version'):
            getattr(lib, name).restype = C.c_int
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise AtacomError(load().atacom_point_last_error().decode())


def default_config():
    cfg = AtacomPointConfig()
    check(load().atacom_point_default_config(C.byref(cfg)))
    return cfg
