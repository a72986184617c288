"""ctypes binding of libatacom_point_policy.so (include/atacom_point_policy_hip.h): the collision-avoidance task's rollout
with the actor network evaluated in the kernel.  It works on the handles of libatacom_point.so (_lib_point) and takes the
network description of the main library (_lib.AtacomMlp).  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C
import os

from ._lib import AtacomError, AtacomMlp

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('ATACOM_POINT_POLICY_LIB') or os.path.join(HERE, 'libatacom_point_policy.so')

OK, E_INVALID, E_HIP, E_UNSUPPORTED = 0, -1, -2, -3

EXPORTS = ['atacom_point_policy_rollout', 'atacom_point_policy_rollout_packed', 'atacom_point_policy_last_error',
           'atacom_point_policy_version']

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
        raise AtacomError("libatacom_point_policy.so is not built (%s). Run `python -m rl_on_manifold_amd.build` -- "
                          "there is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int32
    lib.atacom_point_policy_rollout.argtypes = [vp, i32, C.POINTER(AtacomMlp), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.atacom_point_policy_rollout_packed.argtypes = [vp, i32, vp, C.POINTER(AtacomMlp), vp, vp, vp, i32, vp]
    lib.atacom_point_policy_last_error.restype = C.c_char_p
    lib.atacom_point_policy_version.restype = C.c_char_p
    lib.atacom_point_policy_rollout.restype = C.c_int
    lib.atacom_point_policy_rollout_packed.restype = C.c_int
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise AtacomError(load().atacom_point_policy_last_error().decode())
