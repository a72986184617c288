"""ctypes binding of libatacom_point_policy.so (include/atacom_point_policy_hip.h): the collision-avoidance task's rollout
with the actor network evaluated in the kernel.  It works on the handles of libatacom_point.so (_lib_point) and takes the
network description of the main library (_lib.AtacomMlp).  No numerics here.

Like _lib.py: if the library is missing or cannot be loaded this module raises -- there is no CPU / PyTorch fallback.
"""
import ctypes as C

from . import _binding
from ._binding import AtacomError, OK, E_INVALID, E_HIP, E_UNSUPPORTED  # noqa: F401
from ._lib import AtacomMlp

_vp, _i32, _int, _mlp = C.c_void_p, C.c_int32, C.c_int, C.POINTER(AtacomMlp)
# {symbol: (restype, argtypes)}: every function of include/atacom_point_policy_hip.h
SIGNATURES = {
    'atacom_point_policy_last_error': (C.c_char_p, None),
    'atacom_point_policy_version': (C.c_char_p, None),
    'atacom_point_policy_rollout': (_int, [_vp, _i32, _mlp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'atacom_point_policy_rollout_packed': (_int, [_vp, _i32, _vp, _mlp, _vp, _vp, _vp, _i32, _vp]),
}
EXPORTS = list(SIGNATURES)
LIB_PATH, load, check = _binding.library('point_policy', SIGNATURES)
