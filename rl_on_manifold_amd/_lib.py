"""ctypes binding of libatacom_hip.so (include/atacom_hip.h).  No numerics here.

The library is the product: if it is missing or cannot be loaded this module raises -- there is no
CPU / PyTorch fallback anywhere in the package.
"""
import ctypes as C

from . import _binding
from ._binding import AtacomError, OK, E_INVALID, E_HIP, E_UNSUPPORTED, F32, F64  # noqa: F401

ENV_CIRCLE, ENV_PLANAR, ENV_IIWA, ENV_CIRCLE_EC, ENV_CIRCLE_T = 0, 1, 2, 3, 4
MAX_C, MAX_Q = 12, 6


class AtacomConfig(C.Structure):
    """Mirror of `atacom_config` (include/atacom_hip.h)."""
    _fields_ = [('struct_size', C.c_int32), ('env_id', C.c_int32), ('batch', C.c_int32), ('dtype', C.c_int32),
                ('substeps', C.c_int32), ('horizon', C.c_int32), ('hold_q', C.c_int32), ('bias_mode', C.c_int32),
                ('auto_reset', C.c_int32), ('lanes_per_env', C.c_int32),
                ('dt', C.c_double), ('rref_tol', C.c_double), ('action_penalty', C.c_double), ('gamma', C.c_double),
                ('K', C.c_double * MAX_C), ('Kc', C.c_double * MAX_C), ('vel_max', C.c_double * MAX_Q),
                ('acc_max', C.c_double * MAX_Q), ('Kq', C.c_double * MAX_Q), ('pos_limit', C.c_double * MAX_Q),
                ('base_xy', C.c_double * 2), ('link', C.c_double * 3), ('term_tol', C.c_double), ('random_init', C.c_int32), ('seed', C.c_int32),
                ('dynamics_mode', C.c_int32), ('chart_mode', C.c_int32), ('task', C.c_int32), ('reserved0', C.c_int32),
                ('dt_base', C.c_double),
                ('obs_noise', C.c_int32), ('obs_delay', C.c_int32), ('env_noise', C.c_int32), ('reserved1', C.c_int32),
                ('puck_mass', C.c_double)]


class AtacomMlp(C.Structure):
    """Mirror of `atacom_mlp` (include/atacom_hip.h)."""
    _fields_ = [('struct_size', C.c_int32), ('n_in', C.c_int32), ('hidden', C.c_int32), ('n_out', C.c_int32),
                ('activation', C.c_int32), ('reserved', C.c_int32),
                ('W1', C.c_void_p), ('b1', C.c_void_p), ('W2', C.c_void_p), ('b2', C.c_void_p),
                ('W3', C.c_void_p), ('b3', C.c_void_p), ('obs_shift', C.c_void_p), ('obs_scale', C.c_void_p),
                ('std', C.c_void_p),
                ('sW1', C.c_void_p), ('sb1', C.c_void_p), ('sW2', C.c_void_p), ('sb2', C.c_void_p),
                ('sW3', C.c_void_p), ('sb3', C.c_void_p), ('log_std_min', C.c_double), ('log_std_max', C.c_double),
                ('squash', C.c_int32), ('reserved1', C.c_int32),
                # appended (TD3 / DDPG): a struct_size of MLP_SIZE_V1 still selects the first release's layout
                ('mean_mode', C.c_int32), ('explore', C.c_int32), ('act_scale', C.c_void_p), ('act_low', C.c_void_p),
                ('act_high', C.c_void_p), ('ou_theta', C.c_double), ('ou_dt', C.c_double), ('ou_x0', C.c_void_p),
                ('ou_state', C.c_void_p)]


MLP_SIZE_V1 = AtacomMlp.mean_mode.offset          # ATACOM_MLP_SIZE_V1
EXPLORE_GAUSSIAN, EXPLORE_CLIPPED, EXPLORE_OU = 0, 1, 2


class AtacomDims(C.Structure):
    _fields_ = [('dim_q', C.c_int32), ('n_f', C.c_int32), ('n_g', C.c_int32), ('n_null', C.c_int32),
                ('obs_dim', C.c_int32), ('state_dim', C.c_int32), ('init_state_dim', C.c_int32),
                ('record_dim', C.c_int32)]


_vp, _i32, _u8p, _int = C.c_void_p, C.c_int32, C.c_void_p, C.c_int
_cfg, _mlp = C.POINTER(AtacomConfig), C.POINTER(AtacomMlp)
# {symbol: (restype, argtypes)}: every function of include/atacom_hip.h
SIGNATURES = {
    'atacom_last_error': (C.c_char_p, None),
    'atacom_version': (C.c_char_p, None),
    'atacom_default_config': (_int, [_i32, _cfg]),
    'atacom_get_dims': (_int, [_i32, C.POINTER(AtacomDims)]),
    'atacom_create': (_int, [_cfg, C.c_int, C.POINTER(_vp)]),
    'atacom_destroy': (_int, [_vp]),
    'atacom_reset': (_int, [_vp, _u8p, _vp, _vp, _vp]),
    'atacom_step': (_int, [_vp, _vp, _vp, _vp, _u8p, _u8p, _vp]),
    'atacom_step_masked': (_int, [_vp, _u8p, _vp, _vp, _vp, _u8p, _u8p, _vp]),
    'atacom_canonical_mu': (_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, C.c_double, _vp, _vp]),
    'atacom_rollout': (_int, [_vp, _i32, _vp, _vp, _vp, _vp, _u8p, _u8p, _vp]),
    'atacom_rollout_mlp': (_int, [_vp, _i32, _mlp, _vp, _vp, _vp, _vp, _vp, _u8p, _u8p, _vp]),
    'atacom_rollout_packed': (_int, [_vp, _i32, _vp, _mlp, _vp, _vp, _i32, _vp]),
    'atacom_rollout_compact': (_int, [_vp, _i32, _vp, _mlp, _vp, _vp, _i32, _vp, _i32, _vp, _vp]),
    'atacom_get_stats': (_int, [_vp, C.POINTER(C.c_double * 3), _i32, _vp]),
    'atacom_get_lanes': (_int, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    'atacom_get_policy_lanes': (_int, [_vp, C.POINTER(_i32)]),
    'atacom_set_seed': (_int, [_vp, _i32]),
    'atacom_get_state': (_int, [_vp, _vp, _vp]),
    'atacom_set_state': (_int, [_vp, _vp, _vp]),
    'atacom_get_aux_state': (_int, [_vp, _vp, _vp]),
    'atacom_set_aux_state': (_int, [_vp, _vp, _vp]),
    'atacom_get_filter_state': (_int, [_vp, _vp, _vp]),
    'atacom_set_filter_state': (_int, [_vp, _vp, _vp]),
    'atacom_snapshot_bytes': (C.c_int64, [_vp]),
    'atacom_snapshot_save': (_int, [_vp, _vp, _vp]),
    'atacom_snapshot_restore': (_int, [_vp, _vp, _vp]),
    'atacom_inverse_dynamics': (_int, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    'atacom_forward_dynamics': (_int, [_i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    'atacom_nullspace': (_int, [_i32, _i32, _i32, _i32, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp]),
    'atacom_constraint_terms': (_int, [_cfg, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
}
EXPORTS = list(SIGNATURES)
LIB_PATH, load, check = _binding.library('hip', SIGNATURES)


def default_config(env_id):
    cfg = AtacomConfig()
    check(load().atacom_default_config(env_id, C.byref(cfg)))
    return cfg


def get_dims(env_id):
    d = AtacomDims()
    check(load().atacom_get_dims(env_id, C.byref(d)))
    return d
