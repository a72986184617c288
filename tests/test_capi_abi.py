"""CPU-only checks of the drop-in boundary: the library builds for gfx950, loads, exports every symbol
include/atacom_hip.h declares, and its POD config agrees with the ctypes mirror and with the oracle's
constants.  No compute call is made (no GPU here)."""
import ctypes
import os
import re

import numpy as np

from oracle import atacom_scalar as osc

import abi_tools as abi
from abi_tools import ROOT


def test_library_exports_every_declared_symbol(lib_built):
    from rl_on_manifold_amd import _lib
    assert len(abi.one_symbol_set(lib_built, 'atacom_hip.h', 'atacom_', _lib)) >= 14
    assert _lib.load().atacom_version().startswith(b'atacom_hip')


def test_config_layout_and_reference_constants(lib_built):
    from rl_on_manifold_amd import _lib
    for env_id, spec in ((0, osc.circle_spec()), (1, osc.planar_spec()), (2, osc.iiwa_spec())):
        cfg = _lib.default_config(env_id)
        assert cfg.struct_size == ctypes.sizeof(_lib.AtacomConfig)
        d = _lib.get_dims(env_id)
        assert (d.dim_q, d.n_f, d.n_g, d.n_null, d.obs_dim) == (spec.dim_q, spec.n_f, spec.n_g, spec.n_null, spec.obs_dim)
        assert d.state_dim == 2 * spec.dim_q + spec.n_g + 10
        assert cfg.substeps == spec.substeps and cfg.horizon == spec.horizon and cfg.hold_q == int(spec.hold_q)
        assert abs(cfg.dt - spec.dt) < 1e-18 and cfg.rref_tol == spec.rref_tol
        assert np.allclose(list(cfg.K)[:spec.n_c], spec.K) and np.allclose(list(cfg.Kc)[:spec.n_c], spec.Kc)
        nq = spec.dim_q
        assert np.allclose(list(cfg.vel_max)[:nq], spec.vel_max) and np.allclose(list(cfg.acc_max)[:nq], spec.acc_max)
        assert np.allclose(list(cfg.Kq)[:nq], spec.Kq)
        assert np.allclose(list(cfg.base_xy), spec.base_xy)


def test_integration_doc_binding_stub_matches_the_struct():
    """INTEGRATION.md section 2 shows a maintainer the ctypes mirror of atacom_config: its field list must be the one
    of the shipped binding (it drifted once when dt_base was added)."""
    from rl_on_manifold_amd import _lib
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    body = doc[doc.index('class AtacomConfig(C.Structure)'):]
    body = body[:body.index(']\n\ncfg = AtacomConfig()')]
    assert re.findall(r'\("(\w+)", C\.', body) == [f[0] for f in _lib.AtacomConfig._fields_]


def test_error_reporting_without_gpu(lib_built):
    from rl_on_manifold_amd import _lib
    lib = _lib.load()
    cfg = _lib.AtacomConfig()
    assert lib.atacom_default_config(99, ctypes.byref(cfg)) == -1
    assert b'unknown env_id' in lib.atacom_last_error()
    d = _lib.AtacomDims()
    assert lib.atacom_get_dims(7, ctypes.byref(d)) == -1
    cfg = _lib.default_config(2)
    cfg.struct_size = 8
    h = ctypes.c_void_p()
    assert lib.atacom_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == -1
    assert b'struct_size' in lib.atacom_last_error()
    assert lib.atacom_step(None, None, None, None, None, None, None) == -1
    assert lib.atacom_destroy(None) == 0


def test_engine_refuses_to_run_without_gpu(lib_built):
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from rl_on_manifold_amd import BatchedAtacomEnv, AtacomError
    with pytest.raises(AtacomError):
        BatchedAtacomEnv('circle', 4)


def test_flop_model_is_consistent():
    import bench
    assert 45000 < bench.algorithmic_flops('iiwa') < 60000       # ~50 kFLOP / env-step
    assert bench.algorithmic_flops('circle') < bench.algorithmic_flops('planar') < bench.algorithmic_flops('iiwa')


def test_observation_bounds_follow_the_reference(lib_built, golden):
    """Drop-in detail: the MDPInfo of the iiwa env carries the finite bounds of env_single.py:69-80, with
    the joint limits of the reference's URDF (golden set G10), so MinMaxPreprocessor normalises what it normalises there."""
    import torch  # noqa: F401  (engine imports it)
    from rl_on_manifold_amd import _lib
    from rl_on_manifold_amd.engine import BatchedAtacomEnv
    g = golden('iiwa_urdf')
    lo, hi = BatchedAtacomEnv.observation_bounds(_lib.ENV_IIWA, _lib.default_config(_lib.ENV_IIWA))
    assert np.allclose(lo[:3], [-1, -0.5, -np.pi]) and np.allclose(hi[:3], [1, 0.5, np.pi])
    assert np.all(np.isinf(lo[3:6])) and np.all(np.isinf(hi[3:6]))
    assert np.allclose(hi[6:12], g['pos_upper'][:6]) and np.allclose(lo[6:12], -g['pos_upper'][:6])
    assert np.allclose(hi[12:18], g['vel_limit'][:6]) and np.allclose(lo[12:18], -g['vel_limit'][:6])
    lo, hi = BatchedAtacomEnv.observation_bounds(_lib.ENV_PLANAR, _lib.default_config(_lib.ENV_PLANAR))
    assert lo.shape == (12,) and np.isfinite(hi[[0, 1, 2, 6, 7, 8, 9, 10, 11]]).all()
    lo, hi = BatchedAtacomEnv.observation_bounds(_lib.ENV_CIRCLE, _lib.default_config(_lib.ENV_CIRCLE))
    assert np.all(np.isinf(lo)) and lo.shape == (4,)                                   # circle_base.py:21-22


def _build_c_consumer(lib_built, tmp_path):
    import subprocess
    exe = str(tmp_path / 'capi_demo')
    libdir = os.path.dirname(lib_built)
    cmd = ['gcc', '-std=c11', '-Wall', '-Werror', '-O2', '-D__HIP_PLATFORM_AMD__', os.path.join(ROOT, 'examples', 'capi_demo.c'),
           '-I' + os.path.join(ROOT, 'include'), '-I/opt/rocm/include', '-L' + libdir, '-latacom_hip', '-L/opt/rocm/lib',
           '-lamdhip64', '-lm', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib', '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_header_is_plain_c_and_a_c_program_links(lib_built, tmp_path):
    """The boundary is a C ABI: include/atacom_hip.h compiles as C11 with -Wall -Werror and a plain-C consumer
    (examples/capi_demo.c: no Python, no torch) links against the library."""
    assert os.path.exists(_build_c_consumer(lib_built, tmp_path))


import pytest  # noqa: E402


@pytest.mark.gpu
def test_plain_c_consumer_runs(lib_built, tmp_path):
    import subprocess
    exe = _build_c_consumer(lib_built, tmp_path)
    r = subprocess.run([exe, '2048', '120'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert 'c_max' in r.stdout
