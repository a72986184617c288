"""CPU-only checks of libatacom_point.so, the collision-avoidance task's own library: the header is plain C11, every
declared symbol is exported, the config mirror agrees, the kernels are exactly the {float, double} x {2, 4} set, the
float32 ones keep everything in registers (no scratch, no LDS outside the statistics reduction) and the exec-mask
audit finds nothing.  No compute call is made (no GPU here)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernel_resources import LLVM, _kernels        # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'atacom_point_hip.h')
FAMILIES = ('k_point_reset', 'k_point_step', 'k_point_rollout', 'k_point_stats', 'k_point_state_io')


@pytest.fixture(scope='module')
def point_lib():
    from rl_on_manifold_amd import build
    return build.build_point(verbose=False)


def _declared_functions():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(atacom_point_[a-z_]+)\s*\(', src)))


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "atacom_point_hip.h"\n'
                   'int main(void) { atacom_point_config c; c.struct_size = (int32_t)sizeof c; return c.struct_size == 0; }\n')
    subprocess.check_call(['gcc', '-std=c11', '-pedantic', '-Wall', '-Werror', '-I', os.path.dirname(HEADER), '-c', str(src),
                           '-o', str(tmp_path / 'use.o')])


def test_library_exports_every_declared_symbol(point_lib):
    from rl_on_manifold_amd import _lib_point
    names = _declared_functions()
    assert names == sorted(['atacom_point_' + n for n in (
        'default_config', 'create', 'destroy', 'reset', 'step', 'rollout', 'get_stats', 'get_state', 'set_state', 'set_seed',
        'version', 'last_error')])
    lib = ctypes.CDLL(point_lib)
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(_lib_point.EXPORTS) == names
    assert _lib_point.load().atacom_point_version().startswith(b'atacom_point')


def test_config_mirror_and_reference_defaults(point_lib):
    from rl_on_manifold_amd import _lib_point
    cfg = _lib_point.default_config()
    assert cfg.struct_size == ctypes.sizeof(_lib_point.AtacomPointConfig)
    # collision_avoidance_atacom.py:9: time_step=0.01, horizon=1000, gamma=0.99, n_objects=4, random_walk=False
    assert (cfg.dt, cfg.horizon, cfg.gamma, cfg.n_objects, cfg.random_walk) == (0.01, 1000, 0.99, 4, 0)
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = src[src.index('typedef struct atacom_point_config {'):src.index('} atacom_point_config;')]
    assert re.findall(r'\b(?:int32_t|double)\s+(\w+);', body) == [f[0] for f in _lib_point.AtacomPointConfig._fields_]
    assert _lib_point.AtacomPointConfig._fields_[0][0] == 'struct_size'


def test_errors_are_reported_without_a_gpu(point_lib):
    """Argument checks come before any device call: n_objects = 3 is E_UNSUPPORTED with a message, a stale struct_size
    E_INVALID, and the Python layer raises AtacomError."""
    from rl_on_manifold_amd import _lib_point, AtacomError
    lib = _lib_point.load()
    h = ctypes.c_void_p()
    cfg = _lib_point.default_config()
    cfg.n_objects = 3
    assert lib.atacom_point_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == _lib_point.E_UNSUPPORTED
    msg = lib.atacom_point_last_error().decode()
    assert 'n_objects = 3' in msg and '2 and 4' in msg
    assert not h.value
    cfg = _lib_point.default_config()
    cfg.struct_size -= 8
    assert lib.atacom_point_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == _lib_point.E_INVALID
    assert lib.atacom_point_step(None, None, None, None, None, None, None, None) == _lib_point.E_INVALID
    with pytest.raises(AtacomError):
        _lib_point.check(lib.atacom_point_get_state(None, None, None))


def test_package_exports_the_task():
    import rl_on_manifold_amd as pkg
    assert pkg.BatchedPointReachEnv.__name__ == 'BatchedPointReachEnv'
    assert pkg.PointReachAtacom.__name__ == 'PointReachAtacom'
    import inspect
    sig = inspect.signature(pkg.PointReachAtacom.__init__)
    ref = [('time_step', 0.01), ('horizon', 1000), ('gamma', 0.99), ('n_objects', 4), ('random_walk', False)]
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:6]] == ref
    assert 'host loop' in pkg.BatchedPointReachEnv.rollout_policy.__doc__.lower()


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, 'llvm-readelf')), reason='needs the ROCm LLVM binutils')
def test_kernel_census_and_register_residency(point_lib, tmp_path):
    ks = _kernels(str(tmp_path), so=point_lib)
    names = sorted(k[0].replace('atacom_point::', '') for k in ks)
    want = sorted('%s<%s, %d>' % (f, t, n) for f in FAMILIES for t in ('float', 'double') for n in (2, 4))
    assert names == want, names
    table = []
    for name, lds, scratch, vgpr, agpr, code in sorted(ks):
        name = name.replace('atacom_point::', '')
        table.append('%-34s VGPR %3d AGPR %2d scratch %d LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        if 'float' in name:
            assert scratch == 0, (name, scratch)
            assert lds == 0 or name.startswith('k_point_stats<'), (name, lds)
        assert scratch == 0, (name, scratch)         # the float64 instantiations fit as well
    print('\n'.join(table))


def test_exec_mask_audit_finds_nothing(point_lib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'profiles', 'tools', 'exec_restore_audit.py'), '--so', point_lib],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 copies' in r.stdout, r.stdout


def test_main_library_sources_do_not_include_the_task():
    """The main library's kernel census is pinned (tests/test_policy_kernel_resources.py): the task's units are not among
    its translation units, and nothing of csrc/ that it compiles includes them."""
    from rl_on_manifold_amd import build
    assert not any(u.startswith('atacom_point') for u in build.UNITS)
    assert build.UNITS_POINT == ['atacom_point.hip', 'atacom_point_capi.cpp']
    for f in os.listdir(build.CSRC):
        if not f.startswith('atacom_point'):
            assert 'atacom_point' not in open(os.path.join(build.CSRC, f)).read(), f
