"""CPU-only checks of libatacom_point.so, the collision-avoidance task's own library: the header is plain C11, the declared
symbols are exactly the exported ones and the ctypes table, the config mirror agrees, the kernels are exactly the
{float, double} x {2, 4} set, the float32 ones keep everything in registers (no scratch, no LDS outside the statistics
reduction) and the exec-mask audit finds nothing.  No compute call is made (no GPU here)."""
import ctypes
import inspect
import os
import re

import pytest

import abi_tools as abi

HEADER = 'atacom_point_hip.h'
FAMILIES = ('k_point_reset', 'k_point_step', 'k_point_rollout', 'k_point_stats', 'k_point_state_io')


@pytest.fixture(scope='module')
def point_lib():
    from rl_on_manifold_amd import build
    return build.build('point', verbose=False)


def test_header_is_plain_c11(tmp_path):
    abi.compile_c11(tmp_path, abi.INCLUDE, '#include "atacom_point_hip.h"\n'
                    'int main(void) { atacom_point_config c; c.struct_size = (int32_t)sizeof c; return c.struct_size == 0; }\n')


def test_library_exports_every_declared_symbol(point_lib):
    from rl_on_manifold_amd import _lib_point
    names = abi.one_symbol_set(point_lib, HEADER, 'atacom_point_', _lib_point)
    assert names == sorted(['atacom_point_' + n for n in (
        'default_config', 'create', 'destroy', 'reset', 'step', 'rollout', 'get_stats', 'get_state', 'set_state', 'set_seed',
        'version', 'last_error')])
    assert _lib_point.load().atacom_point_version().startswith(b'atacom_point')


def test_config_mirror_and_reference_defaults(point_lib):
    from rl_on_manifold_amd import _lib_point
    cfg = _lib_point.default_config()
    assert cfg.struct_size == ctypes.sizeof(_lib_point.AtacomPointConfig)
    # collision_avoidance_atacom.py:9: time_step=0.01, horizon=1000, gamma=0.99, n_objects=4, random_walk=False
    assert (cfg.dt, cfg.horizon, cfg.gamma, cfg.n_objects, cfg.random_walk) == (0.01, 1000, 0.99, 4, 0)
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(abi.INCLUDE, HEADER)).read(), flags=re.S)
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
    sig = inspect.signature(pkg.PointReachAtacom.__init__)
    ref = [('time_step', 0.01), ('horizon', 1000), ('gamma', 0.99), ('n_objects', 4), ('random_walk', False)]
    assert [(k, v.default) for k, v in list(sig.parameters.items())[1:6]] == ref
    assert 'host loop' in pkg.BatchedPointReachEnv.rollout_policy.__doc__.lower()


@abi.needs_llvm('llvm-readelf')
def test_kernel_census_and_register_residency(point_lib, tmp_path):
    ks = abi.kernel_rows(point_lib, tmp_path)
    want = sorted('%s<%s, %d>' % (f, t, n) for f in FAMILIES for t in ('float', 'double') for n in (2, 4))
    assert [k[0] for k in ks] == want, ks
    for name, lds, scratch, vgpr, agpr, code in ks:
        print('%-34s VGPR %3d AGPR %2d scratch %d LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        assert scratch == 0, (name, scratch)         # the float64 instantiations fit as well
        if 'float' in name:
            assert lds == 0 or name.startswith('k_point_stats<'), (name, lds)


def test_exec_mask_audit_finds_nothing(point_lib):
    abi.exec_audit(point_lib)
