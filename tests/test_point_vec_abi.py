"""CPU-only checks of libatacom_point_vec.so, the collision-avoidance task's masked step and checkpoint: the header is plain
C11, the declared symbols are exactly the exported ones and the ctypes table, the kernels are exactly
k_point_step_masked<{float, double}, {2, 4}> and k_point_snapshot_copy<{false, true}>, the masked kernels use no scratch (and the
float32 ones no LDS), the exec-mask audit finds nothing, handles are refused before anything of them is used, the image size is
the documented formula, and the other four libraries' unit lists are untouched.  No compute call is made (no GPU here)."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernel_resources import LLVM, _kernels        # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'atacom_point_vec_hip.h')
OWN = {'atacom_point_vec.hip', 'atacom_point_vec_capi.cpp', 'atacom_point_vec.h', 'atacom_point_vec_ops.h'}
FUNCTIONS = ('step_masked', 'snapshot_bytes', 'snapshot_save', 'snapshot_inspect', 'snapshot_restore', 'last_error', 'version')
HANDLE_MAGIC = 0x41505401            # csrc/atacom_point_handle.h: kHandleMagic


@pytest.fixture(scope='module')
def vec_lib():
    from rl_on_manifold_amd import build
    build.build_point(verbose=False)
    return build.build_point_vec(verbose=False)


def _declared_functions():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(atacom_point_vec_[a-z_]+)\s*\(', src)))


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "atacom_point_vec_hip.h"\n'
                   'int main(void) { int32_t seed = 0; uint8_t flag = 0;\n'
                   '    if (atacom_point_vec_snapshot_bytes(0) > 0) return 1;\n'
                   '    if (atacom_point_vec_snapshot_save(0, 0, 0) == ATACOM_POINT_OK) return 2;\n'
                   '    if (atacom_point_vec_snapshot_inspect(0, 0, &seed, 0) == ATACOM_POINT_OK) return 3;\n'
                   '    if (atacom_point_vec_snapshot_restore(0, 0, 0) == ATACOM_POINT_OK) return 4;\n'
                   '    return atacom_point_vec_step_masked(0, &flag, 0, 0, 0, 0, &flag, 0, 0) == ATACOM_POINT_OK; }\n')
    subprocess.check_call(['gcc', '-std=c11', '-pedantic', '-Wall', '-Werror', '-I', os.path.dirname(HEADER), '-c', str(src),
                           '-o', str(tmp_path / 'use.o')])


def test_declared_exported_and_bound_symbols_are_one_set(vec_lib):
    from rl_on_manifold_amd import _lib_point_vec
    names = _declared_functions()
    assert names == sorted('atacom_point_vec_' + n for n in FUNCTIONS)
    nm = os.path.join(LLVM, 'llvm-nm')
    out = subprocess.run([nm if os.path.exists(nm) else 'nm', '-D', '--defined-only', vec_lib], capture_output=True,
                         text=True, check=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith('atacom_'))
    assert exported == names, exported
    assert sorted(_lib_point_vec.EXPORTS) == names
    assert _lib_point_vec.load().atacom_point_vec_version().startswith(b'atacom_point_vec')


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, 'llvm-readelf')), reason='needs the ROCm LLVM binutils')
def test_kernel_census_and_resources(vec_lib, tmp_path):
    from rl_on_manifold_amd import build
    os.makedirs(str(tmp_path / 'vec'))
    ks = _kernels(str(tmp_path / 'vec'), so=vec_lib)
    names = sorted(k[0].replace('atacom_point::', '') for k in ks)
    assert names == sorted(['k_point_step_masked<%s, %d>' % (t, n) for t in ('float', 'double') for n in (2, 4)] +
                           ['k_point_snapshot_copy<%s>' % d for d in ('false', 'true')]), names
    table = []
    for name, lds, scratch, vgpr, agpr, code in sorted(ks):
        name = name.replace('atacom_point::', '')
        table.append('%-34s VGPR %3d AGPR %2d scratch %d LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        assert scratch == 0, (name, scratch)         # everything in registers, the float64 instantiations as well
        assert lds == 0, (name, lds)
    # next to them, not pinned: the plain step of the same build (libatacom_point.so), which a masked-in lane repeats
    os.makedirs(str(tmp_path / 'point'))
    for name, lds, scratch, vgpr, agpr, code in sorted(_kernels(str(tmp_path / 'point'), so=build.build_point(verbose=False))):
        name = name.replace('atacom_point::', '')
        if name.startswith('k_point_step<'):
            table.append('%-34s VGPR %3d AGPR %2d scratch %d LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
    print('\n'.join(table))


def test_exec_mask_audit_finds_nothing(vec_lib):
    """The masked kernel is a block of stores under a narrowed exec mask (the lanes that sit out) in front of the step's large
    register footprint: the shape in which the compiler defect of DESIGN.md section 9 was met."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'profiles', 'tools', 'exec_restore_audit.py'), '--so', vec_lib],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 copies' in r.stdout, r.stdout


def _fake_handle(magic, **cfg):
    """The head of csrc/atacom_point_handle.h -- the layout number, then the configuration -- with no device memory behind it."""
    from rl_on_manifold_amd import _lib_point
    c = _lib_point.default_config()
    for k, v in cfg.items():
        setattr(c, k, v)

    class Handle(ctypes.Structure):
        _fields_ = [('magic', ctypes.c_uint32), ('cfg', type(c)), ('rest', ctypes.c_void_p * 6)]
    h = Handle()
    h.magic, h.cfg = magic, c
    return h


def _snapshot_bytes(batch, n_objects, elem):
    count = 4 * (1 + n_objects) + n_objects + 2 * n_objects + 1 + 2        # csrc/atacom_point.h: Layout<N>::COUNT
    groups = (count + 3) // 4
    return 64 + groups * batch * 4 * elem + batch * 4 * 4


def test_arguments_are_validated_without_a_gpu(vec_lib):
    from rl_on_manifold_amd import _lib_point, _lib_point_vec as lv, AtacomError
    _lib_point.load()
    lib = lv.load()
    p = ctypes.c_void_p(0x1000)                      # never dereferenced
    seed = ctypes.c_int32(0)

    def msg():
        return lib.atacom_point_vec_last_error().decode()

    def every_call(h):
        return [lib.atacom_point_vec_step_masked(h, p, p, None, p, p, p, p, None),
                int(lib.atacom_point_vec_snapshot_bytes(h)),
                lib.atacom_point_vec_snapshot_save(h, p, None),
                lib.atacom_point_vec_snapshot_inspect(h, p, ctypes.byref(seed), None),
                lib.atacom_point_vec_snapshot_restore(h, p, None)]

    assert every_call(None) == [lv.E_INVALID] * 5 and 'null handle' in msg()
    fake = ctypes.create_string_buffer(256)          # not a handle: no magic number
    assert every_call(ctypes.cast(fake, ctypes.c_void_p)) == [lv.E_INVALID] * 5 and 'not a live handle' in msg()
    stale = _fake_handle(HANDLE_MAGIC + 1)
    assert every_call(ctypes.addressof(stale)) == [lv.E_INVALID] * 5 and 'layout number' in msg()
    # a handle with the right layout number and no device memory behind it: the checks that precede every device call
    h = _fake_handle(HANDLE_MAGIC)
    ha = ctypes.addressof(h)
    assert lib.atacom_point_vec_step_masked(ha, None, None, None, p, p, p, None, None) == lv.E_INVALID and 'null argument' in msg()
    assert lib.atacom_point_vec_step_masked(ha, None, p, None, ctypes.c_void_p(0x1004), p, p, None, None) == lv.E_INVALID
    assert 'four elements' in msg()
    for fn in (lib.atacom_point_vec_snapshot_save, lib.atacom_point_vec_snapshot_restore):
        assert fn(ha, None, None) == lv.E_INVALID and 'null argument' in msg()
        assert fn(ha, ctypes.c_void_p(0x1008), None) == lv.E_INVALID and '16 bytes' in msg()
    assert lib.atacom_point_vec_snapshot_inspect(ha, None, None, None) == lv.E_INVALID and 'null argument' in msg()
    # the size of an image: the default configuration (batch 1, float32, 4 obstacles), then the other shapes
    assert int(lib.atacom_point_vec_snapshot_bytes(ha)) == _snapshot_bytes(1, 4, 4) == 64 + 9 * 16 + 16
    for batch, n, dtype, elem in ((333, 2, _lib_point.F32, 4), (333, 4, _lib_point.F64, 8), (1 << 20, 4, _lib_point.F32, 4),
                                  (1 << 27, 4, _lib_point.F64, 8)):
        hh = _fake_handle(HANDLE_MAGIC, batch=batch, n_objects=n, dtype=dtype)
        assert int(lib.atacom_point_vec_snapshot_bytes(ctypes.addressof(hh))) == _snapshot_bytes(batch, n, elem)
    odd = _fake_handle(HANDLE_MAGIC, n_objects=3)
    assert int(lib.atacom_point_vec_snapshot_bytes(ctypes.addressof(odd))) == lv.E_UNSUPPORTED and 'n_objects = 3' in msg()
    assert lib.atacom_point_vec_snapshot_save(ctypes.addressof(odd), p, None) == lv.E_UNSUPPORTED
    with pytest.raises(AtacomError):
        lv.check(lib.atacom_point_vec_snapshot_save(None, p, None))


def test_the_other_libraries_units_are_unchanged():
    from rl_on_manifold_amd import build
    assert build.UNITS_POINT == ['atacom_point.hip', 'atacom_point_capi.cpp']
    assert len(build.UNITS) == 14 and build.UNITS[-1] == 'atacom_capi.cpp'
    assert build.UNITS_POINT_POLICY == ['atacom_point_policy.hip', 'atacom_point_policy_capi.cpp']
    assert build.UNITS_POINT_COMPACT == ['atacom_point_compact.hip', 'atacom_point_compact_capi.cpp']
    assert build.UNITS_POINT_VEC == ['atacom_point_vec.hip', 'atacom_point_vec_capi.cpp']
    assert [t.feeds for t in (build.TARGETS[k] for k in ('hip', 'point', 'point_policy', 'point_compact', 'point_vec'))] == \
        [(), (), ('point',), ('point', 'point_policy'), ('point',)]
    assert list(build.TARGETS) == ['hip', 'point', 'point_policy', 'point_compact', 'point_vec']
    # editing the new files makes none of the other four libraries stale
    for srcs in (build._sources(), build._sources_point(), build._sources_point_policy(), build._sources_point_compact()):
        assert not OWN & {os.path.basename(p) for p in srcs}
        assert not any(p.endswith('atacom_point_vec_hip.h') for p in srcs)
    mine = {os.path.basename(p) for p in build._sources_point_vec()}
    # ... what it borrows makes it stale (the handle, the environment), and the policy and compact libraries' headers do not
    assert OWN | {'atacom_point_handle.h', 'atacom_point.h', 'atacom_point_hip.h', 'atacom_point_vec_hip.h', 'atacom_kernels.h'} <= mine
    assert not {'atacom_point_policy.h', 'atacom_point_policy_ops.h', 'atacom_point_compact.h', 'atacom_point_compact_ops.h'} & mine


def test_a_touched_header_makes_exactly_the_libraries_that_include_it_stale(monkeypatch):
    """The staleness rule of build.py with the fifth target in the table, on faked modification times."""
    from rl_on_manifold_amd import build
    libs = (build.LIB, build.LIB_POINT, build.LIB_POINT_POLICY, build.LIB_POINT_COMPACT, build.LIB_POINT_VEC)
    touched = []
    real_exists = os.path.exists
    monkeypatch.setattr(build.os.path, 'exists', lambda p: p in libs or real_exists(p))
    monkeypatch.setattr(build.os.path, 'getmtime', lambda p: 2.0 if os.path.basename(p) in touched else 1.0)

    def stale():
        return [build.needs_build(), build.needs_build_point(), build.needs_build_point_policy(), build.needs_build_point_compact(),
                build.needs_build_point_vec()]

    assert stale() == [False] * 5
    for header, want in (('atacom_point_vec.h', [False, False, False, False, True]),
                         ('atacom_point_vec_ops.h', [False, False, False, False, True]),
                         ('atacom_point_vec_hip.h', [False, False, False, False, True]),
                         ('atacom_point_vec.hip', [False, False, False, False, True]),
                         ('atacom_point_vec_capi.cpp', [False, False, False, False, True]),
                         ('atacom_point_compact.h', [False, False, False, True, False]),
                         ('atacom_point_policy.h', [False, False, True, True, False]),
                         ('atacom_point.h', [False, True, True, True, True]), ('atacom_point_handle.h', [False, True, True, True, True]),
                         ('atacom_point_hip.h', [False, True, True, True, True]),
                         ('atacom_kernels.h', [True, True, True, True, True])):
        touched[:] = [header]
        assert stale() == want, header
        assert os.path.exists(os.path.join(build.CSRC, header)) or os.path.exists(os.path.join(ROOT, 'include', header)), header


def test_python_surface():
    import rl_on_manifold_amd as pkg
    point, main = pkg.BatchedPointReachEnv, pkg.BatchedAtacomEnv
    assert list(inspect.signature(point.step).parameters)[1:] == ['actions', 'draws', 'mask']
    assert list(inspect.signature(point.step_into).parameters)[1:] == ['actions', 'obs', 'reward', 'absorbing', 'last', 'draws', 'mask']
    for name in ('snapshot', 'restore', 'observe_into'):
        assert list(inspect.signature(getattr(point, name)).parameters) == list(inspect.signature(getattr(main, name)).parameters)
    vec, ref = pkg.VectorizedPointReachEnv, pkg.VectorizedAtacomEnv
    for name in ('info', 'engine', 'seed', 'reset_all', 'step_all', 'render_all', 'stop', 'get_constraints_logs'):
        assert hasattr(vec, name) and hasattr(ref, name), name
    assert list(inspect.signature(vec.reset_all).parameters)[1:] == ['env_mask', 'draws']
    assert list(inspect.signature(vec.step_all).parameters)[1:] == ['env_mask', 'action', 'draws']
    # one mask normalisation, used by both vectorised surfaces
    from rl_on_manifold_amd import _device_env
    for cls in (vec, ref):
        assert 'device_mask' in cls._mask.__code__.co_names
    import torch
    m = _device_env.device_mask([1, 0, 2], 'cpu', 3)
    assert m.dtype == torch.uint8 and m.tolist() == [1, 0, 1]
    assert _device_env.device_mask(torch.tensor([True, False, True]), 'cpu', 3).tolist() == [1, 0, 1]
    assert _device_env.device_mask(None, 'cpu', 3) is None
    with pytest.raises(ValueError):
        _device_env.device_mask([1, 0], 'cpu', 3)
