"""CPU-only checks of libatacom_point_vec.so, the collision-avoidance task's masked step and checkpoint: the header is plain
C11, the declared symbols are exactly the exported ones and the ctypes table, the kernels are exactly
k_point_step_masked<{float, double}, {2, 4}> and k_point_snapshot_copy<{false, true}>, the masked kernels use no scratch (and the
float32 ones no LDS), the exec-mask audit finds nothing, handles are refused before anything of them is used, and the image size
is the documented formula.  No compute call is made (no GPU here)."""
import ctypes
import inspect
import os

import pytest

import abi_tools as abi

FUNCTIONS = ('step_masked', 'snapshot_bytes', 'snapshot_save', 'snapshot_inspect', 'snapshot_restore', 'last_error', 'version')
HANDLE_MAGIC = 0x41505401            # csrc/atacom_point_handle.h: kHandleMagic


@pytest.fixture(scope='module')
def vec_lib():
    from rl_on_manifold_amd import build
    build.build('point', verbose=False)
    return build.build('point_vec', verbose=False)


def test_header_is_plain_c11(tmp_path):
    abi.compile_c11(tmp_path, abi.INCLUDE, '#include "atacom_point_vec_hip.h"\n'
                    'int main(void) { int32_t seed = 0; uint8_t flag = 0;\n'
                    '    if (atacom_point_vec_snapshot_bytes(0) > 0) return 1;\n'
                    '    if (atacom_point_vec_snapshot_save(0, 0, 0) == ATACOM_POINT_OK) return 2;\n'
                    '    if (atacom_point_vec_snapshot_inspect(0, 0, &seed, 0) == ATACOM_POINT_OK) return 3;\n'
                    '    if (atacom_point_vec_snapshot_restore(0, 0, 0) == ATACOM_POINT_OK) return 4;\n'
                    '    return atacom_point_vec_step_masked(0, &flag, 0, 0, 0, 0, &flag, 0, 0) == ATACOM_POINT_OK; }\n')


def test_declared_exported_and_bound_symbols_are_one_set(vec_lib):
    from rl_on_manifold_amd import _lib_point_vec
    names = abi.one_symbol_set(vec_lib, 'atacom_point_vec_hip.h', 'atacom_point_vec_', _lib_point_vec)
    assert names == sorted('atacom_point_vec_' + n for n in FUNCTIONS)
    assert _lib_point_vec.load().atacom_point_vec_version().startswith(b'atacom_point_vec')


@abi.needs_llvm('llvm-readelf')
def test_kernel_census_and_resources(vec_lib, tmp_path):
    from rl_on_manifold_amd import build
    os.makedirs(str(tmp_path / 'vec'))
    ks = abi.kernel_rows(vec_lib, tmp_path / 'vec')
    assert [k[0] for k in ks] == sorted(['k_point_step_masked<%s, %d>' % (t, n) for t in ('float', 'double') for n in (2, 4)] +
                                        ['k_point_snapshot_copy<%s>' % d for d in ('false', 'true')]), ks
    # next to them, not pinned: the plain step of the same build (libatacom_point.so), which a masked-in lane repeats
    os.makedirs(str(tmp_path / 'point'))
    plain = [k for k in abi.kernel_rows(build.build('point', verbose=False), tmp_path / 'point') if k[0].startswith('k_point_step<')]
    for name, lds, scratch, vgpr, agpr, code in ks + plain:
        print('%-34s VGPR %3d AGPR %2d scratch %d LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
    for name, lds, scratch, vgpr, agpr, code in ks:
        assert scratch == 0, (name, scratch)         # everything in registers, the float64 instantiations as well
        assert lds == 0, (name, lds)


def test_exec_mask_audit_finds_nothing(vec_lib):
    """The masked kernel is a block of stores under a narrowed exec mask (the lanes that sit out) in front of the step's large
    register footprint: the shape in which the compiler defect of DESIGN.md section 9 was met."""
    abi.exec_audit(vec_lib)


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
