"""CPU-only checks of libatacom_point_compact.so, the collision-avoidance task's rollout in the compact record format: the
header is plain C11, the declared symbols are exactly the exported ones and the ctypes table, the kernels are exactly
k_point_rollout_compact<{float, double}, {2, 4}, {false, true}>, the float32 ones use no scratch and the ones with
pre-generated actions no LDS, the exec-mask audit finds nothing, and arguments are validated before any device call.
No compute call is made (no GPU here)."""
import ctypes
import inspect
import re

import pytest

import abi_tools as abi
from abi_tools import fake_mlp as _mlp


@pytest.fixture(scope='module')
def compact_lib():
    from rl_on_manifold_amd import build
    build.build('point', verbose=False)
    return build.build('point_compact', verbose=False)


def test_header_is_plain_c11(tmp_path):
    abi.compile_c11(tmp_path, abi.INCLUDE, '#include "atacom_point_compact_hip.h"\n'
                    'int main(void) { atacom_mlp m; int32_t n = 0; m.struct_size = (int32_t)sizeof m;\n'
                    '    return atacom_point_compact_rollout(0, 1, 0, &m, 0, 0, 0, 1, 0, 0, &n, 0) == ATACOM_POINT_OK; }\n')


def test_declared_exported_and_bound_symbols_are_one_set(compact_lib):
    from rl_on_manifold_amd import _lib_point_compact
    names = abi.one_symbol_set(compact_lib, 'atacom_point_compact_hip.h', 'atacom_point_compact_', _lib_point_compact)
    assert names == sorted('atacom_point_compact_' + n for n in ('rollout', 'last_error', 'version'))
    assert _lib_point_compact.load().atacom_point_compact_version().startswith(b'atacom_point_compact')


@abi.needs_llvm('llvm-readelf')
def test_kernel_census_and_resources(compact_lib, tmp_path):
    ks = abi.kernel_rows(compact_lib, tmp_path)
    assert [k[0] for k in ks] == sorted('k_point_rollout_compact<%s, %d, %s>' % (t, n, p) for t in ('float', 'double') for n in (2, 4)
                                        for p in ('false', 'true')), ks
    for name, lds, scratch, vgpr, agpr, code in ks:
        print('%-46s VGPR %3d AGPR %3d scratch %d static LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        assert lds == 0, (name, lds)                 # the network's LDS is dynamic (sized by the launcher); none otherwise
        if 'float' in name:
            assert scratch == 0, (name, scratch)     # everything in registers
            assert vgpr <= 512


@abi.needs_llvm('llvm-objdump')
def test_kernels_with_pregenerated_actions_use_no_lds_and_no_matrix_cores(compact_lib, tmp_path):
    """POLICY = false: no dynamic LDS either (no LDS instruction, no barrier) and no MFMA -- read from the disassembly."""
    seen = 0
    for _, head, body in abi.function_bodies(compact_lib, tmp_path):
        if 'k_point_rollout_compact<' not in head or head.rstrip('>:').endswith('.kd'):
            continue
        words = set(re.findall(r'^\s+([a-z_0-9]+) ', body, flags=re.M))
        heavy = sorted(w for w in words if w.startswith(('ds_', 'v_mfma', 's_barrier')))
        if ', false>' in head:
            seen += 1
            assert not heavy, (head, heavy)
        else:
            assert any(w.startswith('ds_') for w in heavy), head       # the network is staged in LDS
    assert seen == 4, seen


def test_exec_mask_audit_finds_nothing(compact_lib):
    """Lane-predicated store blocks (shadow lanes past the batch, the append branch) next to a large register footprint: the
    shape in which the compiler defect of DESIGN.md section 9 was met."""
    abi.exec_audit(compact_lib)


def test_arguments_are_validated_without_a_gpu(compact_lib):
    from rl_on_manifold_amd import _lib_point_compact as lc, _lib_point_policy as lp, AtacomError
    lib = lc.load()
    fake = ctypes.create_string_buffer(256)          # not a handle: no magic number
    h = ctypes.cast(fake, ctypes.c_void_p)
    p = ctypes.c_void_p(0x1000)                      # never dereferenced

    def rollout(handle=h, n_steps=3, actions=None, net=None, records=p, stride=8, ends=p, cap=4, n_ends=p):
        return lib.atacom_point_compact_rollout(handle, n_steps, actions, None if net is None else ctypes.byref(net), None, None,
                                                records, stride, ends, cap, n_ends, None)

    def msg():
        return lib.atacom_point_compact_last_error().decode()

    assert rollout(handle=None, actions=p) == lc.E_INVALID and 'null' in msg()
    assert rollout(actions=p, records=None) == lc.E_INVALID and 'null' in msg()
    assert rollout() == lc.E_INVALID and 'exactly one' in msg()
    assert rollout(actions=p, net=_mlp()) == lc.E_INVALID and 'exactly one' in msg()
    for n in (0, -1):
        assert rollout(actions=p, n_steps=n) == lc.E_INVALID and 'n_steps must be positive' in msg()
    assert rollout(actions=p, n_steps=1 << 24) == lc.E_INVALID and '2^24' in msg()
    assert rollout(actions=p, stride=1 << 24) == lc.E_INVALID and '2^24' in msg()
    assert rollout(actions=p, n_ends=None) == lc.E_INVALID and 'd_n_ends is required' in msg()
    assert rollout(actions=p, ends=None) == lc.E_INVALID and 'd_ends' in msg()
    assert rollout(actions=p, cap=-1) == lc.E_INVALID and 'ends_capacity must be >= 0' in msg()
    # the network fields: refused with the words of atacom_point_policy_rollout_packed (one validator, two libraries)
    plib = lp.load()
    m = _mlp()
    m.struct_size -= 8
    cases = [(m, lc.E_INVALID, 'struct_size = %d' % m.struct_size)]
    cases += [(_mlp(**{f: bad}), lc.E_UNSUPPORTED, '%s = %d' % (f, bad)) for f, bad in (
        ('hidden', 32), ('n_out', 3), ('n_in', 16), ('activation', 2), ('mean_mode', 2), ('explore', 3), ('squash', 2))]
    cases += [(_mlp(W2=None), lc.E_INVALID, 'null weight'), (_mlp(sW1=0x1000), lc.E_INVALID, 'sigma network'),
              (_mlp(explore=1), lc.E_INVALID, 'act_low'), (_mlp(explore=2), lc.E_INVALID, 'ou_state'),
              (_mlp(explore=2, ou_state=0x1000), lc.E_INVALID, 'ou_dt'),
              (_mlp(explore=1, act_low=0x1000, act_high=0x1000, squash=1), lc.E_INVALID, 'squash')]
    for net, code, word in cases:
        assert rollout(net=net) == code, word
        assert word in msg(), (word, msg())
        assert plib.atacom_point_policy_rollout_packed(h, 3, None, ctypes.byref(net), None, None, p, 8, None) == code
        theirs = plib.atacom_point_policy_last_error().decode()
        assert theirs.replace('atacom_point_policy_rollout_packed', 'X') == msg().replace('atacom_point_compact_rollout', 'X')
    # valid arguments and a pointer that is not a live handle of this build: refused before anything of it is used
    assert rollout(actions=p) == lc.E_INVALID and 'handle' in msg()
    assert rollout(net=_mlp()) == lc.E_INVALID and 'handle' in msg()
    assert rollout(actions=p, ends=None, cap=0) == lc.E_INVALID and 'handle' in msg()       # NULL d_ends goes with capacity 0
    with pytest.raises(AtacomError):
        lc.check(rollout(handle=None, actions=p))


def test_python_surface():
    import rl_on_manifold_amd as pkg
    point, main = pkg.BatchedPointReachEnv.rollout_compact, pkg.BatchedAtacomEnv.rollout_compact
    names = list(inspect.signature(point).parameters)
    assert names[1:] == ['actions', 'policy', 'n_steps', 'noise', 'draws', 'out', 'batch_stride', 'ends_capacity']
    # BatchedAtacomEnv.rollout_compact's plus `draws`, every argument optional
    assert [n for n in names if n != 'draws'] == list(inspect.signature(main).parameters)
    assert all(p.default is None for p in list(inspect.signature(point).parameters.values())[1:])
    assert 'compact' in point.__doc__ and 'ends_capacity' in point.__doc__
