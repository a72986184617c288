"""CPU-only checks of libatacom_point_policy.so, the collision-avoidance task's rollout with the actor network in the kernel:
the header is plain C11, the declared symbols are exactly the exported ones and the ctypes table, the kernels are exactly
k_point_rollout_mlp<{float, double}, {2, 4}>, the float32 ones use no scratch, the exec-mask audit finds nothing and arguments
are validated before any device call.  No compute call is made (no GPU here)."""
import ctypes
import inspect

import pytest

import abi_tools as abi
from abi_tools import fake_mlp as _mlp


@pytest.fixture(scope='module')
def policy_lib():
    from rl_on_manifold_amd import build
    build.build('point', verbose=False)
    return build.build('point_policy', verbose=False)


def test_header_is_plain_c11(tmp_path):
    abi.compile_c11(tmp_path, abi.INCLUDE, '#include "atacom_point_policy_hip.h"\n'
                    'int main(void) { atacom_mlp m; m.struct_size = (int32_t)sizeof m;\n'
                    '    return atacom_point_policy_rollout(0, 1, &m, 0, 0, 0, 0, 0, 0, 0, 0, 0) == ATACOM_POINT_OK; }\n')


def test_library_exports_every_declared_symbol(policy_lib):
    from rl_on_manifold_amd import _lib_point_policy
    names = abi.one_symbol_set(policy_lib, 'atacom_point_policy_hip.h', 'atacom_point_policy_', _lib_point_policy)
    assert names == sorted('atacom_point_policy_' + n for n in ('rollout', 'rollout_packed', 'last_error', 'version'))
    assert _lib_point_policy.load().atacom_point_policy_version().startswith(b'atacom_point_policy')


@abi.needs_llvm('llvm-readelf')
def test_kernel_census_and_scratch(policy_lib, tmp_path):
    ks = abi.kernel_rows(policy_lib, tmp_path)
    assert [k[0] for k in ks] == sorted('k_point_rollout_mlp<%s, %d>' % (t, n) for t in ('float', 'double') for n in (2, 4)), ks
    for name, lds, scratch, vgpr, agpr, code in ks:
        print('%-34s VGPR %3d AGPR %3d scratch %d static LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        assert lds == 0, (name, lds)                 # the network's LDS is dynamic (sized by the launcher)
        if 'float' in name:
            assert scratch == 0, (name, scratch)     # the target of the production kernels: everything in registers
            assert vgpr <= 512


def test_exec_mask_audit_finds_nothing(policy_lib):
    """The kernels hold lane-predicated store blocks (shadow lanes past the batch) next to a large register footprint: the
    shape in which the compiler defect of DESIGN.md section 9 was met."""
    abi.exec_audit(policy_lib)


def test_arguments_are_validated_without_a_gpu(policy_lib):
    from rl_on_manifold_amd import _lib_point_policy as lp, AtacomError
    lib = lp.load()
    fake = ctypes.create_string_buffer(256)          # not a handle: no magic number
    h = ctypes.cast(fake, ctypes.c_void_p)
    out = ctypes.c_void_p(0x1000)

    def rollout(handle, m, n_steps=3):
        return lib.atacom_point_policy_rollout(handle, n_steps, ctypes.byref(m), None, None, out, None, out, out, out, out, None)

    def msg():
        return lib.atacom_point_policy_last_error().decode()

    assert rollout(None, _mlp()) == lp.E_INVALID and 'null' in msg()
    assert lib.atacom_point_policy_rollout_packed(None, 3, None, None, None, None, None, 8, None) == lp.E_INVALID
    m = _mlp()
    m.struct_size -= 8
    assert rollout(h, m) == lp.E_INVALID and 'struct_size = %d' % m.struct_size in msg()
    for field, bad, word in (('hidden', 32, 'hidden = 32'), ('n_out', 3, 'n_out = 3'), ('n_in', 16, 'n_in = 16'),
                             ('activation', 2, 'activation = 2'), ('mean_mode', 2, 'mean_mode = 2'), ('explore', 3, 'explore = 3'),
                             ('squash', 2, 'squash = 2')):
        assert rollout(h, _mlp(**{field: bad})) == lp.E_UNSUPPORTED, field
        assert word in msg(), (field, msg())
    assert rollout(h, _mlp(W2=None)) == lp.E_INVALID and 'null weight' in msg()
    assert rollout(h, _mlp(sW1=0x1000)) == lp.E_INVALID and 'sigma network' in msg()
    assert rollout(h, _mlp(explore=1)) == lp.E_INVALID and 'act_low' in msg()
    assert rollout(h, _mlp(explore=2)) == lp.E_INVALID and 'ou_state' in msg()
    assert rollout(h, _mlp(explore=2, ou_state=0x1000)) == lp.E_INVALID and 'ou_dt' in msg()
    assert rollout(h, _mlp(explore=1, act_low=0x1000, act_high=0x1000, squash=1)) == lp.E_INVALID and 'squash' in msg()
    assert rollout(h, _mlp(), n_steps=0) == lp.E_INVALID and 'n_steps' in msg()
    # a valid network and a pointer that is not a live handle of this build: refused before anything of it is used
    assert rollout(h, _mlp()) == lp.E_INVALID and 'handle' in msg()
    assert lib.atacom_point_policy_rollout_packed(h, 3, out, None, None, None, out, 8, None) == lp.E_INVALID and 'handle' in msg()
    assert lib.atacom_point_policy_rollout_packed(h, 3, out, ctypes.byref(_mlp()), None, None, out, 8, None) == lp.E_INVALID
    assert 'exactly one' in msg()
    with pytest.raises(AtacomError):
        lp.check(rollout(None, _mlp()))


def test_python_surface():
    import rl_on_manifold_amd as pkg
    env = pkg.BatchedPointReachEnv
    assert list(inspect.signature(env.rollout_policy).parameters)[1:] == ['policy', 'n_steps', 'noise', 'draws', 'want_next_obs']
    assert list(inspect.signature(env.rollout_packed).parameters)[1:] == ['actions', 'policy', 'n_steps', 'noise', 'draws', 'out',
                                                                          'batch_stride']
    doc = env.rollout_policy.__doc__.lower()
    assert 'host loop' in doc and 'fused' in doc
    assert hasattr(env, 'unpack_records') and isinstance(env.record_dim, property) and hasattr(env, '_on_my_device')
