"""CPU-only checks of libatacom_point_policy.so, the collision-avoidance task's rollout with the actor network in the kernel:
the header is plain C11, every declared symbol is exported, the kernels are exactly k_point_rollout_mlp<{float, double},
{2, 4}>, the float32 ones use no scratch, the exec-mask audit finds nothing, arguments are validated before any device call,
and the other two libraries' unit lists are untouched.  No compute call is made (no GPU here)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernel_resources import LLVM, _kernels        # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'atacom_point_policy_hip.h')


@pytest.fixture(scope='module')
def policy_lib():
    from rl_on_manifold_amd import build
    build.build_point(verbose=False)
    return build.build_point_policy(verbose=False)


def _declared_functions():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(atacom_point_policy_[a-z_]+)\s*\(', src)))


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "atacom_point_policy_hip.h"\n'
                   'int main(void) { atacom_mlp m; m.struct_size = (int32_t)sizeof m;\n'
                   '    return atacom_point_policy_rollout(0, 1, &m, 0, 0, 0, 0, 0, 0, 0, 0, 0) == ATACOM_POINT_OK; }\n')
    subprocess.check_call(['gcc', '-std=c11', '-pedantic', '-Wall', '-Werror', '-I', os.path.dirname(HEADER), '-c', str(src),
                           '-o', str(tmp_path / 'use.o')])


def test_library_exports_every_declared_symbol(policy_lib):
    from rl_on_manifold_amd import _lib_point_policy
    names = _declared_functions()
    assert names == sorted('atacom_point_policy_' + n for n in ('rollout', 'rollout_packed', 'last_error', 'version'))
    lib = ctypes.CDLL(policy_lib)
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(_lib_point_policy.EXPORTS) == names
    assert _lib_point_policy.load().atacom_point_policy_version().startswith(b'atacom_point_policy')


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, 'llvm-readelf')), reason='needs the ROCm LLVM binutils')
def test_kernel_census_and_scratch(policy_lib, tmp_path):
    ks = _kernels(str(tmp_path), so=policy_lib)
    names = sorted(k[0].replace('atacom_point::', '') for k in ks)
    assert names == sorted('k_point_rollout_mlp<%s, %d>' % (t, n) for t in ('float', 'double') for n in (2, 4)), names
    table = []
    for name, lds, scratch, vgpr, agpr, code in sorted(ks):
        name = name.replace('atacom_point::', '')
        table.append('%-34s VGPR %3d AGPR %3d scratch %d static LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        assert lds == 0, (name, lds)                 # the network's LDS is dynamic (sized by the launcher)
        if 'float' in name:
            assert scratch == 0, (name, scratch)     # the target of the production kernels: everything in registers
            assert vgpr <= 512
    print('\n'.join(table))


def test_exec_mask_audit_finds_nothing(policy_lib):
    """The kernels hold lane-predicated store blocks (shadow lanes past the batch) next to a large register footprint: the
    shape in which the compiler defect of DESIGN.md section 9 was met."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'profiles', 'tools', 'exec_restore_audit.py'), '--so', policy_lib],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 copies' in r.stdout, r.stdout


def _mlp(**kw):
    from rl_on_manifold_amd import _lib
    m = _lib.AtacomMlp()
    m.struct_size = ctypes.sizeof(_lib.AtacomMlp)
    m.n_in, m.hidden, m.n_out = 20, 64, 2
    for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
        setattr(m, k, 0x1000)                        # never dereferenced: every case below is refused on the host
    for k, v in kw.items():
        setattr(m, k, v)
    return m


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


def test_the_other_libraries_units_are_unchanged():
    from rl_on_manifold_amd import build
    assert build.UNITS_POINT == ['atacom_point.hip', 'atacom_point_capi.cpp']
    assert len(build.UNITS) == 14 and build.UNITS[-1] == 'atacom_capi.cpp'
    assert build.UNITS_POINT_POLICY == ['atacom_point_policy.hip', 'atacom_point_policy_capi.cpp']
    assert not set(build.UNITS_POINT_POLICY) & (set(build.UNITS) | set(build.UNITS_POINT))
    # editing the new units makes neither of the other two libraries stale
    own = {'atacom_point_policy.hip', 'atacom_point_policy_capi.cpp', 'atacom_point_policy.h', 'atacom_point_policy_ops.h'}
    for srcs in (build._sources(), build._sources_point()):
        assert not own & {os.path.basename(p) for p in srcs}
        assert not any(p.endswith('atacom_point_policy_hip.h') for p in srcs)
    assert own <= {os.path.basename(p) for p in build._sources_point_policy()}
    assert os.path.basename(build.LIB_POINT_POLICY) == 'libatacom_point_policy.so' or os.environ.get('ATACOM_POINT_POLICY_LIB_OUT')


def test_a_touched_header_makes_exactly_the_libraries_that_include_it_stale(monkeypatch):
    """The staleness rule of build.py (one rule over its table of targets), on faked modification times: no source is edited."""
    from rl_on_manifold_amd import build
    libs = (build.LIB, build.LIB_POINT, build.LIB_POINT_POLICY)
    touched = []
    real_exists = os.path.exists
    monkeypatch.setattr(build.os.path, 'exists', lambda p: p in libs or real_exists(p))
    monkeypatch.setattr(build.os.path, 'getmtime', lambda p: 2.0 if os.path.basename(p) in touched else 1.0)

    def stale():
        return [build.needs_build(), build.needs_build_point(), build.needs_build_point_policy()]

    assert stale() == [False, False, False]
    for header, want in (('atacom_point_policy.h', [False, False, True]), ('atacom_point.h', [False, True, True]),
                         ('atacom_point_handle.h', [False, True, True]), ('atacom_linalg.h', [True, True, True]),
                         ('atacom_capi_common.h', [True, True, True]), ('atacom_point_policy_hip.h', [False, False, True]),
                         ('atacom_point_hip.h', [False, True, True]), ('atacom_capi.cpp', [True, False, False])):
        touched[:] = [header]
        assert stale() == want, header
        assert os.path.exists(os.path.join(build.CSRC, header)) or os.path.exists(os.path.join(ROOT, 'include', header)), header


def test_python_surface():
    import inspect
    import rl_on_manifold_amd as pkg
    env = pkg.BatchedPointReachEnv
    assert list(inspect.signature(env.rollout_policy).parameters)[1:] == ['policy', 'n_steps', 'noise', 'draws', 'want_next_obs']
    assert list(inspect.signature(env.rollout_packed).parameters)[1:] == ['actions', 'policy', 'n_steps', 'noise', 'draws', 'out',
                                                                          'batch_stride']
    doc = env.rollout_policy.__doc__.lower()
    assert 'host loop' in doc and 'fused' in doc
    assert hasattr(env, 'unpack_records') and isinstance(env.record_dim, property) and hasattr(env, '_on_my_device')
