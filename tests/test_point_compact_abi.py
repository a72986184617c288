"""CPU-only checks of libatacom_point_compact.so, the collision-avoidance task's rollout in the compact record format: the
header is plain C11, the declared symbols are exactly the exported ones and the ctypes table, the kernels are exactly
k_point_rollout_compact<{float, double}, {2, 4}, {false, true}>, the float32 ones use no scratch and the ones with
pre-generated actions no LDS, the exec-mask audit finds nothing, arguments are validated before any device call, and the other
three libraries' unit lists are untouched.  No compute call is made (no GPU here)."""
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

HEADER = os.path.join(ROOT, 'include', 'atacom_point_compact_hip.h')
OWN = {'atacom_point_compact.hip', 'atacom_point_compact_capi.cpp', 'atacom_point_compact.h', 'atacom_point_compact_ops.h'}


@pytest.fixture(scope='module')
def compact_lib():
    from rl_on_manifold_amd import build
    build.build_point(verbose=False)
    return build.build_point_compact(verbose=False)


def _declared_functions():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(atacom_point_compact_[a-z_]+)\s*\(', src)))


def test_header_is_plain_c11(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "atacom_point_compact_hip.h"\n'
                   'int main(void) { atacom_mlp m; int32_t n = 0; m.struct_size = (int32_t)sizeof m;\n'
                   '    return atacom_point_compact_rollout(0, 1, 0, &m, 0, 0, 0, 1, 0, 0, &n, 0) == ATACOM_POINT_OK; }\n')
    subprocess.check_call(['gcc', '-std=c11', '-pedantic', '-Wall', '-Werror', '-I', os.path.dirname(HEADER), '-c', str(src),
                           '-o', str(tmp_path / 'use.o')])


def test_declared_exported_and_bound_symbols_are_one_set(compact_lib):
    from rl_on_manifold_amd import _lib_point_compact
    names = _declared_functions()
    assert names == sorted('atacom_point_compact_' + n for n in ('rollout', 'last_error', 'version'))
    nm = os.path.join(LLVM, 'llvm-nm')
    out = subprocess.run([nm if os.path.exists(nm) else 'nm', '-D', '--defined-only', compact_lib], capture_output=True,
                         text=True, check=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith('atacom_'))
    assert exported == names, exported
    assert sorted(_lib_point_compact.EXPORTS) == names
    assert _lib_point_compact.load().atacom_point_compact_version().startswith(b'atacom_point_compact')


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, 'llvm-readelf')), reason='needs the ROCm LLVM binutils')
def test_kernel_census_and_resources(compact_lib, tmp_path):
    ks = _kernels(str(tmp_path), so=compact_lib)
    names = sorted(k[0].replace('atacom_point::', '') for k in ks)
    assert names == sorted('k_point_rollout_compact<%s, %d, %s>' % (t, n, p) for t in ('float', 'double') for n in (2, 4)
                           for p in ('false', 'true')), names
    table = []
    for name, lds, scratch, vgpr, agpr, code in sorted(ks):
        name = name.replace('atacom_point::', '')
        table.append('%-46s VGPR %3d AGPR %3d scratch %d static LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        assert lds == 0, (name, lds)                 # the network's LDS is dynamic (sized by the launcher); none otherwise
        if 'float' in name:
            assert scratch == 0, (name, scratch)     # everything in registers
            assert vgpr <= 512
    print('\n'.join(table))


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, 'llvm-objdump')), reason='needs the ROCm LLVM binutils')
def test_kernels_with_pregenerated_actions_use_no_lds_and_no_matrix_cores(compact_lib, tmp_path):
    """POLICY = false: no dynamic LDS either (no LDS instruction, no barrier) and no MFMA -- read from the disassembly."""
    _kernels(str(tmp_path), so=compact_lib)                      # leaves the code objects in tmp_path as dev<offset>.elf
    seen = 0
    for elf in sorted(f for f in os.listdir(str(tmp_path)) if f.startswith('dev') and f.endswith('.elf')):
        asm = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--demangle', os.path.join(str(tmp_path), elf)],
                             capture_output=True, text=True, check=True).stdout
        for body in re.split(r'\n(?=[0-9a-f]+ <)', asm):
            head = body.split('\n', 1)[0]
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'profiles', 'tools', 'exec_restore_audit.py'), '--so', compact_lib],
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


def test_the_other_libraries_units_are_unchanged():
    from rl_on_manifold_amd import build
    assert build.UNITS_POINT == ['atacom_point.hip', 'atacom_point_capi.cpp']
    assert len(build.UNITS) == 14 and build.UNITS[-1] == 'atacom_capi.cpp'
    assert build.UNITS_POINT_POLICY == ['atacom_point_policy.hip', 'atacom_point_policy_capi.cpp']
    assert build.UNITS_POINT_COMPACT == ['atacom_point_compact.hip', 'atacom_point_compact_capi.cpp']
    assert not set(build.UNITS_POINT_COMPACT) & (set(build.UNITS) | set(build.UNITS_POINT) | set(build.UNITS_POINT_POLICY))
    assert build.TARGETS['point_compact'].feeds == ('point', 'point_policy')
    # editing the new files makes none of the other three libraries stale
    for srcs in (build._sources(), build._sources_point(), build._sources_point_policy()):
        assert not OWN & {os.path.basename(p) for p in srcs}
        assert not any(p.endswith('atacom_point_compact_hip.h') for p in srcs)
    mine = {os.path.basename(p) for p in build._sources_point_compact()}
    assert OWN <= mine
    # ... and what it borrows makes it stale: the handle, the environment, the policy kernel's header and validator
    assert {'atacom_point_handle.h', 'atacom_point.h', 'atacom_point_policy.h', 'atacom_point_policy_ops.h', 'atacom_policy.h',
            'atacom_point_compact_hip.h'} <= mine
    assert os.path.basename(build.LIB_POINT_COMPACT) == 'libatacom_point_compact.so' or os.environ.get('ATACOM_POINT_COMPACT_LIB_OUT')


def test_a_touched_header_makes_exactly_the_libraries_that_include_it_stale(monkeypatch):
    """The staleness rule of build.py with the fourth target in the table, on faked modification times."""
    from rl_on_manifold_amd import build
    libs = (build.LIB, build.LIB_POINT, build.LIB_POINT_POLICY, build.LIB_POINT_COMPACT)
    touched = []
    real_exists = os.path.exists
    monkeypatch.setattr(build.os.path, 'exists', lambda p: p in libs or real_exists(p))
    monkeypatch.setattr(build.os.path, 'getmtime', lambda p: 2.0 if os.path.basename(p) in touched else 1.0)

    def stale():
        return [build.needs_build(), build.needs_build_point(), build.needs_build_point_policy(), build.needs_build_point_compact()]

    assert stale() == [False] * 4
    for header, want in (('atacom_point_compact.h', [False, False, False, True]),
                         ('atacom_point_compact_ops.h', [False, False, False, True]),
                         ('atacom_point_compact_hip.h', [False, False, False, True]),
                         ('atacom_point_compact_capi.cpp', [False, False, False, True]),
                         ('atacom_point_policy.h', [False, False, True, True]),
                         ('atacom_point_policy_ops.h', [False, False, True, True]),
                         ('atacom_point_policy_hip.h', [False, False, True, True]),
                         ('atacom_point.h', [False, True, True, True]), ('atacom_point_handle.h', [False, True, True, True]),
                         ('atacom_kernels.h', [True, True, True, True]), ('atacom_point_policy.hip', [False, False, True, False])):
        touched[:] = [header]
        assert stale() == want, header
        assert os.path.exists(os.path.join(build.CSRC, header)) or os.path.exists(os.path.join(ROOT, 'include', header)), header


def test_python_surface():
    import rl_on_manifold_amd as pkg
    point, main = pkg.BatchedPointReachEnv.rollout_compact, pkg.BatchedAtacomEnv.rollout_compact
    names = list(inspect.signature(point).parameters)
    assert names[1:] == ['actions', 'policy', 'n_steps', 'noise', 'draws', 'out', 'batch_stride', 'ends_capacity']
    # BatchedAtacomEnv.rollout_compact's plus `draws`, every argument optional
    assert [n for n in names if n != 'draws'] == list(inspect.signature(main).parameters)
    assert all(p.default is None for p in list(inspect.signature(point).parameters.values())[1:])
    assert 'compact' in point.__doc__ and 'ends_capacity' in point.__doc__
