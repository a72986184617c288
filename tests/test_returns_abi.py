"""CPU-only checks of libatacom_returns.so, the post-processing of a collection (advantages, normalisation, episode returns): the
header is plain C11, the declared symbols are exactly the exported ones and the ctypes table, every argument rule is enforced
without a GPU and with a message, no kernel uses scratch and only the reduction stage uses LDS, the exec-mask audit finds
nothing and the Python signatures are the documented ones.  No compute call is made (no GPU here)."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

import abi_tools as abi

FUNCTIONS = ('version', 'last_error', 'gae', 'normalize', 'episodes')


@pytest.fixture(scope='module')
def returns_lib():
    from rl_on_manifold_amd import build
    return build.build('returns', verbose=False)


def test_header_is_plain_c11(tmp_path):
    abi.compile_c11(tmp_path, abi.INCLUDE, '#include "atacom_returns_hip.h"\n'
                    'int main(void) {\n'
                    '    atacom_returns_gae_args g = {0}; atacom_returns_normalize_args n = {0}; atacom_returns_episodes_args e = {0};\n'
                    '    g.struct_size = sizeof g; n.struct_size = sizeof n; e.struct_size = sizeof e;\n'
                    '    if (ATACOM_RETURNS_WORKSPACE_DOUBLES(3, 5) != 3 * (15 + 256)) return 1;\n'
                    '    if (atacom_returns_gae(&g) == ATACOM_RETURNS_OK) return 2;\n'
                    '    if (atacom_returns_normalize(&n) == ATACOM_RETURNS_OK) return 3;\n'
                    '    return atacom_returns_episodes(&e) == ATACOM_RETURNS_OK || !atacom_returns_version() || !atacom_returns_last_error(); }\n')


def test_declared_exported_and_bound_symbols_are_one_set(returns_lib):
    from rl_on_manifold_amd import _lib_returns
    names = abi.one_symbol_set(returns_lib, 'atacom_returns_hip.h', 'atacom_returns_', _lib_returns)
    assert names == sorted('atacom_returns_' + n for n in FUNCTIONS)
    assert _lib_returns.load().atacom_returns_version().startswith(b'atacom_returns')


def test_the_ctypes_structs_have_the_layout_of_the_header(tmp_path):
    """sizeof and the offset of the last field of every argument struct, as gcc lays the header out."""
    from rl_on_manifold_amd import _lib_returns as lr
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include "atacom_returns_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(atacom_returns_view), sizeof(atacom_returns_shape),\n'
                   '    sizeof(atacom_returns_gae_args), offsetof(atacom_returns_gae_args, stream), sizeof(atacom_returns_normalize_args),\n'
                   '    offsetof(atacom_returns_normalize_args, stream), sizeof(atacom_returns_episodes_args),\n'
                   '    offsetof(atacom_returns_episodes_args, stream)); return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c11', '-I', abi.INCLUDE, str(src), '-o', exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(lr.View), ctypes.sizeof(lr.Shape), ctypes.sizeof(lr.GaeArgs), lr.GaeArgs.stream.offset,
                   ctypes.sizeof(lr.NormalizeArgs), lr.NormalizeArgs.stream.offset, ctypes.sizeof(lr.EpisodesArgs),
                   lr.EpisodesArgs.stream.offset]
    assert lr.workspace_doubles(3, 5) == 3 * (15 + 256)


def _valid(lr, cls):
    """An argument struct that passes every check (its pointers are never dereferenced on the host)."""
    a = lr.new_args(cls)
    p = 0x1000
    a.shape = lr.Shape(0, lr.F32, lr.FLAG_U8, 4, 5, 1, None)
    for name, kind in cls._fields_:
        if kind is lr.View:
            setattr(a, name, lr.View(p, 5, 1, 20))
        elif name.startswith('d_'):
            setattr(a, name, p)
    if cls is not lr.NormalizeArgs:
        a.gamma = 0.99
    if cls is lr.GaeArgs:
        a.lam = 0.95
    return a


def test_arguments_are_validated_without_a_gpu(returns_lib):
    from rl_on_manifold_amd import _lib_returns as lr, AtacomError
    lib = lr.load()
    calls = {lr.GaeArgs: lib.atacom_returns_gae, lr.NormalizeArgs: lib.atacom_returns_normalize,
             lr.EpisodesArgs: lib.atacom_returns_episodes}

    def msg():
        return lib.atacom_returns_last_error().decode()

    def refused(cls, code, words, **change):
        a = _valid(lr, cls)
        for k, val in change.items():
            obj = a
            *path, leaf = k.split('__')
            for part in path:
                obj = getattr(obj, part)
            setattr(obj, leaf, val)
        assert calls[cls](a) == code, (cls.__name__, change, msg())
        assert words in msg() and calls[cls].__name__ in msg(), (change, msg())

    for cls, fn in calls.items():
        assert fn(None) == lr.E_INVALID and 'null argument' in msg()
        refused(cls, lr.E_INVALID, 'struct_size', struct_size=ctypes.sizeof(cls) - 8)
        refused(cls, lr.E_INVALID, 'n_steps must be >= 1', shape__n_steps=0)
        refused(cls, lr.E_INVALID, 'batch must be >= 1', shape__batch=0)
        refused(cls, lr.E_INVALID, 'n_blocks must be >= 1', shape__n_blocks=0)
        refused(cls, lr.E_INVALID, 'device', shape__device=-1)
        refused(cls, lr.E_UNSUPPORTED, 'no kernel for dtype 2', shape__dtype=2)
        refused(cls, lr.E_UNSUPPORTED, 'exceeds the launch grid', shape__n_blocks=65536)
        for name, kind in cls._fields_:
            if name.startswith('d_'):          # the advantage call needs its two only to normalise
                refused(cls, lr.E_INVALID, 'null argument', normalize=1, **{name: None}) if cls is lr.GaeArgs else \
                    refused(cls, lr.E_INVALID, 'null argument', **{name: None})
            elif kind is lr.View and name not in ('v', 'v_next'):
                refused(cls, lr.E_INVALID, 'null argument', **{name + '__ptr': None})
    for cls in (lr.GaeArgs, lr.EpisodesArgs):
        refused(cls, lr.E_UNSUPPORTED, 'no kernel for flag_dtype 2', shape__flag_dtype=2)
        for bad in (-0.01, 1.01, float('nan')):
            refused(cls, lr.E_INVALID, 'gamma must be in [0, 1]', gamma=bad)
    for bad in (-0.01, 1.01, float('nan')):
        refused(lr.GaeArgs, lr.E_INVALID, 'lam must be in [0, 1]', lam=bad)
    refused(lr.GaeArgs, lr.E_INVALID, 'both', v__ptr=None)
    refused(lr.GaeArgs, lr.E_INVALID, 'both', v_next__ptr=None)
    refused(lr.GaeArgs, lr.E_UNSUPPORTED, 'normalisation', normalize=1, shape__n_steps=65536)
    refused(lr.NormalizeArgs, lr.E_UNSUPPORTED, 'normalisation', shape__n_steps=65536)
    with pytest.raises(AtacomError, match='null argument'):
        lr.check(lib.atacom_returns_gae(None))


def test_python_arguments_are_refused_before_the_library_is_called():
    torch = pytest.importorskip('torch')
    from rl_on_manifold_amd import returns
    r, f = torch.zeros(4, 5), torch.zeros(4, 5, dtype=torch.bool)
    for call, words in ((lambda: returns.compute_gae(r, f, f, r, r, 0.99, 0.95), 'run on a GPU'),
                        (lambda: returns.compute_gae(r, f, f, r, None, 0.99, 0.95), 'both'),
                        (lambda: returns.compute_gae(r, f, f[:3], None, None, 0.99, 0.95), 'shape'),
                        (lambda: returns.compute_gae(r, f, f.double(), None, None, 0.99, 0.95), 'bool, uint8 or'),
                        (lambda: returns.compute_gae(r, f, f.float(), None, None, 0.99, 0.95), 'must both be bool'),
                        (lambda: returns.compute_J(r, f, sizes=[5, 5]), 'does not describe'),
                        (lambda: returns.compute_J(r, f, sizes=[0]), 'no real environment'),
                        (lambda: returns.compute_J(r[0], f[0]), r'\[T, B\]')):
        with pytest.raises(ValueError, match=words):
            call()


@abi.needs_llvm('llvm-readelf')
def test_kernel_census_and_resources(returns_lib, tmp_path):
    ks = abi.kernel_rows(returns_lib, tmp_path)
    flags = {'float': ('float', 'unsigned char'), 'double': ('double', 'unsigned char')}
    want = ['k_returns_gae<%s, %s, %s>' % (e, f, v) for e in flags for f in flags[e] for v in ('false', 'true')] + \
           ['k_returns_episodes<%s, %s>' % (e, f) for e in flags for f in flags[e]] + \
           ['k_returns_%s<%s>' % (k, e) for k in ('lane_stats', 'normalize') for e in flags] + \
           ['k_returns_reduce_partial', 'k_returns_reduce_final<false>', 'k_returns_reduce_final<true>']
    assert [k[0] for k in ks] == sorted(want), ks
    for name, lds, scratch, vgpr, agpr, code in ks:
        print('%-44s VGPR %3d AGPR %2d scratch %d LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        assert scratch == 0, (name, scratch)
        assert lds == (3 * 256 * 8 if name.startswith('k_returns_reduce') else 0), (name, lds)


@abi.needs_llvm('llvm-objdump')
def test_the_scan_kernels_have_no_barrier_and_only_the_explicit_fused_operations(returns_lib, tmp_path):
    """No s_barrier in a scan kernel, and as many fused multiply-adds as the header writes down per step: two per
    step in the advantage kernels (kDepth unrolled steps), one in the episode kernels -- the compiler added none."""
    bodies = abi.function_bodies(returns_lib, tmp_path)
    assert len({elf for elf, _, _ in bodies}) == 1
    # the depth this build was compiled with: the header's default unless ATACOM_HIPCC_FLAGS overrides it
    header = open(os.path.join(abi.ROOT, 'rl_on_manifold_amd', 'csrc', 'atacom_returns.h')).read()
    override = re.search(r'-DATACOM_RETURNS_DEPTH=(\d+)', os.environ.get('ATACOM_HIPCC_FLAGS', ''))
    depth = int((override or re.search(r'define ATACOM_RETURNS_DEPTH (\d+)', header)).group(1))
    seen = 0
    for _, head, body in bodies:
        scan = re.search(r'k_returns_(gae|episodes|lane_stats)<(.*)>', head)
        if not scan:
            continue
        seen += 1
        assert 's_barrier' not in body, head
        fused = len(re.findall(r'\bv_(fma|fmac|mac|mad|pk_fma)_f(32|64)', body))
        per_step = {'gae': 2, 'episodes': 1, 'lane_stats': 0}[scan.group(1)]
        assert fused == per_step * depth, (head, fused)
    assert seen == 14


def test_exec_mask_audit_finds_nothing(returns_lib):
    abi.exec_audit(returns_lib)


def test_python_surface():
    import rl_on_manifold_amd as pkg
    from rl_on_manifold_amd import returns, rollout

    def params(fn):
        return [(p.name, p.kind is p.KEYWORD_ONLY, None if p.default is p.empty else p.default)
                for p in inspect.signature(fn).parameters.values()]

    pos = lambda *names: [(n, False, None) for n in names]          # noqa: E731
    assert params(pkg.compute_gae) == pos('reward', 'absorbing', 'last', 'v', 'v_next', 'gamma', 'lam') + \
        [('sizes', True, None), ('normalize', True, False), ('out', True, None)]
    assert params(pkg.compute_J) == pos('reward', 'last') + [('gamma', False, 1.0), ('sizes', True, None)]
    assert params(pkg.episode_returns) == params(pkg.compute_J)
    assert params(pkg.gae_from_records) == pos('layout', 'g', 'v', 'v_next', 'gamma', 'lam') + \
        [('normalize', True, False), ('out', True, None)]
    assert params(pkg.gae_from_compact) == pos('layout', 'records', 'ends', 'n_ends', 'v', 'v_ends', 'gamma', 'lam') + \
        [('normalize', True, False), ('out', True, None)]
    assert pkg.compute_gae is returns.compute_gae and pkg.normalize_advantages is returns.normalize_advantages
    torch = pytest.importorskip('torch')
    fields, F = rollout.record_fields(4, 2)
    rec = torch.arange(2 * 3 * F, dtype=torch.float32).reshape(2, 3, F)
    cols = rollout.record_columns(rec, fields)
    assert list(cols) == list(fields)
    assert cols['last'].dtype == torch.float32 and cols['last'].data_ptr() == rec[..., fields['last']].data_ptr()   # raw views
    assert torch.equal(cols['reward'], rec[..., 6]) and cols['reward'].stride() == (3 * F, F)
