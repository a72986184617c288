"""CPU-only checks of libatacom_evaluate.so, the network evaluation of a collection: the header is plain C11, the declared symbols
are exactly the exported ones and the ctypes table, every argument rule is enforced without a GPU and with a message, the kernel
census is the sixteen instantiations, the float32 kernels use no scratch and every kernel the documented LDS, the exec-mask audit
finds nothing and the Python signatures are the documented ones (its row of the build table: tests/test_build_table.py).  No
compute call is made (no GPU here)."""
import ctypes
import inspect
import subprocess

import pytest

import abi_tools as abi

FUNCTIONS = ('version', 'last_error', 'mlp')


@pytest.fixture(scope='module')
def evaluate_lib():
    from rl_on_manifold_amd import build
    return build.build('evaluate', verbose=False)


def test_header_is_plain_c11(tmp_path):
    abi.compile_c11(tmp_path, abi.INCLUDE, '#include "atacom_evaluate_hip.h"\n'
                    'int main(void) {\n'
                    '    atacom_evaluate_args a = {0};\n'
                    '    a.struct_size = sizeof a; a.net.struct_size = sizeof a.net; a.net.hidden = ATACOM_EVALUATE_HIDDEN;\n'
                    '    if (ATACOM_EVALUATE_MAX_IN != 32 || ATACOM_EVALUATE_MAX_OUT != 8) return 1;\n'
                    '    if (atacom_evaluate_mlp(&a) == ATACOM_EVALUATE_OK) return 2;\n'
                    '    return !atacom_evaluate_version() || !atacom_evaluate_last_error(); }\n')


def test_declared_exported_and_bound_symbols_are_one_set(evaluate_lib):
    from rl_on_manifold_amd import _lib_evaluate
    names = abi.one_symbol_set(evaluate_lib, 'atacom_evaluate_hip.h', 'atacom_evaluate_', _lib_evaluate)
    assert names == sorted('atacom_evaluate_' + n for n in FUNCTIONS)
    assert _lib_evaluate.load().atacom_evaluate_version().startswith(b'atacom_evaluate')


def test_the_ctypes_structs_have_the_layout_of_the_header(tmp_path):
    """sizeof and the offsets of the fields around the embedded network, as gcc lays the header out."""
    from rl_on_manifold_amd import _lib_evaluate as le
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include "atacom_evaluate_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(atacom_evaluate_view),\n'
                   '    sizeof(atacom_evaluate_args), offsetof(atacom_evaluate_args, n_outer), offsetof(atacom_evaluate_args, net),\n'
                   '    offsetof(atacom_evaluate_args, x), offsetof(atacom_evaluate_args, logp), offsetof(atacom_evaluate_args, stream),\n'
                   '    ATACOM_EVALUATE_MAX_IN, ATACOM_EVALUATE_MAX_OUT, ATACOM_EVALUATE_HIDDEN, ATACOM_EVALUATE_MAX_BLOCKS); return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c11', '-I', abi.INCLUDE, str(src), '-o', exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    A = le.EvaluateArgs
    assert got == [ctypes.sizeof(le.View), ctypes.sizeof(A), A.n_outer.offset, A.net.offset, A.x.offset, A.logp.offset,
                   A.stream.offset, le.MAX_IN, le.MAX_OUT, le.HIDDEN, le.MAX_BLOCKS]


def _valid(le, **net):
    """An argument struct that passes every check (its pointers are never dereferenced on the host): 3 x 5 rows of a 20 -> 2
    network with std, x and action as columns of [3, 5, 30] records, y and logp contiguous, all four requested."""
    a = le.new_args()
    a.device, a.dtype, a.n_blocks, a.n_outer, a.n_inner = 0, le.F32, 0, 3, 5
    a.net = abi.fake_mlp(**dict(dict(std=0x1000), **net))
    a.x, a.action = le.View(0x100000, 150, 30), le.View(0x100000 + 80, 150, 30)
    a.y, a.logp = le.View(0x200000, 10, 2), le.View(0x300000, 5, 1)
    return a


def test_arguments_are_validated_without_a_gpu(evaluate_lib):
    from rl_on_manifold_amd import _lib, _lib_evaluate as le, AtacomError
    lib = le.load()

    def msg():
        return lib.atacom_evaluate_last_error().decode()

    def refused(code, words, net=None, **change):
        a = _valid(le, **(net or {}))
        for k, val in change.items():
            obj = a
            *path, leaf = k.split('__')
            for part in path:
                obj = getattr(obj, part)
            setattr(obj, leaf, val)
        assert lib.atacom_evaluate_mlp(a) == code, (change, net, msg())
        assert words in msg() and 'atacom_evaluate_mlp' in msg(), (change, net, msg())

    assert lib.atacom_evaluate_mlp(None) == le.E_INVALID and 'null argument' in msg() and 'atacom_evaluate_mlp' in msg()
    refused(le.E_INVALID, 'struct_size', struct_size=ctypes.sizeof(le.EvaluateArgs) - 8)
    refused(le.E_INVALID, 'net.struct_size', net__struct_size=ctypes.sizeof(_lib.AtacomMlp) - 4)
    refused(le.E_INVALID, 'device', device=-1)
    refused(le.E_UNSUPPORTED, 'no kernel for dtype 2', dtype=2)
    # sizes below 1
    refused(le.E_INVALID, 'n_outer must be >= 1', n_outer=0)
    refused(le.E_INVALID, 'n_inner must be >= 1', n_inner=0)
    refused(le.E_INVALID, 'n_blocks must be >= 1', n_blocks=-1)
    refused(le.E_UNSUPPORTED, 'is too many', n_outer=2 ** 40, n_inner=2 ** 40)
    refused(le.E_UNSUPPORTED, 'is too many (at most 2147483647 a call)', n_outer=2 ** 16, n_inner=2 ** 15)      # 2^31 rows
    # the network
    for n_in in (0, 33):
        refused(le.E_UNSUPPORTED, 'n_in = %d is outside 1 .. 32' % n_in, net=dict(n_in=n_in))
    for n_out in (0, 9):
        refused(le.E_UNSUPPORTED, 'n_out = %d is outside 1 .. 8' % n_out, net=dict(n_out=n_out))
    refused(le.E_UNSUPPORTED, 'only 64 hidden units', net=dict(hidden=32))
    refused(le.E_UNSUPPORTED, 'activation = 2', net=dict(activation=2))
    for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
        refused(le.E_INVALID, 'null argument', net={k: None})
    # what is out of scope is refused, not ignored
    refused(le.E_UNSUPPORTED, 'sigma network', net=dict(sW1=0x1000))
    refused(le.E_UNSUPPORTED, 'squash', net=dict(squash=1))
    refused(le.E_UNSUPPORTED, 'mean_mode', net=dict(mean_mode=1))
    refused(le.E_UNSUPPORTED, 'explore', net=dict(explore=1))
    # the views
    refused(le.E_INVALID, 'null argument', x__ptr=None)
    refused(le.E_INVALID, 'neither y nor logp', y__ptr=None, logp__ptr=None)
    refused(le.E_INVALID, 'logp needs action and net.std', action__ptr=None)
    refused(le.E_INVALID, 'logp needs action and net.std', net=dict(std=None))
    refused(le.E_INVALID, 'x.stride_inner = 19 is below the row width 20', x__stride_inner=19)
    refused(le.E_INVALID, 'x.stride_outer = -19 is below the row width 20', x__stride_outer=-19)
    refused(le.E_INVALID, 'action.stride_inner = 1 is below the row width 2', action__stride_inner=1)
    refused(le.E_INVALID, 'y.stride_inner = 1 is below the row width 2', y__stride_inner=1)
    refused(le.E_INVALID, 'y.stride_outer = 0 is below the row width 2', y__stride_outer=0)      # an output repeats no row
    refused(le.E_INVALID, 'logp.stride_inner = 0 is below the row width 1', logp__stride_inner=0)
    refused(le.E_INVALID, 'y overlaps x', y__ptr=0x100000 + 4 * 439)                 # the last element of x
    refused(le.E_INVALID, 'y overlaps action', y__ptr=0x100000 + 4 * 440)            # past x, inside the action columns' extent
    refused(le.E_INVALID, 'logp overlaps x', logp__ptr=0x100000 - 4 * 14)            # its last element is x's first
    refused(le.E_INVALID, 'logp overlaps action', logp__ptr=0x100000 + 4 * 440)
    refused(le.E_INVALID, 'y overlaps logp', logp__ptr=0x200000 + 4 * 29)            # the last element of y
    refused(le.E_UNSUPPORTED, 'exceeds the launch grid', n_blocks=65536)
    # an input may repeat a row, a stride of a dimension of size 1 is not read, and y alone needs neither action nor std: these
    # pass every check and fail only at the device, which does not exist
    for change in (dict(x__stride_outer=0), dict(n_outer=1, y__stride_outer=0, x__stride_outer=3),
                   dict(logp__ptr=None, action__ptr=None)):
        a = _valid(le)
        for k, val in change.items():
            obj = a
            *path, leaf = k.split('__')
            for part in path:
                obj = getattr(obj, part)
            setattr(obj, leaf, val)
        a.device = 1 << 20                                          # no such device: nothing is launched either way
        assert lib.atacom_evaluate_mlp(a) == le.E_HIP, (change, msg())
    a = _valid(le)
    a.net.struct_size = _lib.AtacomMlp.mean_mode.offset             # ATACOM_MLP_SIZE_V1: accepted, the appended fields unread
    a.net.mean_mode, a.device = 1, 1 << 20
    assert lib.atacom_evaluate_mlp(a) == le.E_HIP, msg()
    with pytest.raises(AtacomError, match='null argument'):
        le.check(lib.atacom_evaluate_mlp(None))


def test_python_arguments_are_refused_before_the_library_is_called():
    torch = pytest.importorskip('torch')
    from rl_on_manifold_amd import MlpPolicy, evaluate
    from rl_on_manifold_amd.rollout import CompactRecordLayout, RecordLayout
    lin = lambda o, i: (torch.zeros(o, i), torch.zeros(o))          # noqa: E731
    pol = MlpPolicy(*lin(64, 4), *lin(64, 64), *lin(2, 64), std=torch.ones(2))
    critic = MlpPolicy(*lin(64, 4), *lin(64, 64), *lin(1, 64))
    x, act = torch.zeros(3, 5, 4), torch.zeros(3, 5, 2)
    lay, clay = RecordLayout([5], 4, 2), CompactRecordLayout([5], 4, 2, 3)
    for call, words in ((lambda: evaluate.evaluate_mlp(pol, x), 'run on a GPU'),
                        (lambda: evaluate.evaluate_mlp(pol, 3.0), r'\[\.\.\., n_in\]'),
                        (lambda: evaluate.gaussian_log_prob(pol, x, act), 'run on a GPU'),
                        (lambda: evaluate.evaluate_rows(pol, x, y=act.clone()), 'run on a GPU'),
                        (lambda: evaluate.evaluate_rows(pol, x), 'nothing to compute'),
                        (lambda: evaluate.values_from_records(lay, torch.zeros(3, 5, lay.F + 1), critic), 'full records must be'),
                        (lambda: evaluate.values_from_records(lay, torch.zeros(3, 5, lay.F), pol), 'to one value'),
                        (lambda: evaluate.values_from_compact(clay, torch.zeros(3, 5, clay.Fc), None, None, critic), 'rows of time'),
                        (lambda: evaluate.log_prob_from_records(clay, torch.zeros(3, 5, 7), pol), 'records must be')):
        with pytest.raises(ValueError, match=words):
            call()
    ddpg = MlpPolicy(*lin(64, 4), *lin(64, 64), *lin(2, 64), std=torch.ones(2))
    ddpg.explore = 2
    with pytest.raises(ValueError, match='DDPG'):
        ddpg.as_struct_on('cpu', torch.float32)
    m = pol.as_struct_on('cpu', torch.float64)                       # the sibling of as_struct needs no environment
    assert (m.n_in, m.hidden, m.n_out, m.activation) == (4, 64, 2, 0) and m.std and not m.obs_shift and not m.sW1


@abi.needs_llvm('llvm-readelf')
def test_kernel_census_and_resources(evaluate_lib, tmp_path):
    """Sixteen kernels: k_evaluate_mlp<T, CH> for CH = ceil(n_in / 4) = 1 .. 8.  Float32: no scratch, and 63808 bytes of LDS --
    the network block MlpLdsM<.., 64, 8>::NET = 7752 floats, 8 for the constant of logp, and 4 wavefronts x 2048 of staging.
    Float64: the block MlpLds<4 CH, 64, 8>::TOTAL = 5304 + 264 CH doubles and the same 8."""
    ks = abi.kernel_rows(evaluate_lib, tmp_path)
    assert [k[0] for k in ks] == sorted('k_evaluate_mlp<%s, %d>' % (t, ch) for t in ('float', 'double') for ch in range(1, 9)), ks
    for name, lds, scratch, vgpr, agpr, code in ks:
        print('%-28s VGPR %3d AGPR %3d scratch %d LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        ch = int(name[-2])
        if 'float' in name:
            assert scratch == 0, (name, scratch)
            assert lds == 4 * (7752 + 8 + 4 * 2048), (name, lds)
            assert vgpr <= 256, (name, vgpr)           # unified, accumulators included: two wavefronts per SIMD
        else:
            assert lds == 8 * (5304 + 264 * ch + 8), (name, lds)


@abi.needs_llvm('llvm-objdump')
def test_the_float32_kernels_run_on_the_matrix_cores_and_no_kernel_has_an_atomic(evaluate_lib, tmp_path):
    import re
    seen = 0
    for _, head, body in abi.function_bodies(evaluate_lib, tmp_path):
        k = re.search(r'k_evaluate_mlp<(float|double), (\d)>', head)
        if not k:
            continue
        seen += 1
        assert not re.search(r'\b(global|flat|ds|buffer)_atomic|\bds_(add|cmpst|wrxchg)', body), head
        mfma = len(re.findall(r'\bv_mfma_f32_16x16x4[_f32]*\b', body))
        # per 16-row block: 4 CH in layer 1, 64 in layer 2, 16 in the output layer; four blocks per wavefront
        assert mfma == (4 * (4 * int(k.group(2)) + 64 + 16) if k.group(1) == 'float' else 0), (head, mfma)
    assert seen == 16


def test_exec_mask_audit_finds_nothing(evaluate_lib):
    abi.exec_audit(evaluate_lib)


def test_python_surface():
    import rl_on_manifold_amd as pkg
    from rl_on_manifold_amd import evaluate

    def params(fn):
        return [(p.name, p.kind is p.KEYWORD_ONLY, None if p.default is p.empty else p.default)
                for p in inspect.signature(fn).parameters.values()]

    pos = lambda *names: [(n, False, None) for n in names]          # noqa: E731
    assert params(pkg.evaluate_mlp) == pos('net', 'x') + [('out', True, None)]
    assert params(pkg.gaussian_log_prob) == pos('policy', 'obs', 'action') + [('out', True, None), ('mean_out', True, None)]
    assert params(pkg.values_from_records) == pos('layout', 'g', 'critic')
    assert params(pkg.values_from_compact) == pos('layout', 'records', 'ends', 'n_ends', 'critic')
    assert params(pkg.log_prob_from_records) == pos('layout', 'rec', 'policy')
    assert params(pkg.evaluate_rows) == pos('net', 'x') + [('action', False, None), ('y', True, None), ('logp', True, None),
                                                          ('n_blocks', True, 0)]
    assert pkg.evaluate_mlp is evaluate.evaluate_mlp and pkg.values_from_compact is evaluate.values_from_compact
    assert params(pkg.MlpPolicy.as_struct_on) == pos('self', 'device', 'dtype')
    assert params(pkg.MlpPolicy.as_struct) == pos('self', 'env')
