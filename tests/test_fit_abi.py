"""CPU-only checks of libatacom_fit.so, the gradients of an on-policy update: the header is plain C11, the declared symbols are
exactly the exported ones and the ctypes table, every argument rule is enforced without a GPU and with a message, the kernel
census is the sixteen gradient instantiations and the two reductions, the float32 kernels use no scratch and run on the matrix
cores, every kernel has the documented LDS, the exec-mask audit finds nothing and the Python signatures are the documented ones
(its row of the build tables: tests/test_fit_build.py).  No compute call is made (no GPU here)."""
import ctypes
import inspect
import re
import subprocess

import pytest

import abi_tools as abi

FUNCTIONS = ('version', 'last_error', 'workspace_size', 'gradient')


@pytest.fixture(scope='module')
def fit_lib():
    from rl_on_manifold_amd import build
    return build.build('fit', verbose=False)


def test_header_is_plain_c11(tmp_path):
    abi.compile_c11(tmp_path, abi.INCLUDE, '#include "atacom_fit_hip.h"\n'
                    'int main(void) {\n'
                    '    atacom_fit_args a = {0};\n'
                    '    a.struct_size = sizeof a; a.net.struct_size = sizeof a.net; a.net.hidden = ATACOM_FIT_HIDDEN;\n'
                    '    a.head = ATACOM_FIT_PPO_CLIP;\n'
                    '    if (ATACOM_FIT_MAX_IN != 32 || ATACOM_FIT_MAX_OUT != 8 || ATACOM_FIT_STATS != 4) return 1;\n'
                    '    if (atacom_fit_gradient(&a) == ATACOM_FIT_OK || atacom_fit_workspace_size(&a) != 0) return 2;\n'
                    '    return !atacom_fit_version() || !atacom_fit_last_error(); }\n')


def test_declared_exported_and_bound_symbols_are_one_set(fit_lib):
    from rl_on_manifold_amd import _lib_fit
    names = abi.one_symbol_set(fit_lib, 'atacom_fit_hip.h', 'atacom_fit_', _lib_fit)
    assert names == sorted('atacom_fit_' + n for n in FUNCTIONS)
    assert _lib_fit.load().atacom_fit_version().startswith(b'atacom_fit')


def test_the_ctypes_struct_has_the_layout_of_the_header(tmp_path):
    """sizeof and the offset of every field after the embedded network, as gcc lays the header out."""
    from rl_on_manifold_amd import _lib_fit as lf
    fields = ('head', 'n_outer', 'net', 'x', 'action', 'weight', 'logp_old', 'idx', 'n_idx', 'clip', 'grad', 'stats', 'workspace',
              'workspace_bytes', 'stream')
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include "atacom_fit_hip.h"\nint main(void) { printf("%zu", sizeof(atacom_fit_args));\n' +
                   ''.join('    printf(" %%zu", offsetof(atacom_fit_args, %s));\n' % f for f in fields) +
                   '    printf(" %d %d %d %d %d %d %d\\n", ATACOM_FIT_MAX_IN, ATACOM_FIT_MAX_OUT, ATACOM_FIT_HIDDEN, ATACOM_FIT_MAX_BLOCKS,\n'
                   '           ATACOM_FIT_STATS, ATACOM_FIT_VALUE, ATACOM_FIT_PPO_CLIP); return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c11', '-I', abi.INCLUDE, str(src), '-o', exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    A = lf.FitArgs
    assert got == [ctypes.sizeof(A)] + [getattr(A, f).offset for f in fields] + [lf.MAX_IN, lf.MAX_OUT, lf.HIDDEN, lf.MAX_BLOCKS,
                                                                              lf.STATS, lf.VALUE, lf.PPO_CLIP]


X, ACTION, WEIGHT, LOGP, GRAD, STATS, WORK, IDX = 0x100000, 0x100000 + 80, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000
P = 64 * 20 + 64 + 4096 + 64 + 64 * 2 + 2            # the gradient of a 20 -> 2 network


def _valid(lf, **net):
    """An argument struct that passes every check (its pointers are never dereferenced on the host): the PPO head over 3 x 5
    rows of a 20 -> 2 network with std, x and action as columns of [3, 5, 30] records, the rest contiguous."""
    a = lf.new_args()
    a.device, a.dtype, a.n_blocks, a.head, a.n_outer, a.n_inner, a.clip = 0, lf.F32, 0, lf.PPO_CLIP, 3, 5, 0.2
    a.net = abi.fake_mlp(**dict(dict(std=0x1000), **net))
    a.x, a.action = lf.View(X, 150, 30), lf.View(ACTION, 150, 30)
    a.weight, a.logp_old = lf.View(WEIGHT, 5, 1), lf.View(LOGP, 5, 1)
    a.grad, a.stats, a.workspace, a.workspace_bytes = GRAD, STATS, WORK, 4 * (P + 2 + 4) + 256
    return a


def _apply(a, change):
    for k, val in change.items():
        obj = a
        *path, leaf = k.split('__')
        for part in path:
            obj = getattr(obj, part)
        setattr(obj, leaf, val)
    return a


def test_the_workspace_size_follows_the_documented_rule(fit_lib):
    from rl_on_manifold_amd import _lib_fit as lf
    lib = lf.load()
    up = lambda n: (n + 255) // 256 * 256                 # noqa: E731
    q = P + 2 + 4
    assert lib.atacom_fit_workspace_size(_valid(lf)) == up(4 * q)                                  # 15 rows: one workgroup
    assert lib.atacom_fit_workspace_size(_apply(_valid(lf), dict(dtype=lf.F64))) == up(8 * q)      # 15 rows of 16 a workgroup
    assert lib.atacom_fit_workspace_size(_apply(_valid(lf), dict(n_blocks=7))) == up(4 * 7 * q)
    assert lib.atacom_fit_workspace_size(_apply(_valid(lf), dict(n_outer=100, n_inner=100))) == up(4 * 40 * q)     # ceil(10000 / 256)
    assert lib.atacom_fit_workspace_size(_apply(_valid(lf), dict(n_outer=1000, n_inner=1000))) == up(4 * 512 * q)  # the ceiling
    assert lib.atacom_fit_workspace_size(_apply(_valid(lf), dict(n_outer=1000, n_inner=1000, idx=IDX, n_idx=257))) == up(4 * 2 * q)
    assert lib.atacom_fit_workspace_size(_apply(_valid(lf), dict(dtype=lf.F64, idx=IDX, n_idx=33))) == up(8 * 3 * q)
    assert lib.atacom_fit_workspace_size(_apply(_valid(lf), dict(n_blocks=65536))) == 0
    assert 'atacom_fit_workspace_size' in lib.atacom_fit_last_error().decode() and 'launch grid' in lib.atacom_fit_last_error().decode()
    assert lib.atacom_fit_workspace_size(None) == 0


def test_arguments_are_validated_without_a_gpu(fit_lib):
    from rl_on_manifold_amd import _lib, _lib_fit as lf, AtacomError
    lib = lf.load()

    def msg():
        return lib.atacom_fit_last_error().decode()

    def refused(code, words, net=None, **change):
        a = _apply(_valid(lf, **(net or {})), change)
        assert lib.atacom_fit_gradient(a) == code, (change, net, msg())
        assert words in msg() and 'atacom_fit_gradient' in msg(), (change, net, msg())

    assert lib.atacom_fit_gradient(None) == lf.E_INVALID and 'null argument' in msg() and 'atacom_fit_gradient' in msg()
    refused(lf.E_INVALID, 'struct_size', struct_size=ctypes.sizeof(lf.FitArgs) - 8)
    refused(lf.E_INVALID, 'net.struct_size', net__struct_size=ctypes.sizeof(_lib.AtacomMlp) - 4)
    refused(lf.E_INVALID, 'device', device=-1)
    refused(lf.E_UNSUPPORTED, 'no kernel for dtype 2', dtype=2)
    refused(lf.E_UNSUPPORTED, 'head = 2', head=2)
    # sizes
    refused(lf.E_INVALID, 'n_outer must be >= 1', n_outer=0)
    refused(lf.E_INVALID, 'n_inner must be >= 1', n_inner=0)
    refused(lf.E_INVALID, 'n_blocks must be >= 1', n_blocks=-1)
    refused(lf.E_UNSUPPORTED, 'is too many', n_outer=2 ** 40, n_inner=2 ** 40)
    refused(lf.E_UNSUPPORTED, 'is too many (at most 2147483647 a call)', n_outer=2 ** 16, n_inner=2 ** 15)
    refused(lf.E_UNSUPPORTED, 'exceeds the launch grid', n_blocks=65536)
    refused(lf.E_INVALID, 'n_idx must be >= 1 with idx', idx=IDX, n_idx=0)
    refused(lf.E_UNSUPPORTED, 'n_idx = 2147483648 rows is too many', idx=IDX, n_idx=2 ** 31)
    # the network
    for n_in in (0, 33):
        refused(lf.E_UNSUPPORTED, 'n_in = %d is outside 1 .. 32' % n_in, net=dict(n_in=n_in))
    for n_out in (0, 9):
        refused(lf.E_UNSUPPORTED, 'n_out = %d is outside 1 .. 8' % n_out, net=dict(n_out=n_out))
    refused(lf.E_UNSUPPORTED, 'the value head fits a network of one output', head=lf.VALUE)
    refused(lf.E_UNSUPPORTED, 'only 64 hidden units', net=dict(hidden=32))
    refused(lf.E_UNSUPPORTED, 'activation = 2', net=dict(activation=2))
    for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
        refused(lf.E_INVALID, 'null argument', net={k: None})
    # what is out of scope is refused, not ignored
    refused(lf.E_UNSUPPORTED, 'sigma network', net=dict(sW1=0x1000))
    refused(lf.E_UNSUPPORTED, 'squash', net=dict(squash=1))
    refused(lf.E_UNSUPPORTED, 'mean_mode', net=dict(mean_mode=1))
    refused(lf.E_UNSUPPORTED, 'explore', net=dict(explore=1))
    # the views and the head's arguments
    refused(lf.E_INVALID, 'null argument (x)', x__ptr=None)
    refused(lf.E_INVALID, 'null argument (weight)', weight__ptr=None)
    for k in ('grad', 'stats', 'workspace'):
        refused(lf.E_INVALID, 'null argument (grad, stats or workspace)', **{k: None})
    refused(lf.E_INVALID, 'the PPO head needs action, logp_old and net.std', action__ptr=None)
    refused(lf.E_INVALID, 'the PPO head needs action, logp_old and net.std', logp_old__ptr=None)
    refused(lf.E_INVALID, 'the PPO head needs action, logp_old and net.std', net=dict(std=None))
    refused(lf.E_INVALID, 'clip must be > 0', clip=0.0)
    refused(lf.E_INVALID, 'clip must be > 0', clip=-0.2)
    refused(lf.E_INVALID, 'clip must be > 0', clip=float('nan'))
    refused(lf.E_INVALID, 'x.stride_inner = 19 is below the row width 20', x__stride_inner=19)
    refused(lf.E_INVALID, 'x.stride_outer = -19 is below the row width 20', x__stride_outer=-19)
    refused(lf.E_INVALID, 'action.stride_inner = 1 is below the row width 2', action__stride_inner=1)
    # every overlap: each output with each input, and the outputs with each other
    last_x = X + 4 * 439
    for out, span in (('grad', 4 * (P + 2)), ('stats', 16), ('workspace', 4 * (P + 6))):
        refused(lf.E_INVALID, out + ' overlaps x', **{out: last_x})
        refused(lf.E_INVALID, out + ' overlaps action', **{out: X + 4 * 440})          # past x, inside the action columns' extent
        refused(lf.E_INVALID, out + ' overlaps weight', **{out: WEIGHT + 4 * 14})      # the last target
        refused(lf.E_INVALID, out + ' overlaps logp_old', **{out: LOGP - span + 4})    # its last element is logp_old's first
        refused(lf.E_INVALID, out + ' overlaps idx', **{out: IDX + 8 * 3, 'idx': IDX, 'n_idx': 4})
    refused(lf.E_INVALID, 'grad overlaps stats', stats=GRAD + 4 * (P + 1))             # the last d log std
    refused(lf.E_INVALID, 'grad overlaps workspace', workspace=GRAD - 4 * (P + 6) + 4)
    refused(lf.E_INVALID, 'stats overlaps workspace', workspace=STATS + 12)
    refused(lf.E_INVALID, 'workspace_bytes = 22559 is below the 22784', workspace_bytes=4 * (P + 6) - 1)
    # An input may repeat a row, a stride of a dimension of size 1 is not read, the value head needs neither action nor
    # logp_old, std or clip, and adjacent buffers do not overlap: these pass every check and fail only at the device, which does
    # not exist
    for net, change in ((None, dict(x__stride_outer=0)), (None, dict(n_outer=1, x__stride_outer=3)),
                        (None, dict(idx=IDX, n_idx=1000, workspace_bytes=(4 * 4 * (P + 6) + 255) // 256 * 256)),
                        (None, dict(stats=GRAD + 4 * (P + 2))),
                        (dict(n_out=1, std=None), dict(head=lf.VALUE, action__ptr=None, logp_old__ptr=None, clip=0.0))):
        a = _apply(_valid(lf, **(net or {})), change)
        a.device = 1 << 20                                          # no such device: nothing is launched either way
        assert lib.atacom_fit_gradient(a) == lf.E_HIP, (change, msg())
    a = _valid(lf)
    a.net.struct_size = _lib.AtacomMlp.mean_mode.offset             # ATACOM_MLP_SIZE_V1: accepted, the appended fields unread
    a.net.mean_mode, a.device = 1, 1 << 20
    assert lib.atacom_fit_gradient(a) == lf.E_HIP, msg()
    with pytest.raises(AtacomError, match='null argument'):
        lf.check(lib.atacom_fit_gradient(None))


def test_python_arguments_are_refused_before_the_library_is_called():
    torch = pytest.importorskip('torch')
    from rl_on_manifold_amd import MlpPolicy, fit
    from rl_on_manifold_amd.rollout import CompactRecordLayout, RecordLayout
    lin = lambda o, i: (torch.zeros(o, i), torch.zeros(o))          # noqa: E731
    pol = MlpPolicy(*lin(64, 4), *lin(64, 64), *lin(2, 64), std=torch.ones(2))
    nostd = MlpPolicy(*lin(64, 4), *lin(64, 64), *lin(2, 64))
    critic = MlpPolicy(*lin(64, 4), *lin(64, 64), *lin(1, 64))
    x, act, w = torch.zeros(3, 5, 4), torch.zeros(3, 5, 2), torch.zeros(3, 5)
    lay, clay = RecordLayout([5], 4, 2), CompactRecordLayout([5], 4, 2, 3)
    idx = torch.zeros(4, dtype=torch.int64)
    for call, words in ((lambda: fit.value_gradient(critic, x, w), 'run on a GPU'),
                        (lambda: fit.policy_gradient(pol, x, act, w, w), 'run on a GPU'),
                        (lambda: fit.value_gradient(critic, x, w, idx=idx, n_blocks=3), 'run on a GPU'),
                        (lambda: fit.value_gradient_from_records(lay, torch.zeros(3, 5, lay.F), w, critic), 'run on a GPU'),
                        (lambda: fit.policy_gradient_from_records(clay, torch.zeros(4, 5, clay.Fc), w, w, pol), 'run on a GPU'),
                        (lambda: fit.value_gradient(critic, 3.0, w), r'\[\.\.\., n_in\]'),
                        (lambda: fit.value_gradient(critic, x.to(torch.float16), w), 'float32 or float64'),
                        (lambda: fit.value_gradient_from_records(lay, torch.zeros(3, 5, lay.F + 1), w, critic), 'records must be'),
                        (lambda: fit.policy_gradient_from_records(clay, torch.zeros(3, 5, clay.Fc), w, w, pol), 'rows of time'),
                        (lambda: fit.policy_gradient(nostd, x, act, w, w), 'a policy with std'),
                        (lambda: fit.policy_gradient(pol, x, act, w, w, clip=0.0), 'clip must be > 0'),
                        (lambda: fit.value_gradient(pol, x, w), 'to one value'),
                        (lambda: fit.value_gradient(critic, torch.zeros(3, 5, 5), w), 'rows of 5 where the network takes 4'),
                        (lambda: fit.value_gradient(critic, torch.zeros(3, 0, 4), torch.zeros(3, 0)), 'holds no rows'),
                        (lambda: fit.value_gradient(critic, x, torch.zeros(3, 4)), 'target must be a tensor of shape'),
                        (lambda: fit.policy_gradient(pol, x, torch.zeros(3, 5, 3), w, w), 'action must be a tensor of shape'),
                        (lambda: fit.policy_gradient(pol, x, act, w, w.double()), 'logp_old must be a torch.float32'),
                        (lambda: fit.policy_gradient(pol, x, act, torch.zeros(3, 5, 1), w), 'adv must be a tensor of shape'),
                        (lambda: fit.value_gradient(critic, torch.zeros(3, 5, 8)[..., ::2], w), 'must be contiguous'),
                        (lambda: fit.value_gradient(critic, torch.zeros(2, 4, 8, 4)[:, :3, :5], torch.zeros(2, 3, 5)), 'do not collapse'),
                        (lambda: fit.value_gradient(critic, x, w, idx=idx.int()), 'idx must be a one-dimensional int64'),
                        (lambda: fit.value_gradient(critic, x, w, idx=idx[:0]), 'at least one row number'),
                        (lambda: fit.value_gradient(critic, x, w, idx=torch.zeros(8, dtype=torch.int64)[::2]), 'idx must be contiguous'),
                        (lambda: fit.value_gradient(critic, x, w, n_blocks=65536), 'n_blocks must be 0')):
        with pytest.raises(ValueError, match=words):
            call()
    with pytest.raises(ValueError, match='row numbers from 0 to 15'):
        fit.check_idx(torch.tensor([0, 15, 3]), 15)
    g = fit.Gradients(4, 2, fit._lf.PPO_CLIP, torch.float32, 'cpu', 256, None)
    assert g.flat.numel() == 64 * 4 + 64 + 4096 + 64 + 128 + 2 + 2 and g.log_std.shape == (2,) and g.W3.shape == (2, 64)
    assert g.b3.data_ptr() == g.flat.data_ptr() + 4 * (64 * 4 + 64 + 4096 + 64 + 128)
    assert fit.Gradients(4, 1, fit._lf.VALUE, torch.float64, 'cpu', 256, None).log_std is None
    with pytest.raises(ValueError, match='holds no d log std'):
        fit.Gradients(4, 1, fit._lf.VALUE, torch.float32, 'cpu', 256, None).to_module(
            type('N', (), dict(_h1=torch.nn.Linear(4, 64), _h2=torch.nn.Linear(64, 64), _h3=torch.nn.Linear(64, 1)))(), torch.zeros(1))
    with pytest.raises(ValueError, match='where its gradient is'):
        g.to_module(type('N', (), dict(_h1=torch.nn.Linear(5, 64), _h2=torch.nn.Linear(64, 64), _h3=torch.nn.Linear(64, 2)))())


@abi.needs_llvm('llvm-readelf')
def test_kernel_census_and_resources(fit_lib, tmp_path):
    """Eighteen kernels: k_fit_gradient<T, CH> for CH = ceil(n_in / 4) = 1 .. 8 and k_fit_reduce<T>.  Float32: no scratch, at most
    the 512 registers of one wavefront per SIMD (the launch bound), and 63808 bytes of LDS -- the network block
    MlpLdsM<.., 64, 8>::NET = 7752 floats, 8 for the constant of logp, and 4 wavefronts x 2048 of staging (two [16][64]
    transposition buffers).  Float64: 16 records of 285 + 4 CH doubles."""
    ks = abi.kernel_rows(fit_lib, tmp_path)
    want = ['k_fit_gradient<%s, %d>' % (t, ch) for t in ('float', 'double') for ch in range(1, 9)] + ['k_fit_reduce<float>', 'k_fit_reduce<double>']
    assert [k[0] for k in ks] == sorted(want), ks
    for name, lds, scratch, vgpr, agpr, code in ks:
        print('%-28s VGPR %3d AGPR %3d scratch %d LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        if 'reduce' in name:
            assert lds == 8 * 32 * (4 if 'float' in name else 8) and scratch == 0, name       # eight slices of 32 values
            continue
        ch = int(name[-2])
        assert vgpr <= 512, (name, vgpr)               # unified, accumulators included: __launch_bounds__(256, 1)
        if 'float' in name:
            assert scratch == 0, (name, scratch)
            assert lds == 4 * (7752 + 8 + 4 * 2048), (name, lds)
        else:
            assert lds == 8 * 16 * (285 + 4 * ch), (name, lds)


@abi.needs_llvm('llvm-objdump')
def test_the_float32_kernels_run_on_the_matrix_cores_and_no_kernel_has_an_atomic(fit_lib, tmp_path):
    seen = 0
    for _, head, body in abi.function_bodies(fit_lib, tmp_path):
        k = re.search(r'k_fit_(gradient<(float|double), (\d)>|reduce<(float|double)>)', head)
        if not k:
            continue
        seen += 1
        assert not re.search(r'\b(global|flat|ds|buffer)_atomic|\bds_(add|cmpst|wrxchg)', body), head
        mfma = len(re.findall(r'\bv_mfma_f32_16x16x4[_f32]*\b', body))
        if k.group(2) == 'float':
            # per block of 16 rows: forward 4 CH + 64 + 16; W3^T dy 8, W2^T da2 64; dW3 16, dW2 64, dW1 16 per tile of 16 inputs
            ch = int(k.group(3))
            assert mfma == 4 * ch + 64 + 16 + 8 + 64 + 16 + 64 + 16 * (2 if 4 * ch > 16 else 1), (head, mfma)
        else:
            assert mfma == 0, (head, mfma)
    assert seen == 18


def test_exec_mask_audit_finds_nothing(fit_lib):
    abi.exec_audit(fit_lib)


def test_python_surface():
    import rl_on_manifold_amd as pkg
    from rl_on_manifold_amd import fit

    def params(fn):
        return [(p.name, p.kind is p.KEYWORD_ONLY, None if p.default is p.empty else p.default)
                for p in inspect.signature(fn).parameters.values()]

    pos = lambda *names: [(n, False, None) for n in names]          # noqa: E731
    assert params(pkg.value_gradient) == pos('critic', 'obs', 'target') + [('idx', True, None), ('out', True, None), ('n_blocks', True, 0)]
    assert params(pkg.policy_gradient) == pos('policy', 'obs', 'action', 'adv', 'logp_old') + [
        ('clip', True, 0.2), ('idx', True, None), ('out', True, None), ('n_blocks', True, 0)]
    assert params(pkg.value_gradient_from_records) == pos('layout', 'rec', 'target', 'critic') + [('idx', True, None), ('out', True, None)]
    assert params(pkg.policy_gradient_from_records) == pos('layout', 'rec', 'adv', 'logp_old', 'policy') + [
        ('clip', True, 0.2), ('idx', True, None), ('out', True, None)]
    assert params(pkg.Gradients.to_module) == pos('self', 'net') + [('log_std', False, None)]
    assert pkg.value_gradient is fit.value_gradient and pkg.Gradients is fit.Gradients
    for name in ('flat', 'W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'log_std', 'stats', 'workspace'):
        assert hasattr(fit.Gradients(4, 2, fit._lf.PPO_CLIP, __import__('torch').float32, 'cpu', 16, None), name)
