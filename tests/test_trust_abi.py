"""CPU-only checks of libatacom_trust.so, the Fisher-vector product of a trust-region policy step: the header is plain C11, the
declared symbols are exactly the exported ones and the ctypes table, every argument rule is enforced without a GPU and with a
message, the kernel census is the sixteen product instantiations and the two reductions, the float32 kernels use no scratch
and run on the matrix cores, every kernel has the documented LDS, the exec-mask audit finds nothing and the Python signatures
are the documented ones (its row of the build tables: tests/test_trust_build.py).  No compute call is made (no GPU here)."""
import ctypes
import inspect
import re
import subprocess

import pytest

import abi_tools as abi

FUNCTIONS = ('version', 'last_error', 'workspace_size', 'fvp')


@pytest.fixture(scope='module')
def trust_lib():
    from rl_on_manifold_amd import build
    return build.build('trust', verbose=False)


def test_header_is_plain_c11(tmp_path):
    abi.compile_c11(tmp_path, abi.INCLUDE, '#include "atacom_trust_hip.h"\n'
                    'int main(void) {\n'
                    '    atacom_trust_args a = {0};\n'
                    '    a.struct_size = sizeof a; a.net.struct_size = sizeof a.net; a.net.hidden = ATACOM_TRUST_HIDDEN;\n'
                    '    a.damping = 1e-2;\n'
                    '    if (ATACOM_TRUST_MAX_IN != 32 || ATACOM_TRUST_MAX_OUT != 8 || ATACOM_TRUST_MAX_BLOCKS != 65535) return 1;\n'
                    '    if (atacom_trust_fvp(&a) == ATACOM_TRUST_OK || atacom_trust_workspace_size(&a) != 0) return 2;\n'
                    '    return !atacom_trust_version() || !atacom_trust_last_error(); }\n')


def test_declared_exported_and_bound_symbols_are_one_set(trust_lib):
    from rl_on_manifold_amd import _lib_trust
    names = abi.one_symbol_set(trust_lib, 'atacom_trust_hip.h', 'atacom_trust_', _lib_trust)
    assert names == sorted('atacom_trust_' + n for n in FUNCTIONS)
    assert _lib_trust.load().atacom_trust_version().startswith(b'atacom_trust')


def test_the_ctypes_struct_has_the_layout_of_the_header(tmp_path):
    """sizeof and the offset of every field, as gcc lays the header out."""
    from rl_on_manifold_amd import _lib_trust as lt
    fields = ('struct_size', 'device', 'dtype', 'n_blocks', 'n_outer', 'n_inner', 'net', 'x', 'idx', 'n_idx', 'v', 'damping', 'out',
              'workspace', 'workspace_bytes', 'stream')
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include "atacom_trust_hip.h"\nint main(void) { printf("%zu", sizeof(atacom_trust_args));\n' +
                   ''.join('    printf(" %%zu", offsetof(atacom_trust_args, %s));\n' % f for f in fields) +
                   '    printf(" %d %d %d %d\\n", ATACOM_TRUST_MAX_IN, ATACOM_TRUST_MAX_OUT, ATACOM_TRUST_HIDDEN, ATACOM_TRUST_MAX_BLOCKS);\n'
                   '    return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c11', '-I', abi.INCLUDE, str(src), '-o', exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    A = lt.TrustArgs
    assert got == [ctypes.sizeof(A)] + [getattr(A, f).offset for f in fields] + [lt.MAX_IN, lt.MAX_OUT, lt.HIDDEN, lt.MAX_BLOCKS]
    assert [f for f, _ in A._fields_] == list(fields)


X, V, OUT, WORK, IDX = 0x100000, 0x300000, 0x500000, 0x700000, 0x800000
P = 64 * 20 + 64 + 4096 + 64 + 64 * 2 + 2            # the network part of a direction of a 20 -> 2 policy


def _valid(lt, **net):
    """An argument struct that passes every check (its pointers are never dereferenced on the host): 3 x 5 rows of a 20 -> 2
    policy with std, x a column of [3, 5, 30] records, the rest contiguous."""
    a = lt.new_args()
    a.device, a.dtype, a.n_blocks, a.n_outer, a.n_inner, a.damping = 0, lt.F32, 0, 3, 5, 1e-2
    a.net = abi.fake_mlp(**dict(dict(std=0x1000), **net))
    a.x = lt.View(X, 150, 30)
    a.v, a.out, a.workspace, a.workspace_bytes = V, OUT, WORK, 4 * P + 256
    return a


def _apply(a, change):
    for k, val in change.items():
        obj = a
        *path, leaf = k.split('__')
        for part in path:
            obj = getattr(obj, part)
        setattr(obj, leaf, val)
    return a


def test_the_workspace_size_follows_the_documented_rule(trust_lib):
    from rl_on_manifold_amd import _lib_trust as lt
    lib = lt.load()
    up = lambda n: (n + 255) // 256 * 256                 # noqa: E731
    assert P == lt.net_size(20, 2) and lt.size(20, 2) == P + 2
    assert lib.atacom_trust_workspace_size(_valid(lt)) == up(4 * P)                                  # 15 rows: one workgroup
    assert lib.atacom_trust_workspace_size(_apply(_valid(lt), dict(dtype=lt.F64))) == up(8 * P)      # 15 rows of 16 a workgroup
    assert lib.atacom_trust_workspace_size(_apply(_valid(lt), dict(n_blocks=7))) == up(4 * 7 * P)
    assert lib.atacom_trust_workspace_size(_apply(_valid(lt), dict(n_outer=100, n_inner=100))) == up(4 * 40 * P)     # ceil(10000 / 256)
    assert lib.atacom_trust_workspace_size(_apply(_valid(lt), dict(n_outer=1000, n_inner=1000))) == up(4 * 512 * P)  # the ceiling
    assert lib.atacom_trust_workspace_size(_apply(_valid(lt), dict(n_outer=1000, n_inner=1000, idx=IDX, n_idx=257))) == up(4 * 2 * P)
    assert lib.atacom_trust_workspace_size(_apply(_valid(lt), dict(dtype=lt.F64, idx=IDX, n_idx=33))) == up(8 * 3 * P)
    assert lib.atacom_trust_workspace_size(_apply(_valid(lt), dict(dtype=lt.F64, n_outer=100, n_inner=100))) == up(8 * 512 * P)
    assert lib.atacom_trust_workspace_size(_apply(_valid(lt), dict(n_blocks=65536))) == 0
    assert 'atacom_trust_workspace_size' in lib.atacom_trust_last_error().decode() and 'launch grid' in lib.atacom_trust_last_error().decode()
    assert lib.atacom_trust_workspace_size(None) == 0


def test_arguments_are_validated_without_a_gpu(trust_lib):
    from rl_on_manifold_amd import _lib, _lib_trust as lt, AtacomError
    lib = lt.load()

    def msg():
        return lib.atacom_trust_last_error().decode()

    def refused(code, words, net=None, **change):
        a = _apply(_valid(lt, **(net or {})), change)
        assert lib.atacom_trust_fvp(a) == code, (change, net, msg())
        assert words in msg() and 'atacom_trust_fvp' in msg(), (change, net, msg())

    assert lib.atacom_trust_fvp(None) == lt.E_INVALID and 'null argument' in msg() and 'atacom_trust_fvp' in msg()
    refused(lt.E_INVALID, 'struct_size', struct_size=ctypes.sizeof(lt.TrustArgs) - 8)
    refused(lt.E_INVALID, 'net.struct_size', net__struct_size=ctypes.sizeof(_lib.AtacomMlp) - 4)
    refused(lt.E_INVALID, 'device', device=-1)
    refused(lt.E_UNSUPPORTED, 'no kernel for dtype 2', dtype=2)
    # sizes
    refused(lt.E_INVALID, 'n_outer must be >= 1', n_outer=0)
    refused(lt.E_INVALID, 'n_inner must be >= 1', n_inner=0)
    refused(lt.E_INVALID, 'n_blocks must be >= 1', n_blocks=-1)
    refused(lt.E_UNSUPPORTED, 'is too many', n_outer=2 ** 40, n_inner=2 ** 40)
    refused(lt.E_UNSUPPORTED, 'is too many (at most 2147483647 a call)', n_outer=2 ** 16, n_inner=2 ** 15)
    refused(lt.E_UNSUPPORTED, 'exceeds the launch grid', n_blocks=65536)
    refused(lt.E_INVALID, 'n_idx must be >= 1 with idx', idx=IDX, n_idx=0)
    refused(lt.E_UNSUPPORTED, 'n_idx = 2147483648 rows is too many', idx=IDX, n_idx=2 ** 31)
    # the network
    for n_in in (0, 33):
        refused(lt.E_UNSUPPORTED, 'n_in = %d is outside 1 .. 32' % n_in, net=dict(n_in=n_in))
    for n_out in (0, 9):
        refused(lt.E_UNSUPPORTED, 'n_out = %d is outside 1 .. 8' % n_out, net=dict(n_out=n_out))
    refused(lt.E_UNSUPPORTED, 'only 64 hidden units', net=dict(hidden=32))
    refused(lt.E_UNSUPPORTED, 'activation = 2', net=dict(activation=2))
    for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
        refused(lt.E_INVALID, 'null argument', net={k: None})
    # what the gradient library refuses is refused here, not ignored
    refused(lt.E_UNSUPPORTED, 'sigma network', net=dict(sW1=0x1000))
    refused(lt.E_UNSUPPORTED, 'squash', net=dict(squash=1))
    refused(lt.E_UNSUPPORTED, 'mean_mode', net=dict(mean_mode=1))
    refused(lt.E_UNSUPPORTED, 'explore', net=dict(explore=1))
    refused(lt.E_INVALID, 'null argument (net.std', net=dict(std=None))
    # the view, the direction, the outputs
    refused(lt.E_INVALID, 'null argument (x)', x__ptr=None)
    refused(lt.E_INVALID, 'null argument (v)', v=None)
    for k in ('out', 'workspace'):
        refused(lt.E_INVALID, 'null argument (out or workspace)', **{k: None})
    refused(lt.E_INVALID, 'damping must be >= 0', damping=-1e-3)
    refused(lt.E_INVALID, 'damping must be >= 0', damping=float('nan'))
    refused(lt.E_INVALID, 'damping must be >= 0', damping=float('inf'))
    refused(lt.E_INVALID, 'x.stride_inner = 19 is below the row width 20', x__stride_inner=19)
    refused(lt.E_INVALID, 'x.stride_outer = -19 is below the row width 20', x__stride_outer=-19)
    # every overlap: each output with each input, and the outputs with each other
    last_x = X + 4 * 439
    for out, span in (('out', 4 * (P + 2)), ('workspace', 4 * P)):
        refused(lt.E_INVALID, out + ' overlaps x', **{out: last_x})
        refused(lt.E_INVALID, out + ' overlaps x', **{out: X - span + 4})              # its last element is x's first
        refused(lt.E_INVALID, out + ' overlaps v', **{out: V + 4 * (P + 1)})           # the last v_ls
        refused(lt.E_INVALID, out + ' overlaps idx', **{out: IDX + 8 * 3, 'idx': IDX, 'n_idx': 4})
    refused(lt.E_INVALID, 'out overlaps workspace', workspace=OUT + 4 * (P + 1))
    refused(lt.E_INVALID, 'workspace_bytes = 22535 is below the 22784', workspace_bytes=4 * P - 1)
    # An input may repeat a row, a stride of a dimension of size 1 is not read, damping may be 0 and adjacent buffers do not
    # overlap: these pass every check and fail only at the device, which does not exist
    for change in (dict(x__stride_outer=0), dict(n_outer=1, x__stride_outer=3), dict(damping=0.0),
                   dict(idx=IDX, n_idx=1000, workspace_bytes=(4 * 4 * P + 255) // 256 * 256),
                   dict(out=V + 4 * (P + 2)), dict(out=X + 4 * 440), dict(workspace=OUT + 4 * (P + 2))):
        a = _apply(_valid(lt), change)
        a.device = 1 << 20                                          # no such device: nothing is launched either way
        assert lib.atacom_trust_fvp(a) == lt.E_HIP, (change, msg())
    a = _valid(lt)
    a.net.struct_size = _lib.AtacomMlp.mean_mode.offset             # ATACOM_MLP_SIZE_V1: accepted, the appended fields unread
    a.net.mean_mode, a.device = 1, 1 << 20
    assert lib.atacom_trust_fvp(a) == lt.E_HIP, msg()
    with pytest.raises(AtacomError, match='null argument'):
        lt.check(lib.atacom_trust_fvp(None))


def test_python_arguments_are_refused_before_the_library_is_called(monkeypatch):
    import torch
    from rl_on_manifold_amd import MlpPolicy, trust
    from rl_on_manifold_amd.rollout import CompactRecordLayout, RecordLayout

    def never(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(trust._lt, 'load', never)
    lin = lambda o, i: (torch.zeros(o, i), torch.zeros(o))          # noqa: E731
    pol = MlpPolicy(*lin(64, 4), *lin(64, 64), *lin(2, 64), std=torch.ones(2))
    nostd = MlpPolicy(*lin(64, 4), *lin(64, 64), *lin(2, 64))
    n = 64 * 4 + 64 + 4096 + 64 + 128 + 2 + 2
    x, v = torch.zeros(3, 5, 4), torch.zeros(n)
    lay, clay = RecordLayout([5], 4, 2), CompactRecordLayout([5], 4, 2, 3)
    idx = torch.zeros(4, dtype=torch.int64)
    w, ls = torch.zeros(3, 5), torch.zeros(2)
    for call, words in ((lambda: trust.fisher_vector_product(pol, x, v), 'run on a GPU'),
                        (lambda: trust.fisher_vector_product(pol, x, v, damping=0.1, idx=idx, n_blocks=3), 'run on a GPU'),
                        (lambda: trust.fisher_vector_product_from_records(lay, torch.zeros(3, 5, lay.F), v, pol), 'run on a GPU'),
                        (lambda: trust.fisher_vector_product_from_records(clay, torch.zeros(4, 5, clay.Fc), v, pol), 'run on a GPU'),
                        (lambda: trust.FisherProduct.like(pol, x), 'run on a GPU'),
                        (lambda: trust.natural_gradient(pol, x, v), 'run on a GPU'),
                        (lambda: trust.trpo_step(lay, torch.zeros(3, 5, lay.F), w, w, pol, ls), 'run on a GPU'),
                        (lambda: trust.fisher_vector_product(pol, 3.0, v), r'\[\.\.\., n_in\]'),
                        (lambda: trust.fisher_vector_product(pol, x.to(torch.float16), v), 'float32 or float64'),
                        (lambda: trust.fisher_vector_product(nostd, x, v), 'a policy with std'),
                        (lambda: trust.fisher_vector_product(pol, x, v, damping=-1.0), 'damping must be >= 0'),
                        (lambda: trust.fisher_vector_product(pol, x, v, damping=float('nan')), 'damping must be >= 0'),
                        (lambda: trust.fisher_vector_product(pol, torch.zeros(3, 5, 5), v), 'rows of 5 where the network takes 4'),
                        (lambda: trust.fisher_vector_product(pol, torch.zeros(3, 0, 4), v), 'holds no rows'),
                        (lambda: trust.fisher_vector_product(pol, x, v[:-1]), 'v must be a one-dimensional tensor of %d values' % n),
                        (lambda: trust.fisher_vector_product(pol, x, v.double()), 'v must be contiguous, torch.float32'),
                        (lambda: trust.fisher_vector_product(pol, x, torch.zeros(2 * n)[::2]), 'v must be contiguous'),
                        (lambda: trust.fisher_vector_product(pol, torch.zeros(3, 5, 8)[..., ::2], v), 'must be contiguous'),
                        (lambda: trust.fisher_vector_product(pol, torch.zeros(2, 4, 8, 4)[:, :3, :5], v), 'do not collapse'),
                        (lambda: trust.fisher_vector_product(pol, x, v, idx=idx.int()), 'idx must be a one-dimensional int64'),
                        (lambda: trust.fisher_vector_product(pol, x, v, idx=idx[:0]), 'at least one row number'),
                        (lambda: trust.fisher_vector_product(pol, x, v, n_blocks=65536), 'n_blocks must be 0'),
                        (lambda: trust.fisher_vector_product(pol, x, v, out=torch.zeros(n)), 'out must be the FisherProduct'),
                        (lambda: trust.fisher_vector_product_from_records(lay, torch.zeros(3, 5, lay.F + 1), v, pol), 'records must be'),
                        (lambda: trust.fisher_vector_product_from_records(clay, torch.zeros(3, 5, clay.Fc), v, pol), 'rows of time'),
                        (lambda: trust.natural_gradient(pol, x, v, iters=0), 'iters must be an integer >= 1'),
                        (lambda: trust.natural_gradient(pol, x, v, work=3), 'work must be a CgWork'),
                        (lambda: trust.trpo_step(lay, torch.zeros(3, 5, lay.F), w, w, pol, ls, line_search=0), 'line_search must be'),
                        (lambda: trust.trpo_step(lay, torch.zeros(3, 5, lay.F), w, w, pol, ls, max_kl=0.0), 'max_kl must be > 0'),
                        (lambda: trust.trpo_step(lay, torch.zeros(3, 5, lay.F), w, w, pol, ls.double()), 'log_std must be a contiguous'),
                        (lambda: trust.trpo_step(lay, torch.zeros(3, 5, lay.F), w, w, nostd, ls), 'std must be a contiguous'),
                        (lambda: trust.trpo_step(lay, torch.zeros(3, 5, lay.F), w, w, pol, torch.zeros(3)), r'log_std must have the shape \(2,\)')):
        with pytest.raises(ValueError, match=words):
            call()
    p = trust.FisherProduct(4, 2, torch.float32, 'cpu', 256, None)
    assert p.flat.numel() == n and p.log_std.shape == (2,) and p.W3.shape == (2, 64) and p.W1.data_ptr() == p.flat.data_ptr()
    assert p.b3.data_ptr() == p.flat.data_ptr() + 4 * (64 * 4 + 64 + 4096 + 64 + 128)
    assert p.log_std.data_ptr() == p.flat.data_ptr() + 4 * (n - 2) and p.W2.shape == (64, 64)


@abi.needs_llvm('llvm-readelf')
def test_kernel_census_and_resources(trust_lib, tmp_path):
    """Eighteen kernels: k_trust_fvp<T, CH> for CH = ceil(n_in / 4) = 1 .. 8 and k_trust_reduce<T>.  Float32: no scratch, at
    most the 512 registers of one wavefront per SIMD (the launch bound), and 94816 bytes of LDS -- two network blocks
    MlpLdsM<.., 64, 8>::NET = 7752 floats (the weights, the direction), 8 for std^2, and 4 wavefronts x 2048 of staging (two
    [16][64] transposition buffers).  Float64: 16 records of 393 + 4 CH doubles."""
    ks = abi.kernel_rows(trust_lib, tmp_path)
    want = ['k_trust_fvp<%s, %d>' % (t, ch) for t in ('float', 'double') for ch in range(1, 9)] + ['k_trust_reduce<float>', 'k_trust_reduce<double>']
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
            assert lds == 4 * (2 * 7752 + 8 + 4 * 2048) == 94816, (name, lds)
        else:
            assert lds == 8 * 16 * (393 + 4 * ch), (name, lds)


@abi.needs_llvm('llvm-objdump')
def test_the_float32_kernels_run_on_the_matrix_cores(trust_lib, tmp_path):
    seen = 0
    for _, head, body in abi.function_bodies(trust_lib, tmp_path):
        k = re.search(r'k_trust_(fvp<(float|double), (\d)>|reduce<(float|double)>)', head)
        if not k:
            continue
        seen += 1
        mfma = len(re.findall(r'\bv_mfma_f32_16x16x4[_f32]*\b', body))
        if k.group(2) == 'float':
            # per block of 16 rows: forward 4 CH + 64; tangent 4 CH + 128 + 32; W3^T dy 8, W2^T da2 64; dW3 16, dW2 64, dW1 16
            # per tile of 16 inputs
            ch = int(k.group(3))
            assert mfma == 8 * ch + 64 + 128 + 32 + 8 + 64 + 16 + 64 + 16 * (2 if 4 * ch > 16 else 1), (head, mfma)
        else:
            assert mfma == 0, (head, mfma)
    assert seen == 18


def test_exec_mask_audit_finds_nothing(trust_lib):
    abi.exec_audit(trust_lib)


def test_python_surface():
    import rl_on_manifold_amd as pkg
    from rl_on_manifold_amd import trust

    def params(fn):
        return [(p.name, p.kind is p.KEYWORD_ONLY, None if p.default is p.empty else p.default)
                for p in inspect.signature(fn).parameters.values()]

    pos = lambda *names: [(n, False, None) for n in names]          # noqa: E731
    assert params(pkg.fisher_vector_product) == pos('policy', 'obs', 'v') + [
        ('damping', True, 0.0), ('idx', True, None), ('out', True, None), ('n_blocks', True, 0)]
    assert params(pkg.fisher_vector_product_from_records) == pos('layout', 'rec', 'v', 'policy') + [
        ('damping', True, 0.0), ('idx', True, None), ('out', True, None), ('n_blocks', True, 0)]
    assert params(pkg.natural_gradient) == pos('policy', 'obs', 'g') + [
        ('iters', True, 10), ('damping', True, 1e-2), ('residual_tol', True, 1e-10), ('idx', True, None), ('work', True, None)]
    assert params(pkg.trpo_step) == pos('layout', 'rec', 'adv', 'logp_old', 'policy', 'log_std') + [
        ('max_kl', True, 1e-2), ('ent_coeff', True, 0.0), ('cg_iters', True, 10), ('cg_damping', True, 1e-2),
        ('cg_residual_tol', True, 1e-10), ('line_search', True, 10)]
    assert pkg.fisher_vector_product is trust.fisher_vector_product and pkg.trpo_step is trust.trpo_step
    assert pkg.FisherProduct is trust.FisherProduct and pkg.CgWork is trust.CgWork
