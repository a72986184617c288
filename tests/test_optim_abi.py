"""CPU-only checks of libatacom_optim.so, the Adam step with its state on the device: the header is plain C11, the declared
symbols are exactly the exported ones and the ctypes table, the ctypes structs have gcc's layout, the size of a state follows
the documented rule, every argument rule is enforced without a GPU and with a message, the Python layer refuses what would be
updated as a copy, the kernel census is the two steps and the one kernel of init, no kernel uses scratch, the exec-mask audit
finds nothing and the Python signatures are the documented ones (its row of the build tables: tests/test_optim_build.py).  No
compute call is made (no GPU here)."""
import ctypes
import inspect
import subprocess

import pytest

import abi_tools as abi

FUNCTIONS = ('version', 'last_error', 'state_size', 'adam_init', 'adam_step')


@pytest.fixture(scope='module')
def optim_lib():
    from rl_on_manifold_amd import build
    return build.build('optim', verbose=False)


def test_header_is_plain_c11(tmp_path):
    abi.compile_c11(tmp_path, abi.INCLUDE, '#include "atacom_optim_hip.h"\n'
                    'int main(void) {\n'
                    '    atacom_optim_args a = {0};\n'
                    '    a.struct_size = sizeof a; a.n_groups = 1; a.groups[0].n_in = 4; a.groups[0].n_out = 1;\n'
                    '    if (ATACOM_OPTIM_MAX_IN != 32 || ATACOM_OPTIM_MAX_OUT != 8 || ATACOM_OPTIM_MAX_GROUPS != 4 || ATACOM_OPTIM_HEAD != 32) return 1;\n'
                    '    if (atacom_optim_adam_step(&a) == ATACOM_OPTIM_OK || atacom_optim_adam_init(&a) == ATACOM_OPTIM_OK) return 2;\n'
                    '    if (atacom_optim_state_size(ATACOM_OPTIM_F32, 4, 1, 0) == 0) return 3;\n'
                    '    return !atacom_optim_version() || !atacom_optim_last_error(); }\n')


def test_declared_exported_and_bound_symbols_are_one_set(optim_lib):
    from rl_on_manifold_amd import _lib_optim
    names = abi.one_symbol_set(optim_lib, 'atacom_optim_hip.h', 'atacom_optim_', _lib_optim)
    assert names == sorted('atacom_optim_' + n for n in FUNCTIONS) and len(names) == 5
    assert _lib_optim.load().atacom_optim_version().startswith(b'atacom_optim')


def test_the_ctypes_structs_have_the_layout_of_the_header(tmp_path):
    from rl_on_manifold_amd import _lib_optim as lo
    gf = [f for f, _ in lo.Group._fields_]
    af = [f for f, _ in lo.OptimArgs._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include "atacom_optim_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu", sizeof(atacom_optim_group), sizeof(atacom_optim_args));\n' +
                   ''.join('    printf(" %%zu", offsetof(atacom_optim_group, %s));\n' % f for f in gf) +
                   ''.join('    printf(" %%zu", offsetof(atacom_optim_args, %s));\n' % f for f in af) +
                   '    printf(" %d %d %d %d %d\\n", ATACOM_OPTIM_MAX_GROUPS, ATACOM_OPTIM_MAX_IN, ATACOM_OPTIM_MAX_OUT, ATACOM_OPTIM_HIDDEN,\n'
                   '           ATACOM_OPTIM_HEAD); return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c11', '-I', abi.INCLUDE, str(src), '-o', exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(lo.Group), ctypes.sizeof(lo.OptimArgs)] + [getattr(lo.Group, f).offset for f in gf] + \
        [getattr(lo.OptimArgs, f).offset for f in af] + [lo.MAX_GROUPS, lo.MAX_IN, lo.MAX_OUT, lo.HIDDEN, lo.HEAD]
    assert len(gf) == 14 and len(af) == 9


def test_the_state_size_follows_the_documented_rule(optim_lib):
    from rl_on_manifold_amd import _lib_optim as lo
    lib = lo.load()
    assert lo.group_size(1, 1, False) == 4353 and lo.group_size(32, 8, True) == 6800
    for n_in, n_out in ((1, 1), (25, 1), (18, 5), (32, 8)):
        for has in (0, 1):
            N = 64 * n_in + 64 + 4096 + 64 + 64 * n_out + n_out + has * n_out
            assert N == lo.group_size(n_in, n_out, has)
            assert lib.atacom_optim_state_size(lo.F32, n_in, n_out, has) == 32 + 8 * N
            assert lib.atacom_optim_state_size(lo.F64, n_in, n_out, has) == 32 + 16 * N
    for args, words in (((2, 4, 1, 0), 'no kernel for dtype 2'), ((0, 0, 1, 0), 'n_in = 0 is outside 1 .. 32'),
                        ((0, 33, 1, 0), 'n_in = 33'), ((0, 4, 0, 1), 'n_out = 0 is outside 1 .. 8'), ((1, 4, 9, 1), 'n_out = 9')):
        assert lib.atacom_optim_state_size(*args) == 0
        assert words in lib.atacom_optim_last_error().decode() and 'atacom_optim_state_size' in lib.atacom_optim_last_error().decode()


BASE = 0x10000000
N_P, N_C = 64 * 20 + 64 + 4096 + 64 + 128 + 2 + 2, 64 * 20 + 64 + 4096 + 64 + 64 + 1


def _valid(lo):
    """An argument struct that passes every check (its pointers are never dereferenced on the host): float32, a 20 -> 2 policy
    with log_std and std and a 20 -> 1 critic with grad_scale 0.5, every buffer 1 MiB from the next."""
    a = lo.new_args()
    a.device, a.dtype, a.n_groups, a.beta1, a.beta2, a.eps = 0, lo.F32, 2, 0.9, 0.999, 1e-8
    at = BASE
    for g, (n_out, has, scale) in zip(a.groups, ((2, True, 1.0), (1, False, 0.5))):
        g.n_in, g.n_out, g.lr, g.grad_scale = 20, n_out, 3e-4, scale
        for k in lo.PARAMS + (('log_std', 'std') if has else ()) + ('grad', 'state'):
            setattr(g, k, at)
            at += 1 << 20
    return a


def _apply(a, change):
    for k, val in change.items():
        obj = a
        *path, leaf = k.split('__')
        for part in path:
            obj = obj[int(part[1:])] if part[0] == 'g' and part[1:].isdigit() else getattr(obj, part)
        setattr(obj, leaf, val)
    return a


def test_arguments_are_validated_without_a_gpu(optim_lib):
    from rl_on_manifold_amd import _lib_optim as lo, AtacomError
    lib = lo.load()

    def msg():
        return lib.atacom_optim_last_error().decode()

    def refused(code, words, both=True, **change):
        for fn in ('atacom_optim_adam_step', 'atacom_optim_adam_init') if both else ('atacom_optim_adam_step',):
            a = _apply(_valid(lo), change)
            assert getattr(lib, fn)(a) == code, (fn, change, msg())
            assert words in msg() and fn in msg(), (fn, change, msg())

    G0 = _valid(lo).groups[0]
    assert lib.atacom_optim_adam_step(None) == lo.E_INVALID and 'null argument' in msg() and 'atacom_optim_adam_step' in msg()
    assert lib.atacom_optim_adam_init(None) == lo.E_INVALID and 'atacom_optim_adam_init' in msg()
    refused(lo.E_INVALID, 'struct_size', struct_size=ctypes.sizeof(lo.OptimArgs) - 8)
    refused(lo.E_INVALID, 'device', device=-1)
    for n in (0, 5, -1):
        refused(lo.E_INVALID, 'n_groups = %d is outside 1 .. 4' % n, n_groups=n)
    refused(lo.E_UNSUPPORTED, 'no kernel for dtype 2', dtype=2)
    for n_in in (0, 33):
        refused(lo.E_UNSUPPORTED, 'groups[1]: n_in = %d is outside 1 .. 32' % n_in, groups__g1__n_in=n_in)
    for n_out in (0, 9):
        refused(lo.E_UNSUPPORTED, 'groups[0]: n_out = %d is outside 1 .. 8' % n_out, groups__g0__n_out=n_out)
    for k in lo.PARAMS:
        refused(lo.E_INVALID, 'groups[0]: null argument (a weight or bias', **{'groups__g0__' + k: None})
    refused(lo.E_INVALID, 'groups[1]: null argument (grad or state)', both=False, groups__g1__grad=None)
    refused(lo.E_INVALID, 'groups[1]: null argument (grad or state)', groups__g1__state=None)
    refused(lo.E_INVALID, 'groups[1]: std without log_std', groups__g1__std=BASE + (100 << 20))
    for lr in (-1e-3, float('inf'), float('nan')):
        refused(lo.E_INVALID, 'groups[0]: lr must be >= 0 and finite', groups__g0__lr=lr)
    for name in ('beta1', 'beta2'):
        for b in (-0.1, 1.0, 1.5, float('nan')):
            refused(lo.E_INVALID, name + ' must be in [0, 1)', **{name: b})
    for eps in (0.0, -1e-8, float('inf'), float('nan')):
        refused(lo.E_INVALID, 'eps must be > 0 and finite', eps=eps)
    for s in (float('inf'), float('nan')):
        refused(lo.E_INVALID, 'groups[1]: grad_scale must be finite', groups__g1__grad_scale=s)
    refused(lo.E_INVALID, 'groups[0]: state must be aligned to 8 bytes', groups__g0__state=G0.state + 4)
    refused(lo.E_INVALID, 'groups[0]: W2 must be aligned to the dtype', groups__g0__W2=G0.W2 + 2)
    # overlaps inside a group: each parameter's last byte with the next buffer, grad, state and std
    refused(lo.E_INVALID, 'groups[0].W1 overlaps groups[0].b1', groups__g0__b1=G0.W1 + 4 * (64 * 20 - 1))
    refused(lo.E_INVALID, 'groups[0].W2 overlaps groups[0].grad', both=False, groups__g0__grad=G0.W2 - 4 * (N_P - 1))
    refused(lo.E_INVALID, 'groups[0].b3 overlaps groups[0].state', groups__g0__state=G0.b3 - (32 + 8 * N_P) + 8)
    refused(lo.E_INVALID, 'groups[0].log_std overlaps groups[0].std', groups__g0__std=G0.log_std + 4)
    refused(lo.E_INVALID, 'groups[0].grad overlaps groups[0].state', both=False, groups__g0__state=G0.grad + 4 * N_P - 8)
    refused(lo.E_INVALID, 'groups[0].std overlaps groups[0].grad', both=False, groups__g0__grad=G0.std + 4)
    # and across groups: two groups that name the same parameter, one gradient or one state
    refused(lo.E_INVALID, 'groups[0].W3 overlaps groups[1].W3', groups__g1__W3=G0.W3)
    refused(lo.E_INVALID, 'groups[0].b2 overlaps groups[1].W1', groups__g1__W1=G0.b2 + 4 * 63)
    refused(lo.E_INVALID, 'groups[0].grad overlaps groups[1].grad', both=False, groups__g1__grad=G0.grad + 4 * (N_P - 1))
    refused(lo.E_INVALID, 'groups[0].state overlaps groups[1].state', groups__g1__state=G0.state + 32 + 8 * N_P - 8)
    refused(lo.E_INVALID, 'groups[0].state overlaps groups[1].grad', both=False, groups__g1__grad=G0.state)
    # What passes every check fails only at the device, which does not exist: adjacent buffers, a group without std, lr = 0,
    # beta = 0, one group, init without a gradient, float64
    for change in (dict(), dict(groups__g0__b1=G0.W1 + 4 * 64 * 20), dict(groups__g0__std=None), dict(groups__g0__lr=0.0),
                   dict(beta1=0.0, beta2=0.0), dict(n_groups=1), dict(groups__g1__state=G0.state + 32 + 8 * N_P),
                   dict(dtype=lo.F64), dict(groups__g1__grad_scale=-2.0)):
        a = _apply(_valid(lo), change)
        a.device = 1 << 20                                          # no such device: nothing is launched either way
        assert lib.atacom_optim_adam_step(a) == lo.E_HIP, (change, msg())
        assert lib.atacom_optim_adam_init(a) == lo.E_HIP, (change, msg())
    a = _apply(_valid(lo), dict(groups__g0__grad=None, groups__g1__grad=None))
    a.device = 1 << 20
    assert lib.atacom_optim_adam_init(a) == lo.E_HIP, msg()
    with pytest.raises(AtacomError, match='null argument'):
        lo.check(lib.atacom_optim_adam_step(None))


def test_python_arguments_are_refused_before_the_library_is_called():
    torch = pytest.importorskip('torch')
    from rl_on_manifold_amd import Adam, GraphedUpdate, MlpPolicy
    lin = lambda o, i, dt=torch.float32: (torch.zeros(o, i, dtype=dt), torch.zeros(o, dtype=dt))          # noqa: E731
    net = lambda n_in, n_out, dt=torch.float32, **kw: MlpPolicy(*lin(64, n_in, dt), *lin(64, 64, dt), *lin(n_out, 64, dt), **kw)   # noqa: E731
    pol, cri = net(4, 2, std=torch.ones(2)), net(4, 1)
    ls, std = torch.zeros(2), pol.tensors['std']
    strided = net(4, 2)
    strided.tensors['W2'] = torch.zeros(64, 128)[:, ::2]
    numpy_net = net(4, 1)
    numpy_net.tensors['b1'] = [0.0] * 64
    wide = MlpPolicy(*lin(64, 33), *lin(64, 64), *lin(1, 64))
    wrong = MlpPolicy(*lin(32, 4), *lin(32, 32), *lin(1, 32))
    mixed = net(4, 1)
    mixed.tensors['b3'] = torch.zeros(1, dtype=torch.float64)
    for call, words in ((lambda: Adam([dict(net=pol, log_std=ls, std=std), dict(net=cri, scale=0.5)]), 'run on a GPU'),
                        (lambda: Adam([dict(net=net(4, 1, torch.float64))]), 'run on a GPU'),
                        (lambda: Adam([]), 'a list of 1 .. 4 dicts'),
                        (lambda: Adam([dict(net=cri)] * 5), 'a list of 1 .. 4 dicts'),
                        (lambda: Adam(dict(net=cri)), 'a list of 1 .. 4 dicts'),
                        (lambda: Adam([cri]), "a dict with the key 'net'"),
                        (lambda: Adam([dict(net=cri, weight_decay=0.1)]), "a dict with the key 'net'"),
                        (lambda: Adam([dict(net=torch.nn.Linear(4, 1))]), 'net must be an MlpPolicy'),
                        (lambda: Adam([dict(net=cri)], lr=-1.0), 'lr must be >= 0'),
                        (lambda: Adam([dict(net=cri, lr=float('nan'))]), r'groups\[0\]: lr must be >= 0'),
                        (lambda: Adam([dict(net=cri)], betas=(0.9, 1.0)), 'betas must be two numbers'),
                        (lambda: Adam([dict(net=cri)], betas=0.9), 'betas must be two numbers'),
                        (lambda: Adam([dict(net=cri)], eps=0.0), 'eps must be > 0'),
                        (lambda: Adam([dict(net=cri, scale=float('inf'))]), 'scale must be finite'),
                        (lambda: Adam([dict(net=pol, std=std)]), 'std without log_std'),
                        (lambda: Adam([dict(net=numpy_net)]), 'must be tensors'),
                        (lambda: Adam([dict(net=wide)]), 'a 33 -> 1 network is outside'),
                        (lambda: Adam([dict(net=wrong)]), r'W1 must be a tensor of shape \(64, 4\)'),
                        (lambda: Adam([dict(net=pol, log_std=torch.zeros(3))]), r'log_std must be a tensor of shape \(2,\)'),
                        (lambda: Adam([dict(net=pol, log_std=ls, std=torch.ones(2, 1))]), 'std must be a tensor of shape'),
                        (lambda: Adam([dict(net=net(4, 1, torch.float16))]), 'float32 or float64'),
                        (lambda: Adam([dict(net=mixed)]), 'b3 is torch.float64 on cpu where the first parameter is torch.float32'),
                        (lambda: Adam([dict(net=cri), dict(net=net(4, 1, torch.float64))]), r'groups\[1\]: W1 is torch.float64'),
                        (lambda: Adam([dict(net=strided)]), 'W2 must be contiguous'),
                        (lambda: GraphedUpdate(None, None, None, None, None, pol, cri, torch.optim.Adam([ls]), 64), 'an Adam of two groups')):
        with pytest.raises(ValueError, match=words):
            call()


@abi.needs_llvm('llvm-readelf')
def test_kernel_census_and_resources(optim_lib, tmp_path):
    """Three kernels: k_adam<T> for the two dtypes and k_adam_init, which serves both.  None uses scratch; k_adam holds the
    seven broadcast scalars (eight slots) in LDS, k_adam_init none; 1024 threads a workgroup leave a thread 128 registers."""
    ks = abi.kernel_rows(optim_lib, tmp_path)
    assert [k[0].split('(')[0] for k in ks] == sorted(['k_adam<float>', 'k_adam<double>', 'k_adam_init']), ks
    for name, lds, scratch, vgpr, agpr, code in ks:
        print('%-28s VGPR %3d AGPR %3d scratch %d LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        assert scratch == 0, (name, scratch)
        assert vgpr <= 128, (name, vgpr)
        assert lds == (0 if 'init' in name else 8 * (8 if 'double' in name else 4)), (name, lds)


def test_exec_mask_audit_finds_nothing(optim_lib):
    abi.exec_audit(optim_lib)


def test_python_surface():
    import rl_on_manifold_amd as pkg
    from rl_on_manifold_amd import optim

    def params(fn):
        return [(p.name, None if p.default is p.empty else p.default) for p in inspect.signature(fn).parameters.values()]

    pos = lambda *names: [(n, None) for n in names]          # noqa: E731
    assert params(pkg.Adam.__init__) == pos('self', 'groups') + [('lr', 3e-4), ('betas', (0.9, 0.999)), ('eps', 1e-8)]
    assert params(pkg.GraphedUpdate.__init__) == pos('self', 'layout', 'rec', 'adv', 'ret', 'logp_old', 'policy', 'critic', 'optimizer',
                                                     'minibatch') + [('clip', 0.2), ('warmup', 2)]
    assert params(pkg.GraphedUpdate.replay) == pos('self') + [('perm', None)]
    assert [p.kind for p in inspect.signature(pkg.Adam.step).parameters.values()][1] is inspect.Parameter.VAR_POSITIONAL
    assert params(pkg.Adam.restore) == pos('self', 's') and params(pkg.Adam.snapshot) == pos('self') == params(pkg.Adam.steps)
    assert pkg.Adam is optim.Adam and pkg.GraphedUpdate is optim.GraphedUpdate
    assert 'baked into the graph' in optim.GraphedUpdate.__doc__.lower()
