"""CPU-only checks of libatacom_offstep.so, the Adam step of an off-policy update with the target networks' soft update in its
launch: the header is plain C11, the declared symbols are exactly the exported ones and the ctypes table, the ctypes structs have
gcc's layout, the size of a state follows the documented rule, every refusal the header lists is made without a GPU, with
ATACOM_OFFSTEP_E_INVALID and a message, the Python layer refuses what would be updated as a copy, the kernel census is the two
steps and the one kernel of init, no kernel uses scratch, and the Python signatures are the documented ones (its row of the build
tables: tests/test_offstep_build.py).  No compute call is made (no GPU here)."""
import ctypes
import inspect
import subprocess

import pytest

import abi_tools as abi

FUNCTIONS = ('version', 'last_error', 'state_size', 'adam_init', 'adam_step')


@pytest.fixture(scope='module')
def offstep_lib():
    from rl_on_manifold_amd import build
    return build.build('offstep', verbose=False)


def test_header_is_plain_c11(tmp_path):
    abi.compile_c11(tmp_path, abi.INCLUDE, '#include "atacom_offstep_hip.h"\n'
                    'int main(void) {\n'
                    '    atacom_offstep_args a = {0};\n'
                    '    a.struct_size = sizeof a; a.n_groups = 1; a.groups[0].n_in = 4; a.groups[0].n_out = 1; a.groups[0].n_act = 2;\n'
                    '    if (ATACOM_OFFSTEP_MAX_IN != 32 || ATACOM_OFFSTEP_MAX_OUT != 8 || ATACOM_OFFSTEP_MAX_ACT != 8) return 1;\n'
                    '    if (ATACOM_OFFSTEP_MAX_GROUPS != 4 || ATACOM_OFFSTEP_HEAD != 32 || ATACOM_OFFSTEP_TENSORS != 7) return 1;\n'
                    '    if (atacom_offstep_adam_step(&a) == ATACOM_OFFSTEP_OK || atacom_offstep_adam_init(&a) == ATACOM_OFFSTEP_OK) return 2;\n'
                    '    if (atacom_offstep_state_size(ATACOM_OFFSTEP_F32, 4, 1, 2) == 0) return 3;\n'
                    '    return !atacom_offstep_version() || !atacom_offstep_last_error(); }\n')


def test_declared_exported_and_bound_symbols_are_one_set(offstep_lib):
    from rl_on_manifold_amd import _lib_offstep
    names = abi.one_symbol_set(offstep_lib, 'atacom_offstep_hip.h', 'atacom_offstep_', _lib_offstep)
    assert names == sorted('atacom_offstep_' + n for n in FUNCTIONS) and len(names) == 5
    assert _lib_offstep.load().atacom_offstep_version().startswith(b'atacom_offstep')


def test_the_ctypes_structs_have_the_layout_of_the_header(tmp_path):
    from rl_on_manifold_amd import _lib_offstep as ls
    gf = [f for f, _ in ls.Group._fields_]
    af = [f for f, _ in ls.OffstepArgs._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include "atacom_offstep_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu", sizeof(atacom_offstep_group), sizeof(atacom_offstep_args));\n' +
                   ''.join('    printf(" %%zu", offsetof(atacom_offstep_group, %s));\n' % f for f in gf) +
                   ''.join('    printf(" %%zu", offsetof(atacom_offstep_args, %s));\n' % f for f in af) +
                   '    printf(" %zu", sizeof(((atacom_offstep_group*)0)->target));\n'
                   '    printf(" %d %d %d %d %d %d %d\\n", ATACOM_OFFSTEP_MAX_GROUPS, ATACOM_OFFSTEP_MAX_IN, ATACOM_OFFSTEP_MAX_OUT,\n'
                   '           ATACOM_OFFSTEP_MAX_ACT, ATACOM_OFFSTEP_HIDDEN, ATACOM_OFFSTEP_TENSORS, ATACOM_OFFSTEP_HEAD); return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c11', '-I', abi.INCLUDE, str(src), '-o', exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(ls.Group), ctypes.sizeof(ls.OffstepArgs)] + [getattr(ls.Group, f).offset for f in gf] + \
        [getattr(ls.OffstepArgs, f).offset for f in af] + [ls.Group.target.size] + \
        [ls.MAX_GROUPS, ls.MAX_IN, ls.MAX_OUT, ls.MAX_ACT, ls.HIDDEN, ls.TENSORS, ls.HEAD]
    assert len(gf) == 16 and len(af) == 10
    assert gf[4:11] == list(ls.PARAMS)
    from rl_on_manifold_amd import _lib_offpolicy, offgrad
    assert ls.PARAMS == _lib_offpolicy.PARAMS == offgrad.PARAMS          # one order: a pair of soft_update, QGradients.flat, a group


# (n_in, n_out, n_act): the smallest and the largest plain network, a point-sized DDPG critic, the largest critic
CORNERS = ((1, 1, 0), (32, 8, 0), (3, 1, 1), (32, 1, 8))


def test_the_state_size_follows_the_documented_rule(offstep_lib):
    from rl_on_manifold_amd import _lib_offstep as ls, _lib_optim as lo, _lib_offgrad as lg
    lib = ls.load()
    assert ls.group_size(1, 1, 0) == 4353 and ls.group_size(32, 8, 0) == 6792 and ls.group_size(32, 1, 8) == 6849
    for n_in, n_out, n_act in CORNERS + ((25, 1, 0), (18, 5, 3), (32, 8, 8)):
        N = 64 * n_in + 64 + 4096 + 64 + 64 * n_out + n_out + 64 * n_act
        assert N == ls.group_size(n_in, n_out, n_act)
        assert lib.atacom_offstep_state_size(ls.F32, n_in, n_out, n_act) == 32 + 8 * N
        assert lib.atacom_offstep_state_size(ls.F64, n_in, n_out, n_act) == 32 + 16 * N
        if n_act == 0:                                       # the order and size of fit.Gradients.flat without log std
            assert N == lo.group_size(n_in, n_out, False)
        elif n_out == 1:                                     # and of QGradients.flat
            assert N == lg.grad_size(n_in, 1, n_act)
    for args, words in (((2, 4, 1, 0), 'no kernel for dtype 2'), ((-1, 4, 1, 0), 'no kernel for dtype -1'),
                        ((0, 0, 1, 0), 'n_in = 0 is outside 1 .. 32'), ((0, 33, 1, 0), 'n_in = 33'),
                        ((0, 4, 0, 1), 'n_out = 0 is outside 1 .. 8'), ((1, 4, 9, 1), 'n_out = 9'),
                        ((0, 4, 1, -1), 'n_act = -1 is outside 0 .. 8'), ((1, 4, 1, 9), 'n_act = 9')):
        assert lib.atacom_offstep_state_size(*args) == 0
        assert words in lib.atacom_offstep_last_error().decode() and 'atacom_offstep_state_size' in lib.atacom_offstep_last_error().decode()


BASE = 0x10000000
N_A, N_Q = 64 * 20 + 64 + 4096 + 64 + 128 + 2, 64 * 22 + 64 + 4096 + 64 + 64 + 1 + 128


def _valid(ls):
    """An argument struct that passes every check (its pointers are never dereferenced on the host): float32, a 20 -> 2 actor
    and a TD3 critic of 22 first-layer inputs and 2 action columns, both with a target and a gradient, every buffer 1 MiB from
    the next."""
    a = ls.new_args()
    a.device, a.dtype, a.n_groups, a.beta1, a.beta2, a.eps, a.tau = 0, ls.F32, 2, 0.9, 0.999, 1e-8, 5e-3
    at = BASE
    for g, (n_in, n_out, n_act, lr) in zip(a.groups, ((20, 2, 0, 1e-4), (22, 1, 2, 3e-4))):
        g.n_in, g.n_out, g.n_act, g.lr, g.grad_scale = n_in, n_out, n_act, lr, 1.0
        for j, k in enumerate(ls.PARAMS[:7 if n_act else 6]):
            setattr(g, k, at)
            g.target[j] = at + (1 << 20)
            at += 2 << 20
        for k in ('grad', 'state'):
            setattr(g, k, at)
            at += 1 << 20
    return a


def _apply(a, change):
    for k, val in change.items():
        obj = a
        *path, leaf = k.split('__')
        for part in path:
            obj = obj[int(part[1:])] if part[0] == 'g' and part[1:].isdigit() else getattr(obj, part)
        if leaf[0] == 't' and leaf[1:].isdigit():
            obj.target[int(leaf[1:])] = val
        else:
            setattr(obj, leaf, val)
    return a


def test_arguments_are_validated_without_a_gpu(offstep_lib):
    from rl_on_manifold_amd import _lib_offstep as ls, AtacomError
    lib = ls.load()

    def msg():
        return lib.atacom_offstep_last_error().decode()

    def refused(words, **change):
        for fn in ('atacom_offstep_adam_step', 'atacom_offstep_adam_init'):
            a = _apply(_valid(ls), change)
            assert getattr(lib, fn)(a) == ls.E_INVALID, (fn, change, msg())
            assert words in msg() and fn in msg(), (fn, change, msg())

    G0, G1 = _valid(ls).groups[0], _valid(ls).groups[1]
    T0 = [G0.target[j] for j in range(7)]
    assert lib.atacom_offstep_adam_step(None) == ls.E_INVALID and 'null argument' in msg() and 'atacom_offstep_adam_step' in msg()
    assert lib.atacom_offstep_adam_init(None) == ls.E_INVALID and 'atacom_offstep_adam_init' in msg()
    refused('struct_size', struct_size=ctypes.sizeof(ls.OffstepArgs) - 8)
    refused('struct_size', struct_size=0)
    refused('device', device=-1)
    for n in (0, 5, -1):
        refused('n_groups = %d is outside 1 .. 4' % n, n_groups=n)
    for dt in (2, -1):
        refused('no kernel for dtype %d' % dt, dtype=dt)
    for n_in in (0, 33):
        refused('groups[1]: n_in = %d is outside 1 .. 32' % n_in, groups__g1__n_in=n_in)
    for n_out in (0, 9):
        refused('groups[0]: n_out = %d is outside 1 .. 8' % n_out, groups__g0__n_out=n_out)
    for n_act in (-1, 9):
        refused('groups[1]: n_act = %d is outside 0 .. 8' % n_act, groups__g1__n_act=n_act)
    for k in ls.PARAMS[:6]:
        refused('groups[0]: null argument (a weight or bias', **{'groups__g0__' + k: None})
    refused('groups[1]: null argument (a weight or bias', groups__g1__W2a=None)
    refused('groups[1]: null argument (state)', groups__g1__state=None)
    for lr in (-1e-3, float('inf'), float('-inf'), float('nan')):
        refused('groups[0]: lr must be >= 0 and finite', groups__g0__lr=lr)
    for tau in (-1e-3, 1.0 + 1e-9, float('inf'), float('nan')):
        refused('tau must be in [0, 1]', tau=tau)
    for name in ('beta1', 'beta2'):
        for b in (-0.1, 1.0, 1.5, float('nan')):
            refused(name + ' must be in [0, 1)', **{name: b})
    for eps in (0.0, -1e-8, float('inf'), float('nan')):
        refused('eps must be > 0 and finite', eps=eps)
    for s in (float('inf'), float('nan')):
        refused('groups[1]: grad_scale must be finite', groups__g1__grad_scale=s)
    # a target is all of its tensors or none: one missing, one alone, and W2a's of a critic missing
    refused('groups[0]: target is partly set: 5 of its 6', groups__g0__t2=None)
    refused('groups[0]: target is partly set: 1 of its 6', **{'groups__g0__t%d' % j: None for j in range(1, 6)})
    refused('groups[1]: target is partly set: 6 of its 7', groups__g1__t6=None)
    refused('groups[0]: state must be aligned to 8 bytes', groups__g0__state=G0.state + 4)
    refused('groups[0]: W2 must be aligned to the dtype', groups__g0__W2=G0.W2 + 2)
    refused('groups[0]: target b1 must be aligned to the dtype', groups__g0__t1=T0[1] + 1)
    refused('groups[0]: grad must be aligned to the dtype', groups__g0__grad=G0.grad + 2)
    # overlaps inside a group: a parameter's last byte with the next buffer, with its target, with grad and with the state
    refused('groups[0].W1 overlaps groups[0].b1', groups__g0__b1=G0.W1 + 4 * (64 * 20 - 1))
    refused('groups[0].W1 overlaps groups[0].target.W1', groups__g0__t0=G0.W1 + 4 * (64 * 20 - 1))
    refused('groups[0].target.b1 overlaps groups[0].W2', groups__g0__W2=T0[1] + 4 * 63)
    refused('groups[0].target.W2 overlaps groups[0].target.b2', groups__g0__t3=T0[2] + 4 * 4095)
    refused('groups[0].W2 overlaps groups[0].grad', groups__g0__grad=G0.W2 - 4 * (N_A - 1))
    refused('groups[0].target.W3 overlaps groups[0].grad', groups__g0__grad=T0[4] + 4 * 127)
    refused('groups[0].b3 overlaps groups[0].state', groups__g0__state=G0.b3 - (32 + 8 * N_A) + 8)
    refused('groups[0].target.b3 overlaps groups[0].state', groups__g0__state=T0[5])
    refused('groups[0].grad overlaps groups[0].state', groups__g0__state=G0.grad + 4 * N_A - 8)
    refused('groups[1].W3 overlaps groups[1].W2a', groups__g1__W2a=G1.W3 + 4 * 63)
    # and across groups: one parameter, one target or one state named twice; a gradient under another group's state or target
    refused('groups[0].W3 overlaps groups[1].W3', groups__g1__W3=G0.W3)
    refused('groups[0].b2 overlaps groups[1].W1', groups__g1__W1=G0.b2 + 4 * 63)
    refused('groups[0].target.W2 overlaps groups[1].target.W2', groups__g1__t2=T0[2] + 4 * 4095)
    refused('groups[0].W2 overlaps groups[1].target.W2', groups__g1__t2=G0.W2)
    refused('groups[0].state overlaps groups[1].state', groups__g1__state=G0.state + 32 + 8 * N_A - 8)
    refused('groups[0].state overlaps groups[1].grad', groups__g1__grad=G0.state)
    refused('groups[0].target.W1 overlaps groups[1].grad', groups__g1__grad=T0[0] + 4 * (64 * 20 - 1))
    # What passes every check fails only at the device, which does not exist: adjacent buffers, a group without a target,
    # without a gradient or without both, lr = 0, beta = 0, tau at both ends, one group, float64, a negative scale, a plain
    # network whose unused W2a pointers hold anything, and two groups that read ONE gradient (nothing writes it)
    for change in (dict(), dict(groups__g0__b1=G0.W1 + 4 * 64 * 20), dict(groups__g0__lr=0.0), dict(beta1=0.0, beta2=0.0),
                   dict(tau=0.0), dict(tau=1.0), dict(n_groups=1), dict(groups__g1__state=G0.state + 32 + 8 * N_A),
                   dict(dtype=ls.F64), dict(groups__g1__grad_scale=-2.0),
                   {'groups__g0__t%d' % j: None for j in range(6)},
                   dict(groups__g0__grad=None), dict(groups__g0__grad=None, groups__g1__grad=None),
                   dict({'groups__g1__t%d' % j: None for j in range(7)}, groups__g1__grad=None),
                   dict(groups__g0__W2a=G0.W1, groups__g0__t6=G0.W1 + 4), dict(groups__g1__grad=G0.grad)):
        a = _apply(_valid(ls), change)
        a.device = 1 << 20                                          # no such device: nothing is launched either way
        assert lib.atacom_offstep_adam_step(a) == ls.E_HIP, (change, msg())
        assert lib.atacom_offstep_adam_init(a) == ls.E_HIP, (change, msg())
    with pytest.raises(AtacomError, match='null argument'):
        ls.check(lib.atacom_offstep_adam_step(None))


def _nets(torch):
    from rl_on_manifold_amd import MlpPolicy, QCritic
    lin = lambda o, i, dt=torch.float32: (torch.zeros(o, i, dtype=dt), torch.zeros(o, dtype=dt))          # noqa: E731
    net = lambda n_in, n_out, dt=torch.float32: MlpPolicy(*lin(64, n_in, dt), *lin(64, 64, dt), *lin(n_out, 64, dt))   # noqa: E731

    def critic(n1, k, dt=torch.float32, kind='td3'):
        (W1, b1), (W2, b2), (W3, b3) = lin(64, n1, dt), lin(64, 64, dt), lin(1, 64, dt)
        return QCritic(W1, b1, W2, b2, torch.zeros(64, k, dtype=dt), W3, b3, kind=kind)
    return net, critic


def test_python_arguments_are_refused_before_the_library_is_called():
    torch = pytest.importorskip('torch')
    from rl_on_manifold_amd import GraphedFit, TrackedAdam
    net, critic = _nets(torch)
    act, act_t, q, q_t = net(4, 2), net(4, 2), critic(6, 2), critic(6, 2)
    strided = net(4, 2)
    strided.tensors['W2'] = torch.zeros(64, 128)[:, ::2]
    listed = net(4, 1)
    listed.tensors['b1'] = [0.0] * 64
    mixed = critic(6, 2)
    mixed.tensors['W2a'] = torch.zeros(64, 2, dtype=torch.float64)
    wide = critic(6, 9, kind='ddpg')
    TA = TrackedAdam
    for call, words in ((lambda: TA([dict(net=act, target=act_t), dict(net=q, target=q_t)]), 'run on a GPU'),
                        (lambda: TA([dict(net=critic(3, 1, torch.float64, 'ddpg'))]), 'run on a GPU'),
                        (lambda: TA([]), 'a list of 1 .. 4 dicts'),
                        (lambda: TA([dict(net=q)] * 5), 'a list of 1 .. 4 dicts'),
                        (lambda: TA(dict(net=q)), 'a list of 1 .. 4 dicts'),
                        (lambda: TA([q]), "a dict with the key 'net'"),
                        (lambda: TA([dict(net=q, log_std=torch.zeros(1))]), "a dict with the key 'net'"),
                        (lambda: TA([dict(net=torch.nn.Linear(4, 1))]), 'net must be an MlpPolicy or a QCritic'),
                        (lambda: TA([dict(net=q, target=act_t)]), 'target must be another QCritic'),
                        (lambda: TA([dict(net=act, target=q_t)]), 'target must be another MlpPolicy'),
                        (lambda: TA([dict(net=q, target=q)]), 'target must be another QCritic'),
                        (lambda: TA([dict(net=q, target=critic(6, 3))]), r'target W2a must be a tensor of shape \(64, 2\)'),
                        (lambda: TA([dict(net=act, target=net(5, 2))]), r'target W1 must be a tensor of shape \(64, 4\)'),
                        (lambda: TA([dict(net=q)], lr=-1.0), 'lr must be >= 0'),
                        (lambda: TA([dict(net=q, lr=float('nan'))]), r'groups\[0\]: lr must be >= 0'),
                        (lambda: TA([dict(net=q)], betas=(0.9, 1.0)), 'betas must be two numbers'),
                        (lambda: TA([dict(net=q)], eps=0.0), 'eps must be > 0'),
                        (lambda: TA([dict(net=q)], tau=1.5), r'tau must be in \[0, 1\]'),
                        (lambda: TA([dict(net=q)], tau=float('nan')), r'tau must be in \[0, 1\]'),
                        (lambda: TA([dict(net=q, scale=float('inf'))]), 'scale must be finite'),
                        (lambda: TA([dict(net=listed)]), 'must be tensors'),
                        (lambda: TA([dict(net=wide)]), 'with 9 action columns is outside'),
                        (lambda: TA([dict(net=net(33, 1))]), 'a 33 -> 1 network'),
                        (lambda: TA([dict(net=net(4, 1, torch.float16))]), 'float32 or float64'),
                        (lambda: TA([dict(net=mixed)]), 'W2a is torch.float64 on cpu where the first parameter is torch.float32'),
                        (lambda: TA([dict(net=act), dict(net=critic(6, 2, torch.float64))]), r'groups\[1\]: W1 is torch.float64'),
                        (lambda: TA([dict(net=strided)]), 'W2 must be contiguous'),
                        (lambda: GraphedFit(None, act, act_t, q, q_t, torch.optim.Adam([torch.zeros(1)]), 64, 0.99), 'a TrackedAdam of the groups'),
                        (lambda: GraphedFit(None, act, act_t, (q, q, q), (q_t, q_t, q_t), None, 64, 0.99), 'one QCritic each or a pair each')):
        with pytest.raises(ValueError, match=words):
            call()


@abi.needs_llvm('llvm-readelf')
def test_kernel_census_and_resources(offstep_lib, tmp_path):
    """Three kernels: k_adam_track<T> for the two dtypes and k_adam_track_init, which serves both.  None uses scratch;
    k_adam_track holds the seven broadcast scalars (eight slots) in LDS, the init kernel none; 1024 threads a workgroup leave a
    thread 128 registers."""
    ks = abi.kernel_rows(offstep_lib, tmp_path)
    assert [k[0].split('(')[0] for k in ks] == sorted(['k_adam_track<float>', 'k_adam_track<double>', 'k_adam_track_init']), ks
    for name, lds, scratch, vgpr, agpr, code in ks:
        print('%-28s VGPR %3d AGPR %3d scratch %d LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        assert scratch == 0, (name, scratch)
        assert vgpr <= 128, (name, vgpr)
        assert lds == (0 if 'init' in name else 8 * (8 if 'double' in name else 4)), (name, lds)


def test_exec_mask_audit_finds_nothing(offstep_lib):
    abi.exec_audit(offstep_lib)


def test_python_surface():
    import rl_on_manifold_amd as pkg
    from rl_on_manifold_amd import offstep

    def params(fn):
        return [(p.name, None if p.default is p.empty else p.default) for p in inspect.signature(fn).parameters.values()]

    pos = lambda *names: [(n, None) for n in names]          # noqa: E731
    assert params(pkg.TrackedAdam.__init__) == pos('self', 'groups') + [('lr', 3e-4), ('betas', (0.9, 0.999)), ('eps', 1e-8), ('tau', 5e-3)]
    assert params(pkg.GraphedFit.__init__)[:14] == pos('self', 'mem', 'actor', 'actor_target', 'critics', 'critic_targets', 'optimizer',
                                                       'minibatch', 'gamma') + [('policy_delay', 2), ('noise_std', 0.0),
                                                                                ('noise_clip', 0.0), ('low', None), ('high', None)]
    assert params(pkg.GraphedFit.replay) == pos('self') + [('idx', None), ('eps', None)] == params(pkg.GraphedFit.eager)
    kinds = [p.kind for p in inspect.signature(pkg.TrackedAdam.step).parameters.values()]
    assert kinds[1] is inspect.Parameter.VAR_POSITIONAL and kinds[2] is inspect.Parameter.KEYWORD_ONLY
    assert params(pkg.TrackedAdam.restore) == pos('self', 's')
    assert params(pkg.TrackedAdam.snapshot) == pos('self') == params(pkg.TrackedAdam.steps) == params(pkg.TrackedAdam.zero_state)
    assert pkg.TrackedAdam is offstep.TrackedAdam and pkg.GraphedFit is offstep.GraphedFit
    assert 'baked into the graph' in offstep.GraphedFit.__doc__.lower() and 'no forks' in offstep.GraphedFit.__doc__
