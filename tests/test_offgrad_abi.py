"""CPU-only checks of libatacom_offgrad.so, the backward half of a DDPG / TD3 update: the header is plain C11, the declared
symbols are exactly the exported ones and the ctypes table, the ctypes structs have gcc's layout, every argument rule is enforced
without a GPU and with a message, and the code objects are what DESIGN.md section 7g says (its row of the build tables:
tests/test_offgrad_build.py).  No compute call is made (no GPU here).

The kernel census: thirty-four kernels.  k_offgrad_critic<T, CH> and k_offgrad_actor<T, CH> for T = float, double and
CH = ceil(n1 / 4) = 1 .. 8 of the critic's first layer, and k_offgrad_reduce<T>."""
import ctypes
import inspect
import re
import subprocess

import pytest

import abi_tools as abi

FUNCTIONS = ('version', 'last_error', 'workspace_size', 'critic_gradient', 'actor_gradient')


@pytest.fixture(scope='module')
def og_lib():
    from rl_on_manifold_amd import build
    return build.build('offgrad', verbose=False)


def test_header_is_plain_c11(tmp_path):
    abi.compile_c11(tmp_path, abi.INCLUDE, '#include "atacom_offgrad_hip.h"\n'
                    'int main(void) {\n'
                    '    atacom_offgrad_critic_args c = {0};\n'
                    '    atacom_offgrad_actor_args a = {0};\n'
                    '    c.struct_size = sizeof c; a.struct_size = sizeof a;\n'
                    '    a.actor.struct_size = sizeof a.actor; a.actor.hidden = ATACOM_OFFGRAD_HIDDEN; c.critics[1].kind = ATACOM_OFFGRAD_TD3;\n'
                    '    if (ATACOM_OFFGRAD_MAX_IN != 32 || ATACOM_OFFGRAD_MAX_ACT != 8 || ATACOM_OFFGRAD_STATS != 4) return 1;\n'
                    '    if (atacom_offgrad_critic_gradient(&c) == ATACOM_OFFGRAD_OK || atacom_offgrad_actor_gradient(&a) == ATACOM_OFFGRAD_OK) return 2;\n'
                    '    if (atacom_offgrad_workspace_size(ATACOM_OFFGRAD_F32, 2, 25, 1, 7, 256, 0) == 0) return 3;\n'
                    '    return !atacom_offgrad_version() || !atacom_offgrad_last_error(); }\n')


def test_declared_exported_and_bound_symbols_are_one_set(og_lib):
    from rl_on_manifold_amd import _lib_offgrad
    names = abi.one_symbol_set(og_lib, 'atacom_offgrad_hip.h', 'atacom_offgrad_', _lib_offgrad)
    assert names == sorted('atacom_offgrad_' + n for n in FUNCTIONS)
    assert _lib_offgrad.load().atacom_offgrad_version().startswith(b'atacom_offgrad')


STRUCTS = {
    'atacom_offgrad_critic': ('Critic', ('kind', 'n_obs', 'n_act', 'activation', 'W1', 'b1', 'W2', 'b2', 'W2a', 'W3', 'b3', 'obs_shift',
                                         'obs_scale', 'act_scale')),
    'atacom_offgrad_critic_args': ('CriticArgs', ('struct_size', 'device', 'dtype', 'n_blocks', 'n_critics', 'reserved', 'n_outer',
                                                  'n_inner', 'critics', 'obs', 'action', 'target', 'target_stride', 'idx', 'n_idx', 'grad',
                                                  'stats', 'workspace', 'workspace_bytes', 'stream')),
    'atacom_offgrad_actor_args': ('ActorArgs', ('struct_size', 'device', 'dtype', 'n_blocks', 'n_outer', 'n_inner', 'actor', 'critic', 'obs',
                                                'idx', 'n_idx', 'grad', 'stats', 'action_out', 'action_out_stride', 'dqda_out',
                                                'dqda_out_stride', 'workspace', 'workspace_bytes', 'stream')),
}


def test_the_ctypes_structs_have_the_layout_of_the_header(tmp_path):
    """sizeof and the offset of every field, as gcc lays the header out; the critic descriptor is field for field that of
    libatacom_offpolicy.so."""
    from rl_on_manifold_amd import _lib_offgrad as lg, _lib_offpolicy as lo
    src = tmp_path / 'layout.c'
    body = ''
    for cname, (_, fields) in STRUCTS.items():
        body += '    printf("%%zu", sizeof(%s));\n' % cname
        body += ''.join('    printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f in fields) + '    printf("\\n");\n'
    src.write_text('#include <stdio.h>\n#include "atacom_offgrad_hip.h"\nint main(void) {\n' + body +
                   '    printf("%d %d %d %d %d %d %d\\n", ATACOM_OFFGRAD_DDPG, ATACOM_OFFGRAD_TD3, ATACOM_OFFGRAD_MAX_IN, '
                   'ATACOM_OFFGRAD_MAX_ACT, ATACOM_OFFGRAD_HIDDEN, ATACOM_OFFGRAD_MAX_BLOCKS, ATACOM_OFFGRAD_STATS);\n    return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c11', '-I', abi.INCLUDE, str(src), '-o', exe])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, (cname, (pyname, fields)) in zip(lines, STRUCTS.items()):
        S = getattr(lg, pyname)
        assert [int(x) for x in line.split()] == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields], cname
        assert [f for f, _ in S._fields_] == list(fields), cname
    assert [int(x) for x in lines[-1].split()] == [lg.DDPG, lg.TD3, lg.MAX_IN, lg.MAX_ACT, lg.HIDDEN, lg.MAX_BLOCKS, lg.STATS]
    assert [(f, t) for f, t in lg.Critic._fields_] == [(f, t) for f, t in lo.Critic._fields_]
    assert lg.grad_size(25, 1, 7) == 64 * 25 + 64 + 4096 + 64 + 64 + 1 + 64 * 7


MEM, IDX, TGT, GRAD, STATS, AOUT, DQ, WS = 0x100000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000, 0x900000
N, D, K = 1000, 18, 7
F = 2 * D + K + 3


def _critic(lg, **kw):
    c = lg.Critic()
    c.kind, c.n_obs, c.n_act, c.activation = lg.TD3, D, K, 0
    for k in ('W1', 'b1', 'W2', 'b2', 'W2a', 'W3', 'b3'):
        setattr(c, k, 0x1000)                            # never dereferenced
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _apply(a, change):
    for k, val in change.items():
        obj = a
        *path, leaf = k.split('__')
        for part in path:
            obj = obj[int(part)] if part.isdigit() else getattr(obj, part)
        if leaf.isdigit():
            obj[int(leaf)] = val
        else:
            setattr(obj, leaf, val)
    return a


def _valid_critic(lg):
    """256 rows gathered through idx from the columns of a [1000, F] memory, a pair: passes every check."""
    a = lg.new_args(lg.CriticArgs)
    a.device, a.dtype, a.n_outer, a.n_inner, a.n_critics = 0, lg.F32, 1, N, 2
    a.critics[0], a.critics[1] = _critic(lg), _critic(lg)
    a.obs, a.action = lg.View(MEM, 0, F), lg.View(MEM + 4 * D, 0, F)
    a.target, a.target_stride, a.idx, a.n_idx = TGT, 1, IDX, 256
    a.grad[0], a.grad[1], a.stats[0], a.stats[1] = GRAD, GRAD + 0x40000, STATS, STATS + 0x100
    a.workspace = WS
    a.workspace_bytes = lg.load().atacom_offgrad_workspace_size(lg.F32, 2, D + K, 1, K, 256, 0)
    return a


def _valid_actor(lg):
    a = lg.new_args(lg.ActorArgs)
    a.device, a.dtype, a.n_outer, a.n_inner = 0, lg.F32, 1, N
    a.actor = abi.fake_mlp(n_in=D, n_out=K, mean_mode=1, explore=1, std=0x1000, act_scale=0x1000)        # a from_td3 policy as it is
    a.critic = _critic(lg)
    a.obs = lg.View(MEM, 0, F)
    a.idx, a.n_idx, a.grad, a.stats = IDX, 256, GRAD, STATS
    a.action_out, a.action_out_stride, a.dqda_out, a.dqda_out_stride = AOUT, K, DQ, K
    a.workspace = WS
    a.workspace_bytes = lg.load().atacom_offgrad_workspace_size(lg.F32, 1, D, K, 0, 256, 0)
    return a


def test_workspace_size(og_lib):
    from rl_on_manifold_amd import _lib_offgrad as lg
    lib = lg.load()
    size = lib.atacom_offgrad_workspace_size
    q = lg.grad_size(25, 1, 7) + lg.STATS
    assert size(lg.F32, 1, 25, 1, 7, 256, 0) == (1 * q * 4 + 255) // 256 * 256                 # one tile of 4 x 64 rows
    assert size(lg.F32, 2, 25, 1, 7, 257, 0) == (2 * 2 * q * 4 + 255) // 256 * 256
    assert size(lg.F64, 2, 25, 1, 7, 257, 0) == (2 * 17 * q * 8 + 255) // 256 * 256            # tiles of 16 rows
    assert size(lg.F32, 1, 25, 1, 7, 1 << 20, 0) == (512 * q * 4 + 255) // 256 * 256           # the ceiling of the library's choice
    assert size(lg.F32, 1, 25, 1, 7, 16, 7) == (7 * q * 4 + 255) // 256 * 256
    for args, words in (((2, 1, 25, 1, 7, 16, 0), 'no kernel for dtype 2'), ((0, 3, 25, 1, 7, 16, 0), 'n_nets = 3'),
                        ((0, 1, 33, 1, 7, 16, 0), 'n_in = 33'), ((0, 1, 25, 9, 0, 16, 0), 'n_out = 9'), ((0, 1, 25, 1, 9, 16, 0), 'n_act = 9'),
                        ((0, 1, 25, 1, 7, 0, 0), 'rows = 0'), ((0, 1, 25, 1, 7, 16, 65536), 'n_blocks = 65536')):
        assert size(*args) == 0 and words in lib.atacom_offgrad_last_error().decode(), args


def test_arguments_are_validated_without_a_gpu(og_lib):
    from rl_on_manifold_amd import _lib, _lib_offgrad as lg, AtacomError
    lib = lg.load()

    def msg():
        return lib.atacom_offgrad_last_error().decode()

    def refused(fn, valid, code, words, **change):
        a = _apply(valid(lg), change)
        assert getattr(lib, fn)(a) == code, (fn, change, msg())
        assert words in msg() and fn in msg(), (fn, change, msg())

    for fn, valid, cls in (('atacom_offgrad_critic_gradient', _valid_critic, lg.CriticArgs),
                           ('atacom_offgrad_actor_gradient', _valid_actor, lg.ActorArgs)):
        ref = lambda *a, **k: refused(fn, valid, *a, **k)          # noqa: E731
        assert getattr(lib, fn)(None) == lg.E_INVALID and 'null argument' in msg() and fn in msg()
        ref(lg.E_INVALID, 'struct_size', struct_size=ctypes.sizeof(cls) - 8)
        ref(lg.E_INVALID, 'device', device=-1)
        ref(lg.E_UNSUPPORTED, 'no kernel for dtype 2', dtype=2)
        ref(lg.E_INVALID, 'n_outer must be >= 1', n_outer=0)
        ref(lg.E_INVALID, 'n_inner must be >= 1', n_inner=0)
        ref(lg.E_INVALID, 'n_blocks must be >= 1', n_blocks=-1)
        ref(lg.E_UNSUPPORTED, 'is too many (at most 2147483647 a call)', n_outer=2 ** 16, n_inner=2 ** 15)
        ref(lg.E_UNSUPPORTED, 'exceeds the launch grid', n_blocks=65536)
        ref(lg.E_INVALID, 'n_idx must be >= 1 with idx', n_idx=0)
        ref(lg.E_UNSUPPORTED, 'n_idx = 2147483648 rows is too many', n_idx=2 ** 31)
        cr = 'critics__1__' if fn.endswith('critic_gradient') else 'critic__'
        ref(lg.E_UNSUPPORTED, 'kind = 2', **{cr + 'kind': 2})
        for n_obs in (0, 33):
            ref(lg.E_UNSUPPORTED, 'n_obs = %d is outside 1 .. 32' % n_obs, **{cr + 'n_obs': n_obs})
        for n_act in (0, 9):                                                                        # k > 8
            ref(lg.E_UNSUPPORTED, 'n_act = %d is outside 1 .. 8' % n_act, **{cr + 'n_act': n_act})
        ref(lg.E_UNSUPPORTED, 'n1 = n_obs + n_act = 33', **{cr + 'n_obs': 26})                      # n1 > 32
        ref(lg.E_UNSUPPORTED, 'activation = 2', **{cr + 'activation': 2})
        for k in ('W1', 'b1', 'W2', 'b2', 'W2a', 'W3', 'b3'):
            ref(lg.E_INVALID, 'null argument (a weight or bias of the critic)', **{cr + k: None})
        ref(lg.E_INVALID, 'W2a must be aligned to the dtype', **{cr + 'W2a': 0x1002})
        ref(lg.E_INVALID, 'act_scale must be aligned to the dtype', **{cr + 'act_scale': 0x1001})
        ref(lg.E_INVALID, 'null argument (obs)', obs__ptr=None)
        ref(lg.E_INVALID, 'obs must be aligned to the dtype', obs__ptr=MEM + 2)
        ref(lg.E_INVALID, 'idx must be aligned', idx=IDX + 4)
        ref(lg.E_INVALID, 'obs.stride_inner = 17 is below the row width 18', obs__stride_inner=17)
        ref(lg.E_INVALID, 'null argument (workspace)', workspace=None)
        ref(lg.E_INVALID, 'workspace must be aligned to 16 bytes', workspace=WS + 8)
        a = valid(lg)
        ref(lg.E_INVALID, 'workspace_bytes = %d is below the %d' % (a.workspace_bytes - 256, a.workspace_bytes), workspace_bytes=a.workspace_bytes - 256)
        ref(lg.E_INVALID, 'workspace_bytes', n_blocks=3)                                             # sized for one workgroup
        ref(lg.E_INVALID, 'workspace overlaps obs', workspace=MEM + 1600)
        ref(lg.E_INVALID, 'workspace overlaps idx', workspace=IDX + 8 * 256 - 16)
    # ---- the critic call
    c = lambda *a, **k: refused('atacom_offgrad_critic_gradient', _valid_critic, *a, **k)          # noqa: E731
    for n in (0, 3):
        c(lg.E_INVALID, 'n_critics = %d' % n, n_critics=n)
    c(lg.E_INVALID, 'the two critics differ', critics__1__kind=lg.DDPG)
    c(lg.E_INVALID, 'the two critics differ', critics__1__n_obs=D - 1)
    c(lg.E_INVALID, 'the two critics differ', critics__1__n_act=K - 1)
    c(lg.E_INVALID, 'null argument (action)', action__ptr=None)
    c(lg.E_INVALID, 'null argument (target)', target=None)
    c(lg.E_INVALID, 'null argument (grad[1] or stats[1])', grad__1=None)
    c(lg.E_INVALID, 'null argument (grad[0] or stats[0])', stats__0=None)
    c(lg.E_INVALID, 'target must be aligned to the dtype', target=TGT + 1)
    c(lg.E_INVALID, 'grad must be aligned to the dtype', grad__0=GRAD + 2)
    c(lg.E_INVALID, 'action.stride_inner = -6 is below the row width 7', action__stride_inner=-6)
    c(lg.E_INVALID, 'grad[0] overlaps obs', grad__0=MEM + 4 * (F * (N - 1) + D - 1))
    c(lg.E_INVALID, 'grad[0] overlaps action', grad__0=MEM + 4 * (F * (N - 1) + D + K - 1))
    c(lg.E_INVALID, 'stats[1] overlaps target', stats__1=TGT + 4 * 255)
    c(lg.E_INVALID, 'grad[1] overlaps idx', grad__1=IDX + 8 * 255)
    c(lg.E_INVALID, 'grad[0] overlaps grad[1]', grad__1=GRAD + 4 * 100)
    c(lg.E_INVALID, 'grad[0] overlaps stats[0]', stats__0=GRAD + 4)
    c(lg.E_INVALID, 'stats[0] overlaps stats[1]', stats__1=STATS + 12)
    c(lg.E_INVALID, 'grad[1] overlaps workspace', workspace=GRAD + 0x40000 + 16)
    # ---- the actor call
    t = lambda *a, **k: refused('atacom_offgrad_actor_gradient', _valid_actor, *a, **k)          # noqa: E731
    t(lg.E_INVALID, 'actor.struct_size', actor__struct_size=ctypes.sizeof(_lib.AtacomMlp) - 4)
    t(lg.E_UNSUPPORTED, 'only 64 hidden units', actor__hidden=32)
    t(lg.E_INVALID, 'the actor maps 17 to 7', actor__n_in=D - 1)
    t(lg.E_INVALID, 'the actor maps 18 to 6', actor__n_out=K - 1)
    t(lg.E_UNSUPPORTED, 'actor: activation = 2', actor__activation=2)
    t(lg.E_INVALID, 'null argument (a weight or bias of the actor)', actor__W2=None)
    t(lg.E_UNSUPPORTED, 'sigma network', actor__sW1=0x1000)
    t(lg.E_UNSUPPORTED, 'squash', actor__squash=1)
    t(lg.E_UNSUPPORTED, 'mean_mode = 2', actor__mean_mode=2)
    t(lg.E_INVALID, 'actor.W3 must be aligned to the dtype', actor__W3=0x1002)
    t(lg.E_INVALID, 'null argument (grad or stats)', grad=None)
    t(lg.E_INVALID, 'null argument (grad or stats)', stats=None)
    t(lg.E_INVALID, 'action_out must be aligned', action_out=AOUT + 2)
    t(lg.E_INVALID, 'action_out_stride = 6 is below the row width 7', action_out_stride=6)
    t(lg.E_INVALID, 'dqda_out_stride = 0 is below the row width 7', dqda_out_stride=0)
    t(lg.E_INVALID, 'grad overlaps obs', grad=MEM + 4 * (F * (N - 1) + D - 1))
    t(lg.E_INVALID, 'stats overlaps idx', stats=IDX)
    t(lg.E_INVALID, 'grad overlaps stats', stats=GRAD + 4 * 1000)
    t(lg.E_INVALID, 'grad overlaps action_out', action_out=GRAD + 4 * 8)
    t(lg.E_INVALID, 'action_out overlaps dqda_out', dqda_out=AOUT + 4 * (256 * K - 1))
    t(lg.E_INVALID, 'dqda_out overlaps workspace', workspace=DQ + 16)
    t(lg.E_INVALID, 'action_out overlaps obs', action_out=MEM - 4 * (256 * K - 1))
    # What passes every check fails only at the device, which does not exist: the valid calls, one critic, no idx, a repeated
    # input row, no optional outputs, a DDPG critic of the maximum size, mean_mode 0, float64
    for fn, valid, changes in (('atacom_offgrad_critic_gradient', _valid_critic,
                                (dict(), dict(n_critics=1), dict(idx=None), dict(obs__stride_inner=0),
                                 dict(n_critics=1, critics__0__kind=lg.DDPG, critics__0__n_obs=32, critics__0__n_act=8))),
                               ('atacom_offgrad_actor_gradient', _valid_actor,
                                (dict(), dict(action_out=None), dict(dqda_out=None, action_out=None), dict(idx=None), dict(actor__mean_mode=0)))):
        for change in changes:
            a = _apply(valid(lg), change)
            a.workspace_bytes = 1 << 30
            a.device = 1 << 20
            assert getattr(lib, fn)(a) == lg.E_HIP, (fn, change, msg())
    a = _valid_actor(lg)
    a.actor.struct_size = _lib.AtacomMlp.mean_mode.offset            # ATACOM_MLP_SIZE_V1: accepted, runs mean_mode 0
    a.device = 1 << 20
    assert lib.atacom_offgrad_actor_gradient(a) == lg.E_HIP, msg()
    with pytest.raises(AtacomError, match='null argument'):
        lg.check(lib.atacom_offgrad_critic_gradient(None))


def test_python_arguments_are_refused_before_the_library_is_called(monkeypatch):
    import torch
    from rl_on_manifold_amd import MlpPolicy, QCritic, ReplayMemory, offgrad

    def never(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(offgrad._lg, 'load', never)
    lin = lambda o, i: (torch.zeros(o, i), torch.zeros(o))          # noqa: E731
    pol = MlpPolicy(*lin(64, 4), *lin(64, 64), *lin(2, 64))
    pol3 = MlpPolicy(*lin(64, 4), *lin(64, 64), *lin(3, 64))
    cr = QCritic(*lin(64, 6), *lin(64, 64), torch.zeros(64, 2), *lin(1, 64), kind='td3')
    dd = QCritic(*lin(64, 4), *lin(64, 64), torch.zeros(64, 2), *lin(1, 64), kind='ddpg')
    wide = QCritic(*lin(64, 33), *lin(64, 64), torch.zeros(64, 8), *lin(1, 64), kind='td3')
    x, a, y = torch.zeros(5, 4), torch.zeros(5, 2), torch.zeros(5)
    idx = torch.tensor([4, 0, 4])
    for call, words in ((lambda: offgrad.critic_gradient(cr, x, a, y), 'run on a GPU'),
                        (lambda: offgrad.critic_gradient([cr, cr], x, a, y[:3], idx=idx), 'run on a GPU'),
                        (lambda: offgrad.actor_gradient(pol, cr, x), 'run on a GPU'),
                        (lambda: offgrad.critic_gradient(pol, x, a, y), 'one QCritic or a pair'),
                        (lambda: offgrad.critic_gradient([cr, cr, cr], x, a, y), 'one QCritic or a pair'),
                        (lambda: offgrad.critic_gradient([cr, dd], x, a, y), 'the two critics differ'),
                        (lambda: offgrad.critic_gradient(wide, torch.zeros(5, 25), torch.zeros(5, 8), y), 'n1 = 33'),
                        (lambda: offgrad.critic_gradient(cr, x, a, y[:4]), 'target must be a tensor of shape \\(5,\\)'),
                        (lambda: offgrad.critic_gradient(cr, x, a, y, idx=idx), 'target must be a tensor of shape \\(3,\\)'),
                        (lambda: offgrad.critic_gradient(cr, x, a, y.double()), 'target must be a torch.float32 tensor'),
                        (lambda: offgrad.critic_gradient(cr, x, a[:, :1], y), 'action must be a tensor of shape'),
                        (lambda: offgrad.critic_gradient(cr, x, a, y, idx=idx.int()), 'idx must be a one-dimensional int64'),
                        (lambda: offgrad.critic_gradient(cr, x, a, y, n_blocks=-1), 'n_blocks must be 0'),
                        (lambda: offgrad.critic_gradient(cr, x.half(), a, y), 'obs must be float32 or float64'),
                        (lambda: offgrad.critic_gradient(cr, torch.zeros(0, 4), a, y), 'obs holds no rows'),
                        (lambda: offgrad.actor_gradient(pol, pol, x), 'critic must be a QCritic'),
                        (lambda: offgrad.actor_gradient(cr, cr, x), 'actor must be an MlpPolicy'),
                        (lambda: offgrad.actor_gradient(pol3, cr, x), 'the actor maps 4 to 3'),
                        (lambda: offgrad.actor_gradient(pol, cr, torch.zeros(5, 3)), 'obs must be a tensor of shape'),
                        (lambda: ReplayMemory(8, 4, 2, device='cpu').critic_gradient(cr, idx, y[:3]), 'run on a GPU'),
                        (lambda: ReplayMemory(8, 4, 2, device='cpu').actor_gradient(pol, cr, idx), 'run on a GPU')):
        with pytest.raises(ValueError, match=words):
            call()

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self._h1, self._h2_s, self._h2_a, self._h3 = (torch.nn.Linear(6, 64), torch.nn.Linear(64, 64),
                                                          torch.nn.Linear(2, 64, bias=False), torch.nn.Linear(64, 1))
    g = offgrad.QGradients(6, 2, torch.float32, 'cpu', torch.empty(0, dtype=torch.uint8), None)
    assert g.flat.numel() == 64 * 6 + 64 + 4096 + 64 + 64 + 1 + 128 and g.W2a.shape == (64, 2) and g.W3.shape == (1, 64)
    assert g.W2a.data_ptr() == g.flat.data_ptr() + 4 * (g.flat.numel() - 128)
    net = Net()
    g.to_module(net)
    assert net._h2_a.weight.grad is g.W2a and net._h1.bias.grad is g.b1 and net._h3.weight.grad is g.W3
    torch.optim.Adam(net.parameters()).step()
    with pytest.raises(ValueError, match='a parameter is'):
        offgrad.QGradients(5, 2, torch.float32, 'cpu', None, None).to_module(net)


@abi.needs_llvm('llvm-readelf')
def test_kernel_census_and_resources(og_lib, tmp_path):
    """Thirty-four kernels (the module docstring).  Float32: no scratch, 63808 bytes of static LDS -- one network block
    MlpLdsM<.., 64, 8>::NET = 7752 floats with W2a in the unread rows of its W3 block, 8 floats, and 4 wavefronts x 2048 of
    staging -- which is <= 65536, and at most 512 registers: the budget of __launch_bounds__(256, 1), one wavefront per SIMD.
    Float64: one record per row, 16 rows."""
    ks = abi.kernel_rows(og_lib, tmp_path)
    want = ['k_offgrad_%s<%s, %d>' % (n, t, ch) for n in ('critic', 'actor') for t in ('float', 'double') for ch in range(1, 9)] + \
           ['k_offgrad_reduce<float>', 'k_offgrad_reduce<double>']
    assert [k[0] for k in ks] == sorted(want), ks
    for name, lds, scratch, vgpr, agpr, code in ks:
        print('%-30s VGPR %3d AGPR %3d scratch %d LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        assert lds <= 65536 and vgpr <= 512, (name, lds, vgpr)
        if 'reduce' in name:
            assert scratch == 0 and lds == 8 * 32 * (4 if 'float' in name else 8), name
        elif 'float' in name:
            assert scratch == 0, (name, scratch)
            assert lds == 4 * (7752 + 8 + 4 * 2048) == 63808, (name, lds)
        else:
            assert lds == 8 * 16 * ((4 * 64 + 32 + 8 + 8 + 3) + (0 if 'critic' in name else 64 + 64 + 32 + 8)), (name, lds)


@abi.needs_llvm('llvm-objdump')
def test_the_float32_kernels_run_on_the_matrix_cores_without_atomics(og_lib, tmp_path):
    seen = 0
    for _, head, body in abi.function_bodies(og_lib, tmp_path):
        k = re.search(r'k_offgrad_(critic|actor|reduce)<(float|double)(?:, (\d))?>', head)
        if not k:
            continue
        seen += 1
        assert not re.search(r'\b(global|flat|buffer|ds)_atomic|\bds_(add|cmpst)', body), head
        mfma = len(re.findall(r'\bv_mfma_f32_16x16x4[_f32]*\b', body))
        if k.group(2) == 'float' and k.group(1) != 'reduce':
            ch, nt = int(k.group(3)), 2 if int(k.group(3)) > 4 else 1
            forward = 4 * ch + 64 + 8 + 16
            backward = 16 + 8 + 64 + 64 + 16 * nt                       # dW3, delta2, dW2, delta1, dW1
            if k.group(1) == 'critic':
                assert mfma == forward + backward + 16, (head, mfma)    # + dW2a
            else:
                # three forward passes, the actor's two without action steps and its second without the output layer (only its
                # activations are recomputed); the actor's backward pass; the critic's delta1 and the two parts of its input gradient
                assert mfma == 3 * forward - 2 * 8 - 16 + backward + 64 + 16 + 16, (head, mfma)
        else:
            assert mfma == 0, (head, mfma)
    assert seen == 34


def test_exec_mask_audit_finds_nothing(og_lib):
    abi.exec_audit(og_lib)


def test_python_surface():
    import rl_on_manifold_amd as pkg
    from rl_on_manifold_amd import offgrad

    def params(fn):
        return [(p.name, p.kind is p.KEYWORD_ONLY, None if p.default is p.empty else p.default)
                for p in inspect.signature(fn).parameters.values()]

    pos = lambda *names: [(n, False, None) for n in names]          # noqa: E731
    assert params(pkg.critic_gradient) == pos('critics', 'obs', 'action', 'target') + [('idx', True, None), ('out', True, None), ('n_blocks', True, 0)]
    assert params(pkg.actor_gradient) == pos('actor', 'critic', 'obs') + [('idx', True, None), ('out', True, None), ('action_out', True, None),
                                                                         ('dqda_out', True, None), ('n_blocks', True, 0)]
    assert [p[0] for p in params(pkg.ReplayMemory.critic_gradient)] == ['self', 'critics', 'idx', 'target', 'kw']
    assert [p[0] for p in params(pkg.ReplayMemory.actor_gradient)] == ['self', 'actor', 'critic', 'idx', 'kw']
    assert pkg.critic_gradient is offgrad.critic_gradient and pkg.actor_gradient is offgrad.actor_gradient and pkg.QGradients is offgrad.QGradients
    from rl_on_manifold_amd import _lib_offpolicy
    assert offgrad.PARAMS == _lib_offpolicy.PARAMS
