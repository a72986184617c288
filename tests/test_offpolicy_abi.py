"""CPU-only checks of libatacom_offpolicy.so, the forward half of a DDPG / TD3 update: the header is plain C11, the declared
symbols are exactly the exported ones and the ctypes table, the ctypes structs have gcc's layout, every argument rule is enforced
without a GPU and with a message, and the code objects are what DESIGN.md section 7f says (its row of the build tables:
tests/test_offpolicy_build.py).  No compute call is made (no GPU here).

The kernel census: eighteen kernels.  k_offpolicy_net<T, CH> for T = float, double and CH = ceil(n1 / 4) = 1 .. 8 serves both
atacom_offpolicy_q and atacom_offpolicy_target (the phases are a launch-uniform loop), and k_soft_update<T>."""
import ctypes
import inspect
import re
import subprocess

import pytest

import abi_tools as abi

FUNCTIONS = ('version', 'last_error', 'q', 'target', 'soft_update')


@pytest.fixture(scope='module')
def off_lib():
    from rl_on_manifold_amd import build
    return build.build('offpolicy', verbose=False)


def test_header_is_plain_c11(tmp_path):
    abi.compile_c11(tmp_path, abi.INCLUDE, '#include "atacom_offpolicy_hip.h"\n'
                    'int main(void) {\n'
                    '    atacom_offpolicy_q_args q = {0};\n'
                    '    atacom_offpolicy_target_args t = {0};\n'
                    '    atacom_offpolicy_soft_update_args s = {0};\n'
                    '    q.struct_size = sizeof q; t.struct_size = sizeof t; s.struct_size = sizeof s;\n'
                    '    t.actor.struct_size = sizeof t.actor; t.actor.hidden = ATACOM_OFFPOLICY_HIDDEN; t.critics[1].kind = ATACOM_OFFPOLICY_TD3;\n'
                    '    s.pairs[3].n_act = ATACOM_OFFPOLICY_MAX_ACT; s.tau = 5e-3;\n'
                    '    if (ATACOM_OFFPOLICY_MAX_IN != 32 || ATACOM_OFFPOLICY_MAX_ACT != 8 || ATACOM_OFFPOLICY_MAX_PAIRS != 4) return 1;\n'
                    '    if (atacom_offpolicy_q(&q) == ATACOM_OFFPOLICY_OK || atacom_offpolicy_target(&t) == ATACOM_OFFPOLICY_OK) return 2;\n'
                    '    if (atacom_offpolicy_soft_update(&s) == ATACOM_OFFPOLICY_OK) return 3;\n'
                    '    return !atacom_offpolicy_version() || !atacom_offpolicy_last_error(); }\n')


def test_declared_exported_and_bound_symbols_are_one_set(off_lib):
    from rl_on_manifold_amd import _lib_offpolicy
    names = abi.one_symbol_set(off_lib, 'atacom_offpolicy_hip.h', 'atacom_offpolicy_', _lib_offpolicy)
    assert names == sorted('atacom_offpolicy_' + n for n in FUNCTIONS)
    assert _lib_offpolicy.load().atacom_offpolicy_version().startswith(b'atacom_offpolicy')


STRUCTS = {
    'atacom_offpolicy_critic': ('Critic', ('kind', 'n_obs', 'n_act', 'activation', 'W1', 'b1', 'W2', 'b2', 'W2a', 'W3', 'b3', 'obs_shift',
                                           'obs_scale', 'act_scale')),
    'atacom_offpolicy_q_args': ('QArgs', ('struct_size', 'device', 'dtype', 'n_blocks', 'n_outer', 'n_inner', 'critic', 'obs', 'action',
                                          'idx', 'n_idx', 'q', 'q_stride', 'stream')),
    'atacom_offpolicy_target_args': ('TargetArgs', ('struct_size', 'device', 'dtype', 'n_blocks', 'n_critics', 'reserved', 'n_outer',
                                                    'n_inner', 'actor', 'critics', 'next_obs', 'reward', 'absorbing', 'eps', 'eps_stride',
                                                    'noise_std', 'noise_clip', 'gamma', 'act_low', 'act_high', 'idx', 'n_idx', 'y',
                                                    'y_stride', 'action_out', 'action_out_stride', 'stream')),
    'atacom_offpolicy_pair': ('Pair', ('n_in', 'n_out', 'n_act', 'reserved', 'target', 'online')),
    'atacom_offpolicy_soft_update_args': ('SoftUpdateArgs', ('struct_size', 'device', 'dtype', 'n_pairs', 'tau', 'stream', 'pairs')),
}


def test_the_ctypes_structs_have_the_layout_of_the_header(tmp_path):
    """sizeof and the offset of every field, as gcc lays the header out."""
    from rl_on_manifold_amd import _lib_offpolicy as lo
    src = tmp_path / 'layout.c'
    body = ''
    for cname, (_, fields) in STRUCTS.items():
        body += '    printf("%%zu", sizeof(%s));\n' % cname
        body += ''.join('    printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f in fields) + '    printf("\\n");\n'
    src.write_text('#include <stdio.h>\n#include "atacom_offpolicy_hip.h"\nint main(void) {\n' + body +
                   '    printf("%d %d %d %d %d %d %d %d\\n", ATACOM_OFFPOLICY_DDPG, ATACOM_OFFPOLICY_TD3, ATACOM_OFFPOLICY_MAX_IN, '
                   'ATACOM_OFFPOLICY_MAX_ACT, ATACOM_OFFPOLICY_HIDDEN, ATACOM_OFFPOLICY_MAX_BLOCKS, ATACOM_OFFPOLICY_MAX_PAIRS, '
                   'ATACOM_OFFPOLICY_TENSORS);\n    return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c11', '-I', abi.INCLUDE, str(src), '-o', exe])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, (cname, (pyname, fields)) in zip(lines, STRUCTS.items()):
        S = getattr(lo, pyname)
        assert [int(x) for x in line.split()] == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields], cname
        assert [f for f, _ in S._fields_] == list(fields), cname
    assert [int(x) for x in lines[-1].split()] == [lo.DDPG, lo.TD3, lo.MAX_IN, lo.MAX_ACT, lo.HIDDEN, lo.MAX_BLOCKS, lo.MAX_PAIRS, lo.TENSORS]


MEM, IDX, EPS, Y, AOUT, LOW, HIGH = 0x100000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x700100
N, D, K = 1000, 18, 7
F = 2 * D + K + 3


def _critic(lo, **kw):
    c = lo.Critic()
    c.kind, c.n_obs, c.n_act, c.activation = lo.TD3, D, K, 0
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
        setattr(obj, leaf, val)
    return a


def _valid_q(lo):
    """256 rows gathered through idx from the columns of a [1000, F] memory: passes every check."""
    a = lo.new_args(lo.QArgs)
    a.device, a.dtype, a.n_outer, a.n_inner, a.critic = 0, lo.F32, 1, N, _critic(lo)
    a.obs, a.action = lo.View(MEM, 0, F), lo.View(MEM + 4 * D, 0, F)
    a.idx, a.n_idx, a.q, a.q_stride = IDX, 256, Y, 1
    return a


def _valid_target(lo):
    a = lo.new_args(lo.TargetArgs)
    a.device, a.dtype, a.n_outer, a.n_inner, a.n_critics = 0, lo.F32, 1, N, 2
    a.actor = abi.fake_mlp(n_in=D, n_out=K, mean_mode=1, explore=1, std=0x1000)        # a from_td3 policy as it is
    a.critics[0], a.critics[1] = _critic(lo), _critic(lo)
    o = D + K
    a.next_obs, a.reward, a.absorbing = lo.View(MEM + 4 * (o + 1), 0, F), lo.View(MEM + 4 * o, 0, F), lo.View(MEM + 4 * (o + 1 + D), 0, F)
    a.eps, a.eps_stride, a.noise_std, a.noise_clip, a.gamma, a.act_low, a.act_high = EPS, K, 0.2, 0.5, 0.99, LOW, HIGH
    a.idx, a.n_idx, a.y, a.y_stride, a.action_out, a.action_out_stride = IDX, 256, Y, 1, AOUT, K
    return a


def _valid_soft(lo):
    a = lo.new_args(lo.SoftUpdateArgs)
    a.device, a.dtype, a.n_pairs, a.tau = 0, lo.F32, 2, 5e-3
    for j, (n_in, n_out, n_act) in enumerate(((D, K, 0), (D + K, 1, K))):
        p = a.pairs[j]
        p.n_in, p.n_out, p.n_act = n_in, n_out, n_act
        for i in range(lo.TENSORS if n_act else 6):
            p.target[i], p.online[i] = 0x1000000 * (j + 1) + 0x10000 * i, 0x4000000 * (j + 1) + 0x10000 * i
    return a


def test_arguments_are_validated_without_a_gpu(off_lib):
    from rl_on_manifold_amd import _lib, _lib_offpolicy as lo, AtacomError
    lib = lo.load()

    def msg():
        return lib.atacom_offpolicy_last_error().decode()

    def refused(fn, valid, code, words, **change):
        a = _apply(valid(lo), change)
        assert getattr(lib, fn)(a) == code, (fn, change, msg())
        assert words in msg() and fn in msg(), (fn, change, msg())

    for fn, valid, cls in (('atacom_offpolicy_q', _valid_q, lo.QArgs), ('atacom_offpolicy_target', _valid_target, lo.TargetArgs)):
        ref = lambda *a, **k: refused(fn, valid, *a, **k)          # noqa: E731
        assert getattr(lib, fn)(None) == lo.E_INVALID and 'null argument' in msg() and fn in msg()
        ref(lo.E_INVALID, 'struct_size', struct_size=ctypes.sizeof(cls) - 8)
        ref(lo.E_INVALID, 'device', device=-1)
        ref(lo.E_UNSUPPORTED, 'no kernel for dtype 2', dtype=2)
        ref(lo.E_INVALID, 'n_outer must be >= 1', n_outer=0)
        ref(lo.E_INVALID, 'n_inner must be >= 1', n_inner=0)
        ref(lo.E_INVALID, 'n_blocks must be >= 1', n_blocks=-1)
        ref(lo.E_UNSUPPORTED, 'is too many (at most 2147483647 a call)', n_outer=2 ** 16, n_inner=2 ** 15)
        ref(lo.E_UNSUPPORTED, 'exceeds the launch grid', n_blocks=65536)
        ref(lo.E_INVALID, 'n_idx must be >= 1 with idx', n_idx=0)
        ref(lo.E_UNSUPPORTED, 'n_idx = 2147483648 rows is too many', n_idx=2 ** 31)
        cr = 'critic__' if fn.endswith('_q') else 'critics__1__'
        ref(lo.E_UNSUPPORTED, 'kind = 2', **{cr + 'kind': 2})
        for n_obs in (0, 33):
            ref(lo.E_UNSUPPORTED, 'n_obs = %d is outside 1 .. 32' % n_obs, **{cr + 'n_obs': n_obs})
        for n_act in (0, 9):
            ref(lo.E_UNSUPPORTED, 'n_act = %d is outside 1 .. 8' % n_act, **{cr + 'n_act': n_act})
        ref(lo.E_UNSUPPORTED, 'n1 = n_obs + n_act = 33', **{cr + 'n_obs': 26})                    # TD3 (25, 8) and its like
        ref(lo.E_UNSUPPORTED, 'activation = 2', **{cr + 'activation': 2})
        for k in ('W1', 'b1', 'W2', 'b2', 'W2a', 'W3', 'b3'):
            ref(lo.E_INVALID, 'null argument (a weight or bias of the critic)', **{cr + k: None})
    # ---- q: views and overlaps
    q = lambda *a, **k: refused('atacom_offpolicy_q', _valid_q, *a, **k)          # noqa: E731
    q(lo.E_INVALID, 'null argument (obs)', obs__ptr=None)
    q(lo.E_INVALID, 'null argument (action)', action__ptr=None)
    q(lo.E_INVALID, 'null argument (q)', q=None)
    q(lo.E_INVALID, 'obs.stride_inner = 17 is below the row width 18', obs__stride_inner=17)
    q(lo.E_INVALID, 'action.stride_inner = -6 is below the row width 7', action__stride_inner=-6)
    q(lo.E_INVALID, 'q_stride = 0 is below the row width 1', q_stride=0)
    q(lo.E_INVALID, 'q overlaps obs', q=MEM + 4 * (F * (N - 1) + D - 1))
    q(lo.E_INVALID, 'q overlaps action', q=MEM + 4 * (F * (N - 1) + D + K - 1))            # past the last obs, on the last action
    q(lo.E_INVALID, 'q overlaps idx', q=IDX + 8 * 255)
    # ---- target
    t = lambda *a, **k: refused('atacom_offpolicy_target', _valid_target, *a, **k)          # noqa: E731
    for n in (0, 3):
        t(lo.E_INVALID, 'n_critics = %d' % n, n_critics=n)
    t(lo.E_INVALID, 'the two critics differ', critics__1__kind=lo.DDPG)
    t(lo.E_INVALID, 'the two critics differ', critics__1__n_obs=D - 1)
    t(lo.E_INVALID, 'the two critics differ', critics__1__n_act=K - 1)
    t(lo.E_INVALID, 'actor.struct_size', actor__struct_size=ctypes.sizeof(_lib.AtacomMlp) - 4)
    t(lo.E_UNSUPPORTED, 'only 64 hidden units', actor__hidden=32)
    t(lo.E_INVALID, 'the actor maps 17 to 7', actor__n_in=D - 1)
    t(lo.E_INVALID, 'the actor maps 18 to 6', actor__n_out=K - 1)
    t(lo.E_UNSUPPORTED, 'actor: activation = 2', actor__activation=2)
    t(lo.E_INVALID, 'null argument (a weight or bias of the actor)', actor__W2=None)
    t(lo.E_UNSUPPORTED, 'sigma network', actor__sW1=0x1000)
    t(lo.E_UNSUPPORTED, 'squash', actor__squash=1)
    t(lo.E_UNSUPPORTED, 'mean_mode = 2', actor__mean_mode=2)
    t(lo.E_INVALID, 'noise_std must be >= 0', noise_std=-0.1)
    t(lo.E_INVALID, 'noise_std must be >= 0', noise_std=float('nan'))
    t(lo.E_INVALID, 'noise_clip must be >= 0', noise_clip=-0.5)
    t(lo.E_INVALID, 'noise_clip must be >= 0', noise_clip=float('inf'))
    t(lo.E_INVALID, 'gamma must be finite', gamma=float('inf'))
    t(lo.E_INVALID, 'gamma must be finite', gamma=float('nan'))
    t(lo.E_INVALID, 'act_low and act_high are given together', act_high=None)
    t(lo.E_INVALID, 'act_low and act_high are given together', act_low=None)
    t(lo.E_INVALID, 'null argument (next_obs, reward or absorbing)', reward__ptr=None)
    t(lo.E_INVALID, 'null argument (y)', y=None)
    t(lo.E_INVALID, 'next_obs.stride_inner = 17 is below the row width 18', next_obs__stride_inner=17)
    t(lo.E_INVALID, 'eps_stride = 6 is below the row width 7', eps_stride=6)
    t(lo.E_INVALID, 'y_stride = 0 is below the row width 1', y_stride=0)
    t(lo.E_INVALID, 'action_out_stride = 6 is below the row width 7', action_out_stride=6)
    t(lo.E_INVALID, 'y overlaps next_obs', y=MEM + 4 * (D + K + 1))
    t(lo.E_INVALID, 'y overlaps reward', y=MEM + 4 * (D + K) - 4 * 255)
    t(lo.E_INVALID, 'y overlaps absorbing', y=MEM + 4 * (F * (N - 1) + 2 * D + K + 1))
    t(lo.E_INVALID, 'y overlaps eps', y=EPS + 4 * (256 * K - 1))
    t(lo.E_INVALID, 'y overlaps idx', y=IDX)
    t(lo.E_INVALID, 'action_out overlaps eps', action_out=EPS - 4 * (256 * K - 1))
    t(lo.E_INVALID, 'y overlaps action_out', action_out=Y - 4 * (256 * K - 1))
    # ---- soft update
    s = lambda *a, **k: refused('atacom_offpolicy_soft_update', _valid_soft, *a, **k)          # noqa: E731
    assert lib.atacom_offpolicy_soft_update(None) == lo.E_INVALID and 'null argument' in msg()
    s(lo.E_INVALID, 'struct_size', struct_size=8)
    s(lo.E_INVALID, 'device', device=-1)
    s(lo.E_UNSUPPORTED, 'no kernel for dtype 2', dtype=2)
    for n in (0, 5):
        s(lo.E_INVALID, 'n_pairs = %d is outside 1 .. 4' % n, n_pairs=n)
    for tau in (-1e-3, 1.5, float('nan')):
        s(lo.E_INVALID, 'tau must be in [0, 1]', tau=tau)
    s(lo.E_UNSUPPORTED, 'pairs[1]: n_in = 33', pairs__1__n_in=33)
    s(lo.E_UNSUPPORTED, 'pairs[0]: n_out = 9', pairs__0__n_out=9)
    s(lo.E_UNSUPPORTED, 'pairs[1]: n_act = 9', pairs__1__n_act=9)
    s(lo.E_INVALID, 'pairs[0]: null argument (W2a)', pairs__0__n_act=2)
    a = _valid_soft(lo)
    a.pairs[1].online[2] = None
    assert lib.atacom_offpolicy_soft_update(a) == lo.E_INVALID and 'pairs[1]: null argument (W2)' in msg()
    a = _valid_soft(lo)
    a.pairs[0].target[3] = a.pairs[0].target[3] + 2
    assert lib.atacom_offpolicy_soft_update(a) == lo.E_INVALID and 'must be aligned' in msg()
    for (pj, i), (qj, qi, side), words in (((1, 0), (0, 0, 'target'), 'pairs[0].target.W1 overlaps pairs[1].target.W1'),      # across pairs
                                          ((0, 1), (0, 0, 'target'), 'pairs[0].target.W1 overlaps pairs[0].target.b1'),      # within a pair
                                          ((1, 6), (1, 6, 'online'), 'pairs[1].target.W2a overlaps pairs[1].online.W2a'),     # its own online
                                          ((0, 2), (1, 4, 'online'), 'pairs[0].target.W2 overlaps pairs[1].online.W3')):
        a = _valid_soft(lo)
        a.pairs[pj].target[i] = getattr(a.pairs[qj], side)[qi] + 4
        assert lib.atacom_offpolicy_soft_update(a) == lo.E_INVALID and words in msg(), msg()
    # What passes every check fails only at the device, which does not exist: the valid calls, one critic, no eps, no bounds, no
    # idx, a repeated input row, adjacent buffers, an online set shared by two pairs, tau at both ends
    for fn, valid, changes in (('atacom_offpolicy_q', _valid_q, (dict(), dict(idx=None), dict(obs__stride_inner=0), dict(q=IDX + 8 * 256),
                                                                 dict(critic__kind=lo.DDPG, critic__n_obs=32, critic__n_act=8))),
                               ('atacom_offpolicy_target', _valid_target, (dict(), dict(n_critics=1), dict(eps=None), dict(act_low=None, act_high=None),
                                                                           dict(action_out=None), dict(idx=None, y=Y, action_out=None, eps=None),
                                                                           dict(actor__mean_mode=0), dict(y=EPS + 4 * 256 * K))),
                               ('atacom_offpolicy_soft_update', _valid_soft, (dict(), dict(tau=0.0), dict(tau=1.0), dict(n_pairs=1)))):
        for change in changes:
            a = _apply(valid(lo), change)
            a.device = 1 << 20
            assert getattr(lib, fn)(a) == lo.E_HIP, (fn, change, msg())
    a = _valid_soft(lo)
    for i in range(6):
        a.pairs[1].n_in, a.pairs[1].n_out, a.pairs[1].n_act = D, K, 0
        a.pairs[1].online[i] = a.pairs[0].online[i]
    a.device = 1 << 20
    assert lib.atacom_offpolicy_soft_update(a) == lo.E_HIP, msg()
    a = _valid_target(lo)
    a.actor.struct_size = _lib.AtacomMlp.mean_mode.offset            # ATACOM_MLP_SIZE_V1: accepted, runs mean_mode 0
    a.device = 1 << 20
    assert lib.atacom_offpolicy_target(a) == lo.E_HIP, msg()
    with pytest.raises(AtacomError, match='null argument'):
        lo.check(lib.atacom_offpolicy_q(None))


def test_python_arguments_are_refused_before_the_library_is_called(monkeypatch):
    import torch
    from rl_on_manifold_amd import MlpPolicy, QCritic, RecordLayout, ReplayMemory, offpolicy

    def never(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(offpolicy._lo, 'load', never)
    lin = lambda o, i: (torch.zeros(o, i), torch.zeros(o))          # noqa: E731
    pol = MlpPolicy(*lin(64, 4), *lin(64, 64), *lin(2, 64))
    cr = QCritic(*lin(64, 6), *lin(64, 64), torch.zeros(64, 2), *lin(1, 64), kind='td3')
    dd = QCritic(*lin(64, 4), *lin(64, 64), torch.zeros(64, 2), *lin(1, 64), kind='ddpg')
    assert (cr.n_obs, cr.n_act, dd.n_obs, dd.n_act) == (4, 2, 4, 2)
    x, a, r = torch.zeros(5, 4), torch.zeros(5, 2), torch.zeros(5)
    for call, words in ((lambda: offpolicy.q_values(cr, x, a), 'run on a GPU'),
                        (lambda: offpolicy.td_target(pol, cr, x, r, r, 0.99), 'run on a GPU'),
                        (lambda: offpolicy.soft_update(cr, dd, 0.5), 'differ in shape'),
                        (lambda: offpolicy.soft_update(cr, cr, 1.5), 'tau must be in'),
                        (lambda: offpolicy.soft_update([cr] * 5, [cr] * 5, 0.5), '1 to 4 pairs'),
                        (lambda: offpolicy.soft_update(cr, cr, 0.5), 'run on a GPU'),
                        (lambda: offpolicy.q_values(pol, x, a), 'critic must be a QCritic'),
                        (lambda: QCritic(*lin(64, 6), *lin(64, 64), torch.zeros(64, 2), *lin(1, 64), kind='sac'), "kind must be"),
                        (lambda: QCritic(*lin(64, 2), *lin(64, 64), torch.zeros(64, 2), *lin(1, 64), kind='td3'), 'first layer'),
                        (lambda: ReplayMemory(0, 4, 2, device='cpu'), 'capacity must be >= 1'),
                        (lambda: ReplayMemory(8, 4, 2, device='cpu').sample(3), 'the memory is empty')):
        with pytest.raises(ValueError, match=words):
            call()

    class Net(torch.nn.Module):
        def __init__(self, n1):
            super().__init__()
            self._h1, self._h2_s, self._h2_a, self._h3 = (torch.nn.Linear(n1, 64), torch.nn.Linear(64, 64),
                                                          torch.nn.Linear(2, 64, bias=False), torch.nn.Linear(64, 1))
            self._action_scaling = torch.tensor([0.5, 2.0])
    assert QCritic.from_module(Net(6), 4).kind == 'td3' and QCritic.from_module(Net(4), 4).kind == 'ddpg'
    assert QCritic.from_module(Net(6), 4).tensors['act_scale'].tolist() == [0.5, 2.0]
    with pytest.raises(ValueError, match='_h1 takes 5 inputs'):
        QCritic.from_module(Net(5), 4)
    # the memory's bookkeeping needs no GPU: it is host integers and torch indexing
    mem = ReplayMemory(7, 4, 2, device='cpu')
    rows = torch.arange(15 * mem.F, dtype=torch.float32).reshape(15, mem.F)
    mem.add_fields(rows[:, :4], rows[:, 4:6], rows[:, 6], rows[:, 7:11], rows[:, 11], rows[:, 12])
    assert (mem.head, mem.size) == (1, 7) and torch.equal(mem.storage[1:], rows[8:14]) and torch.equal(mem.storage[0], rows[14])
    assert mem.initialized(7) and not mem.initialized(8) and int(mem.sample(100).max()) < 7
    # tensors on another device than the storage are refused by name, before anything is written
    before, away = mem.storage.clone(), rows.to('meta')
    with pytest.raises(ValueError, match="the fields live on meta, the memory's storage on cpu"):
        mem.add_fields(rows[:, :4], rows[:, 4:6], rows[:, 6], away[:, 7:11], rows[:, 11], rows[:, 12])
    with pytest.raises(ValueError, match="the records live on meta"):
        mem.add(RecordLayout([5], 4, 2), away.reshape(3, 5, mem.F))
    assert (mem.head, mem.size) == (1, 7) and torch.equal(mem.storage, before)


@abi.needs_llvm('llvm-readelf')
def test_kernel_census_and_resources(off_lib, tmp_path):
    """Eighteen kernels (the module docstring).  Float32: no scratch, at most 256 registers (two wavefronts per SIMD) and 63808
    bytes of LDS -- one network block MlpLdsM<.., 64, 8>::NET = 7752 floats with W2a in the unread rows of its W3 block, 8
    floats, and 4 wavefronts x 2048 of staging -- which is <= 65536.  Float64: MlpLds<4 CH, 64, 8>::TOTAL + 512 doubles."""
    ks = abi.kernel_rows(off_lib, tmp_path)
    want = ['k_offpolicy_net<%s, %d>' % (t, ch) for t in ('float', 'double') for ch in range(1, 9)] + ['k_soft_update<float>', 'k_soft_update<double>']
    assert [k[0] for k in ks] == sorted(want), ks
    for name, lds, scratch, vgpr, agpr, code in ks:
        print('%-30s VGPR %3d AGPR %3d scratch %d LDS %d code %d' % (name, vgpr, agpr, scratch, lds, code))
        assert lds <= 65536, (name, lds)
        if 'soft' in name:
            assert lds == 0 and scratch == 0, name
            continue
        ch = int(name[-2])
        if 'float' in name:
            assert scratch == 0 and vgpr <= 256, (name, scratch, vgpr)
            assert lds == 4 * (7752 + 8 + 4 * 2048) == 63808, (name, lds)
        else:
            total = 64 * (4 * ch + 4) + 64 * 68 + 64 * 8 + 64 + 64 + 8 + 4 * ch + 4 * ch + 8 + 40        # MlpLds<4 CH, 64, 8>::TOTAL
            assert lds == 8 * (total + 512), (name, lds)
            assert vgpr <= 512, (name, vgpr)


@abi.needs_llvm('llvm-objdump')
def test_the_float32_kernels_run_on_the_matrix_cores(off_lib, tmp_path):
    seen = 0
    for _, head, body in abi.function_bodies(off_lib, tmp_path):
        k = re.search(r'k_(offpolicy_net<(float|double), (\d)>|soft_update<(float|double)>)', head)
        if not k:
            continue
        seen += 1
        mfma = len(re.findall(r'\bv_mfma_f32_16x16x4[_f32]*\b', body))
        if k.group(2) == 'float':
            # per block of 16 rows: 4 CH (layer 1) + 64 (W2 h1) + 2 x 4 (the action steps, each behind its uniform branch) + 16 (layer
            # 3), four blocks; the phases are a loop, so the forward pass is in the code once
            assert mfma == 4 * (4 * int(k.group(3)) + 64 + 8 + 16), (head, mfma)
        else:
            assert mfma == 0, (head, mfma)
    assert seen == 18


def test_exec_mask_audit_finds_nothing(off_lib):
    abi.exec_audit(off_lib)


def test_python_surface():
    import rl_on_manifold_amd as pkg
    from rl_on_manifold_amd import offpolicy

    def params(fn):
        return [(p.name, p.kind is p.KEYWORD_ONLY, None if p.default is p.empty else p.default)
                for p in inspect.signature(fn).parameters.values()]

    pos = lambda *names: [(n, False, None) for n in names]          # noqa: E731
    assert params(pkg.q_values) == pos('critic', 'obs', 'action') + [('idx', True, None), ('out', True, None), ('n_blocks', True, 0)]
    assert params(pkg.td_target) == pos('actor', 'critics', 'next_obs', 'reward', 'absorbing', 'gamma') + [
        ('eps', True, None), ('noise_std', True, 0.0), ('noise_clip', True, 0.0), ('low', True, None), ('high', True, None),
        ('idx', True, None), ('out', True, None), ('action_out', True, None), ('n_blocks', True, 0)]
    assert params(pkg.soft_update) == pos('targets', 'onlines', 'tau')
    assert [p[0] for p in params(pkg.QCritic.__init__)] == ['self', 'W1', 'b1', 'W2', 'b2', 'W2a', 'W3', 'b3', 'kind', 'act_scale',
                                                            'obs_shift', 'obs_scale', 'activation']
    assert [p[0] for p in params(pkg.ReplayMemory.__init__)] == ['self', 'capacity', 'obs_dim', 'n_null', 'dtype', 'device']
    for name in ('add', 'add_compact', 'add_fields', 'sample', 'initialized', 'q_values', 'td_target', 'columns'):
        assert callable(getattr(pkg.ReplayMemory, name)), name
    assert pkg.q_values is offpolicy.q_values and pkg.ReplayMemory is offpolicy.ReplayMemory and pkg.QCritic is offpolicy.QCritic
