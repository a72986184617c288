"""CPU-only checks of libatacom_soft.so, a SAC update on the device: the header is plain C11, the declared symbols are exactly
the exported ones and the ctypes table, the ctypes structs have gcc's layout, every argument rule is enforced without a GPU and
with a message, workspace_size, the overlap checks, and the code objects are what DESIGN.md section 7h says (float32 without
scratch; registers and LDS).  No compute call is made (no GPU here).

The kernel census: fifty-two kernels.  k_soft_target<T, CH>, k_soft_critic<T, CH> and k_soft_actor<T, CH> for T = float, double
and CH = ceil((D + k) / 4) = 1 .. 8 of the critics' first layer, k_soft_reduce<T> and k_soft_alpha<T>."""
import ctypes
import subprocess

import pytest

import abi_tools as abi

FUNCTIONS = ('version', 'last_error', 'workspace_size', 'target', 'critic_gradient', 'actor_gradient', 'alpha_step')


@pytest.fixture(scope='module')
def soft_lib():
    from rl_on_manifold_amd import build
    return build.build('soft', verbose=False)


def test_header_is_plain_c11(tmp_path):
    abi.compile_c11(tmp_path, abi.INCLUDE, '#include "atacom_soft_hip.h"\n'
                    'int main(void) {\n'
                    '    atacom_soft_target_args t = {0};\n'
                    '    atacom_soft_critic_args c = {0};\n'
                    '    atacom_soft_actor_args a = {0};\n'
                    '    atacom_soft_alpha_args s = {0};\n'
                    '    t.struct_size = sizeof t; c.struct_size = sizeof c; a.struct_size = sizeof a; s.struct_size = sizeof s;\n'
                    '    a.policy.struct_size = sizeof a.policy; a.policy.hidden = ATACOM_SOFT_HIDDEN; c.critics[1].n_act = 1;\n'
                    '    if (ATACOM_SOFT_MAX_IN != 32 || ATACOM_SOFT_MAX_ACT != 8 || ATACOM_SOFT_STATS != 4 || ATACOM_SOFT_ALPHA_STATE != 48) return 1;\n'
                    '    if (atacom_soft_target(&t) == ATACOM_SOFT_OK || atacom_soft_critic_gradient(&c) == ATACOM_SOFT_OK) return 2;\n'
                    '    if (atacom_soft_actor_gradient(&a) == ATACOM_SOFT_OK || atacom_soft_alpha_step(&s) == ATACOM_SOFT_OK) return 2;\n'
                    '    if (atacom_soft_workspace_size(ATACOM_SOFT_F32, 2, 23, 1, 256, 0) == 0) return 3;\n'
                    '    return !atacom_soft_version() || !atacom_soft_last_error(); }\n')


def test_declared_exported_and_bound_symbols_are_one_set(soft_lib):
    from rl_on_manifold_amd import _lib_soft
    names = abi.one_symbol_set(soft_lib, 'atacom_soft_hip.h', 'atacom_soft_', _lib_soft)
    assert names == sorted('atacom_soft_' + n for n in FUNCTIONS)
    assert _lib_soft.load().atacom_soft_version().startswith(b'atacom_soft')


def test_the_ctypes_structs_have_the_layout_of_the_header(tmp_path):
    """sizeof and the offset of every field, as gcc lays the header out."""
    from rl_on_manifold_amd import _lib_soft as ls
    structs = {'atacom_soft_critic': ls.Critic, 'atacom_soft_target_args': ls.TargetArgs, 'atacom_soft_critic_args': ls.CriticArgs,
               'atacom_soft_actor_args': ls.ActorArgs, 'atacom_soft_alpha_args': ls.AlphaArgs}
    body = ''
    for cname, S in structs.items():
        body += '    printf("%%zu", sizeof(%s));\n' % cname
        body += ''.join('    printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in S._fields_) + '    printf("\\n");\n'
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include "atacom_soft_hip.h"\nint main(void) {\n' + body +
                   '    printf("%d %d %d %d %d %d\\n", ATACOM_SOFT_MAX_IN, ATACOM_SOFT_MAX_ACT, ATACOM_SOFT_HIDDEN, ATACOM_SOFT_MAX_BLOCKS, '
                   'ATACOM_SOFT_STATS, ATACOM_SOFT_ALPHA_STATE);\n    return 0; }\n')
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c11', '-I', abi.INCLUDE, str(src), '-o', exe])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, (cname, S) in zip(lines, structs.items()):
        assert [int(x) for x in line.split()] == [ctypes.sizeof(S)] + [getattr(S, f).offset for f, _ in S._fields_], cname
    assert [int(x) for x in lines[-1].split()] == [ls.MAX_IN, ls.MAX_ACT, ls.HIDDEN, ls.MAX_BLOCKS, ls.STATS, ls.ALPHA_STATE]
    assert ls.grad_size(23, 1) == 64 * 23 + 64 + 4096 + 64 + 64 + 1


MEM, IDX, TGT, GRAD, STATS, AOUT, DQ, WS, EPS, LA, Y, LP, QO = (0x100000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000, 0x900000,
                                                                 0xb00000, 0xc00000, 0xd00000, 0xe00000, 0xf00000)
N, D, K = 1000, 18, 5
F = 2 * D + K + 3


def _critic(ls, **kw):
    c = ls.Critic()
    c.n_obs, c.n_act, c.activation = D, K, 0
    for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
        setattr(c, k, 0x1000)                            # never dereferenced
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _policy():
    return abi.fake_mlp(n_in=D, n_out=K, squash=1, sW1=0x1000, sb1=0x1000, sW2=0x1000, sb2=0x1000, sW3=0x1000, sb3=0x1000,
                        log_std_min=-20.0, log_std_max=2.0)


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


def _valid_target(ls):
    """256 rows gathered through idx from the columns of a [1000, F] memory: passes every check."""
    a = ls.new_args(ls.TargetArgs)
    a.device, a.dtype, a.n_outer, a.n_inner, a.n_critics = 0, ls.F32, 1, N, 2
    a.policy = _policy()
    a.critics[0], a.critics[1] = _critic(ls), _critic(ls)
    a.next_obs, a.reward, a.absorbing = ls.View(MEM + 4 * (D + K + 1), 0, F), ls.View(MEM + 4 * (D + K), 0, F), ls.View(MEM + 4 * (2 * D + K + 1), 0, F)
    a.eps, a.eps_stride, a.log_alpha, a.gamma, a.idx, a.n_idx = EPS, K, LA, 0.99, IDX, 256
    a.y, a.y_stride, a.action_out, a.action_out_stride, a.logp_out, a.logp_out_stride = Y, 1, AOUT, K, LP, 1
    return a


def _valid_critic(ls):
    a = ls.new_args(ls.CriticArgs)
    a.device, a.dtype, a.n_outer, a.n_inner, a.n_critics = 0, ls.F32, 1, N, 2
    a.critics[0], a.critics[1] = _critic(ls), _critic(ls)
    a.obs, a.action = ls.View(MEM, 0, F), ls.View(MEM + 4 * D, 0, F)
    a.target, a.target_stride, a.idx, a.n_idx = TGT, 1, IDX, 256
    a.grad[0], a.grad[1], a.stats[0], a.stats[1] = GRAD, GRAD + 0x40000, STATS, STATS + 0x100
    a.workspace = WS
    a.workspace_bytes = ls.load().atacom_soft_workspace_size(ls.F32, 2, D + K, 1, 256, 0)
    return a


def _valid_actor(ls):
    a = ls.new_args(ls.ActorArgs)
    a.device, a.dtype, a.n_outer, a.n_inner = 0, ls.F32, 1, N
    a.policy = _policy()
    a.critics[0], a.critics[1] = _critic(ls), _critic(ls)
    a.obs = ls.View(MEM, 0, F)
    a.eps, a.eps_stride, a.log_alpha, a.target_entropy, a.idx, a.n_idx = EPS, K, LA, -5.0, IDX, 256
    a.grad_mu, a.grad_sigma, a.stats = GRAD, GRAD + 0x40000, STATS
    a.action_out, a.action_out_stride, a.logp_out, a.logp_out_stride = AOUT, K, LP, 1
    a.q_out, a.q_out_stride, a.dqda_out, a.dqda_out_stride = QO, 2, DQ, K
    a.workspace = WS
    a.workspace_bytes = ls.load().atacom_soft_workspace_size(ls.F32, 2, D, K, 256, 0)
    return a


def _valid_alpha(ls):
    a = ls.new_args(ls.AlphaArgs)
    a.device, a.dtype, a.log_alpha, a.grad, a.state = 0, ls.F32, LA, STATS + 8, GRAD
    a.lr, a.beta1, a.beta2, a.eps = 3e-4, 0.9, 0.999, 1e-8
    return a


def test_workspace_size(soft_lib):
    from rl_on_manifold_amd import _lib_soft as ls
    lib = ls.load()
    size = lib.atacom_soft_workspace_size
    q = ls.grad_size(23, 1) + ls.STATS
    assert size(ls.F32, 1, 23, 1, 256, 0) == (1 * q * 4 + 255) // 256 * 256                 # one tile of 4 x 64 rows
    assert size(ls.F32, 2, 23, 1, 257, 0) == (2 * 2 * q * 4 + 255) // 256 * 256
    assert size(ls.F64, 2, 23, 1, 257, 0) == (2 * 17 * q * 8 + 255) // 256 * 256            # tiles of 16 rows
    assert size(ls.F32, 1, 23, 1, 1 << 20, 0) == (512 * q * 4 + 255) // 256 * 256           # the ceiling of the library's choice
    assert size(ls.F32, 1, 23, 1, 16, 7) == (7 * q * 4 + 255) // 256 * 256
    qa = ls.grad_size(18, 5) + ls.STATS
    assert size(ls.F32, 2, 18, 5, 256, 0) == (2 * qa * 4 + 255) // 256 * 256
    for args, words in (((2, 1, 23, 1, 16, 0), 'no kernel for dtype 2'), ((0, 3, 23, 1, 16, 0), 'n_nets = 3'), ((0, 1, 33, 1, 16, 0), 'n_in = 33'),
                        ((0, 1, 23, 9, 16, 0), 'n_out = 9'), ((0, 1, 23, 1, 0, 0), 'rows = 0'), ((0, 1, 23, 1, 16, 65536), 'n_blocks = 65536')):
        assert size(*args) == 0 and words in lib.atacom_soft_last_error().decode(), args


def test_arguments_are_validated_without_a_gpu(soft_lib):
    from rl_on_manifold_amd import _lib_soft as ls
    lib = ls.load()

    def msg():
        return lib.atacom_soft_last_error().decode()

    def refused(fn, valid, code, words, **change):
        a = _apply(valid(ls), change)
        assert getattr(lib, fn)(a) == code, (fn, change, msg())
        assert words in msg() and fn in msg(), (fn, change, msg())

    calls = (('atacom_soft_target', _valid_target, ls.TargetArgs), ('atacom_soft_critic_gradient', _valid_critic, ls.CriticArgs),
             ('atacom_soft_actor_gradient', _valid_actor, ls.ActorArgs))
    for fn, valid, cls in calls:
        ref = lambda *a, **k: refused(fn, valid, *a, **k)          # noqa: E731
        assert getattr(lib, fn)(None) == ls.E_INVALID and 'null argument' in msg() and fn in msg()
        ref(ls.E_INVALID, 'struct_size', struct_size=ctypes.sizeof(cls) - 8)
        ref(ls.E_INVALID, 'device', device=-1)
        ref(ls.E_UNSUPPORTED, 'no kernel for dtype 2', dtype=2)
        ref(ls.E_INVALID, 'n_outer must be >= 1', n_outer=0)
        ref(ls.E_INVALID, 'n_inner must be >= 1', n_inner=0)
        ref(ls.E_UNSUPPORTED, 'rows is too many', n_outer=1 << 31, n_inner=2)
        ref(ls.E_INVALID, 'n_blocks must be >= 1', n_blocks=-1)
        ref(ls.E_UNSUPPORTED, 'exceeds the launch grid', n_blocks=65536)
        ref(ls.E_INVALID, 'n_idx must be >= 1 with idx', n_idx=0)
        ref(ls.E_UNSUPPORTED, 'n_act = 9', critics__0__n_act=9)
        ref(ls.E_UNSUPPORTED, 'n_act = 0', critics__0__n_act=0)
        ref(ls.E_UNSUPPORTED, 'first-layer inputs exceed 32', critics__0__n_obs=28)
        ref(ls.E_UNSUPPORTED, 'activation = 2', critics__1__activation=2)
        ref(ls.E_INVALID, 'null argument (a weight or bias of the critic)', critics__1__W2=None)
        ref(ls.E_INVALID, 'the two critics differ', critics__1__n_obs=D - 1)
        ref(ls.E_INVALID, 'obs_shift must be aligned', critics__0__obs_shift=0x1002)
    for fn, valid, _ in (calls[0], calls[2]):                      # the calls that take the policy
        ref = lambda *a, **k: refused(fn, valid, *a, **k)          # noqa: E731
        ref(ls.E_INVALID, 'policy.struct_size', policy__struct_size=8)
        ref(ls.E_UNSUPPORTED, 'only 64 hidden units', policy__hidden=32)
        ref(ls.E_INVALID, 'the policy maps', policy__n_out=K - 1)
        ref(ls.E_UNSUPPORTED, 'without a sigma network', policy__sW2=None)
        ref(ls.E_UNSUPPORTED, 'without squash', policy__squash=0)
        ref(ls.E_INVALID, 'log_std_min must be below log_std_max', policy__log_std_min=3.0)
        ref(ls.E_INVALID, 'null argument (a weight or bias of the mu network)', policy__b3=None)
        ref(ls.E_INVALID, 'null argument (eps)', eps=None)
        ref(ls.E_INVALID, 'null argument (log_alpha)', log_alpha=None)
        ref(ls.E_INVALID, 'eps_stride = 4 is below the row width 5', eps_stride=4)
        ref(ls.E_INVALID, 'act_scale must be aligned', act_scale=0x1002)
        ref(ls.E_INVALID, 'action_out_stride = 4 is below the row width 5', action_out_stride=4)
        ref(ls.E_INVALID, 'action_out overlaps eps', action_out=EPS + 4)
        ref(ls.E_INVALID, 'logp_out overlaps log_alpha', logp_out=LA)
    refused('atacom_soft_target', _valid_target, ls.E_UNSUPPORTED, 'n_critics = 1', n_critics=1)
    refused('atacom_soft_target', _valid_target, ls.E_INVALID, 'gamma must be finite', gamma=float('inf'))
    refused('atacom_soft_target', _valid_target, ls.E_INVALID, 'null argument (y)', y=None)
    refused('atacom_soft_target', _valid_target, ls.E_INVALID, 'null argument (next_obs, reward or absorbing)', reward__ptr=None)
    refused('atacom_soft_target', _valid_target, ls.E_INVALID, 'y overlaps next_obs', y=MEM + 4 * F)
    refused('atacom_soft_target', _valid_target, ls.E_INVALID, 'y overlaps action_out', action_out=Y)
    refused('atacom_soft_target', _valid_target, ls.E_INVALID, 'next_obs.stride_inner = 17 is below the row width 18', next_obs__stride_inner=17)
    cr = lambda *a, **k: refused('atacom_soft_critic_gradient', _valid_critic, *a, **k)      # noqa: E731
    cr(ls.E_INVALID, 'n_critics = 3', n_critics=3)
    cr(ls.E_INVALID, 'null argument (target)', target=None)
    cr(ls.E_INVALID, 'null argument (grad[1] or stats[1])', grad__1=None)
    cr(ls.E_INVALID, 'null argument (workspace)', workspace=None)
    cr(ls.E_INVALID, 'workspace must be aligned to 16 bytes', workspace=WS + 8)
    cr(ls.E_INVALID, 'that atacom_soft_workspace_size gives', workspace_bytes=1024)
    cr(ls.E_INVALID, 'grad[0] overlaps grad[1]', grad__1=GRAD + 64)
    cr(ls.E_INVALID, 'grad[0] overlaps obs', grad__0=MEM + 0x100)
    cr(ls.E_INVALID, 'stats[1] overlaps target', stats__1=TGT + 8)
    cr(ls.E_INVALID, 'workspace overlaps idx', idx=WS + 64)
    ac = lambda *a, **k: refused('atacom_soft_actor_gradient', _valid_actor, *a, **k)        # noqa: E731
    ac(ls.E_INVALID, 'target_entropy must be finite', target_entropy=float('nan'))
    ac(ls.E_INVALID, 'null argument (grad_mu, grad_sigma or stats)', grad_sigma=None)
    ac(ls.E_INVALID, 'grad_mu overlaps grad_sigma', grad_sigma=GRAD + 64)
    ac(ls.E_INVALID, 'q_out_stride = 1 is below the row width 2', q_out_stride=1)
    ac(ls.E_INVALID, 'q_out overlaps dqda_out', dqda_out=QO + 8)
    ac(ls.E_INVALID, 'stats overlaps log_alpha', stats=LA)
    ac(ls.E_INVALID, 'that atacom_soft_workspace_size gives', workspace_bytes=1024)
    al = lambda *a, **k: refused('atacom_soft_alpha_step', _valid_alpha, *a, **k)            # noqa: E731
    assert lib.atacom_soft_alpha_step(None) == ls.E_INVALID
    al(ls.E_INVALID, 'struct_size', struct_size=8)
    al(ls.E_UNSUPPORTED, 'no kernel for dtype 3', dtype=3)
    al(ls.E_INVALID, 'null argument (log_alpha, grad or state)', state=None)
    al(ls.E_INVALID, 'state must be aligned', state=GRAD + 4)
    al(ls.E_INVALID, 'lr must be >= 0', lr=-1.0)
    al(ls.E_INVALID, 'beta1 and beta2 must be in [0, 1)', beta2=1.0)
    al(ls.E_INVALID, 'eps must be > 0', eps=0.0)
    al(ls.E_INVALID, 'log_alpha overlaps grad', grad=LA)
    al(ls.E_INVALID, 'state overlaps grad', grad=GRAD + 40)


def test_the_python_layer_refuses_before_the_library():
    """Wrong devices, shapes and dtypes raise ValueError without a GPU."""
    torch = pytest.importorskip('torch')
    from rl_on_manifold_amd import MlpPolicy, SoftCritic, soft_actor_gradient, soft_critic_gradient, soft_td_target, AlphaAdam
    z = lambda *s: torch.zeros(*s)                                                         # noqa: E731
    net = lambda i, o: (z(64, i), z(64), z(64, 64), z(64), z(o, 64), z(o))                   # noqa: E731
    crs = [SoftCritic(*net(D + K, 1), n_act=K) for _ in range(2)]
    pol = MlpPolicy(*net(D, K), sigma_weights=net(D, K), squash=True)
    obs, act, eps, la = z(40, D), z(40, K), z(40, K), z(1)
    with pytest.raises(ValueError, match='run on a GPU'):
        soft_critic_gradient(crs, obs, act, z(40))
    with pytest.raises(ValueError, match='run on a GPU'):
        soft_actor_gradient(pol, crs, obs, eps, la, -5.0)
    with pytest.raises(ValueError, match='run on a GPU'):
        soft_td_target(pol, crs, obs, z(40), z(40), 0.99, la, eps)
    with pytest.raises(ValueError, match='target must be a tensor of shape'):
        soft_critic_gradient(crs, obs, act, z(39))
    with pytest.raises(ValueError, match='pair of SoftCritic'):
        soft_actor_gradient(pol, crs[:1], obs, eps, la, -5.0)
    with pytest.raises(ValueError, match='sigma network and squash'):
        soft_actor_gradient(MlpPolicy(*net(D, K)), crs, obs, eps, la, -5.0)
    with pytest.raises(ValueError, match='the policy maps'):
        soft_actor_gradient(MlpPolicy(*net(D, K - 1), sigma_weights=net(D, K - 1), squash=True), crs, obs, eps, la, -5.0)
    with pytest.raises(ValueError, match='eps must be a tensor of shape'):
        soft_actor_gradient(pol, crs, obs, z(40, K + 1), la, -5.0)
    with pytest.raises(ValueError, match='log_alpha must be a tensor of one'):
        soft_actor_gradient(pol, crs, obs, eps, z(2), -5.0)
    with pytest.raises(ValueError, match='float32 or float64'):
        soft_actor_gradient(pol, crs, obs.half(), eps, la, -5.0)
    with pytest.raises(ValueError, match='target_entropy must be finite'):
        soft_actor_gradient(pol, crs, obs, eps, la, float('nan'))
    with pytest.raises(ValueError, match='gamma must be finite'):
        soft_td_target(pol, crs, obs, z(40), z(40), float('inf'), la, eps)
    with pytest.raises(ValueError, match='n_blocks must be 0'):
        soft_critic_gradient(crs, obs, act, z(40), n_blocks=-1)
    with pytest.raises(ValueError, match='run on a GPU'):
        AlphaAdam(la)
    with pytest.raises(ValueError, match='one float32 or float64 value'):
        AlphaAdam(z(2))


@abi.needs_llvm('llvm-readelf')
def test_the_code_objects_are_what_the_design_says(soft_lib, tmp_path):
    """Fifty-two kernels; every float32 kernel without scratch, 63808 bytes of LDS (one network resident and 8 KB of staging per
    wavefront), within the 512 registers of one wavefront per SIMD; the register counts DESIGN.md section 7h records."""
    rows = abi.kernel_rows(soft_lib, tmp_path)
    names = [r[0] for r in rows]
    want = ['k_soft_%s<%s, %d>' % (k, t, ch) for k in ('target', 'critic', 'actor') for t in ('float', 'double') for ch in range(1, 9)]
    want += ['k_soft_reduce<%s>' % t for t in ('float', 'double')] + ['k_soft_alpha<%s>' % t for t in ('float', 'double')]
    assert sorted(names) == sorted(want)
    f32 = [r for r in rows if r[0].startswith(('k_soft_target<float', 'k_soft_critic<float', 'k_soft_actor<float'))]
    for name, lds, scratch, vgpr, agpr, _ in f32:
        assert scratch == 0 and lds == 63808 and vgpr <= 512, (name, lds, scratch, vgpr, agpr)
    worst = {k: max(r[3] for r in f32 if r[0].startswith('k_soft_%s<' % k)) for k in ('target', 'critic', 'actor')}
    print(worst)
    assert worst['target'] <= 176 and worst['critic'] <= 376 and worst['actor'] <= 472          # 164, 360, 453 (+ slack)
    assert all(r[2] == 0 for r in rows if r[0].startswith(('k_soft_reduce', 'k_soft_alpha')))
    assert all(r[1] <= 65536 for r in rows)
