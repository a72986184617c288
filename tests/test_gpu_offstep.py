"""GPU tests of libatacom_offstep.so (rl_on_manifold_amd/offstep.py): the tracked Adam step is bit-equal to the libraries that are
already verified (optim.Adam for p, m, v and the head of plain networks, soft_update for the targets), critic groups are bit-equal
in float32 to the numpy restatement of tests/offstep_oracle.py and within 1e-12 of scale of torch.optim.Adam plus the torch
target expression in float64, a group without a gradient keeps its bits while its target moves, tau has two exact ends, nothing
outside the named buffers is written, one launch of four groups gives the bits of four launches of one, and GraphedFit replays
what its eager body and the hand-written sequence of the existing calls compute, which in float64 is a torch module / autograd /
torch.optim.Adam loop in MushroomRL's order.

The shapes are offstep_oracle.SHAPES: the smallest and the largest plain network, a point-sized DDPG critic and the largest
critic -- segments shorter than the workgroup (b3: one value) and longer (W2: 4096 values), W2a absent and present."""
import copy
import os
import struct
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import offstep_oracle as fo                                   # noqa: E402

DEV = 'cuda:0'
DT = {'f32': torch.float32, 'f64': torch.float64}
NP = {'f32': np.float32, 'f64': np.float64}
PAD = 16                                                      # border elements on each side of a framed buffer
BORDER = 24680.0
BYTE = 0x5a
SCALE = 0.5                                                   # grad_scale of every raw group: a power of two is exact, not 1


def _framed(values):
    """`values` (numpy, 1-d) on the device inside a larger buffer with patterned borders -> (buffer, the view of the values)."""
    t = torch.from_numpy(np.array(values))                   # a writable copy
    if t.dtype == torch.uint8:
        buf = torch.full((t.numel() + 128,), BYTE, dtype=torch.uint8, device=DEV)
        mid = buf[64:64 + t.numel()]
    else:
        buf = torch.full((t.numel() + 2 * PAD,), BORDER, dtype=t.dtype, device=DEV)
        mid = buf[PAD:PAD + t.numel()]
    mid.copy_(t)
    return buf, mid


def _borders_intact(buf, mid):
    lo = (mid.data_ptr() - buf.data_ptr()) // buf.element_size()
    pat = BYTE if buf.dtype == torch.uint8 else BORDER
    return bool((buf[:lo] == pat).all()) and bool((buf[lo + mid.numel():] == pat).all())


class Raw:
    """Groups driven through the C ABI itself, every buffer framed: one per shape, from offstep_oracle.case.  `targets[k]` says
    whether group k has a target network."""

    def __init__(self, dt, shapes=fo.SHAPES, targets=None):
        from rl_on_manifold_amd import _lib_offstep as ls
        self.ls, self.lib, self.dt, self.shapes = ls, ls.load(), dt, shapes
        self.code = ls.F32 if dt == 'f32' else ls.F64
        self.targets = [True] * len(shapes) if targets is None else targets
        self.cases = [fo.case(s, NP[dt]) for s in shapes]
        self.groups = []
        for shape, c, has in zip(shapes, self.cases, self.targets):
            g, o = dict(frames={}), 0
            for name, shp in fo.segments(*shape):
                n = int(np.prod(shp))
                g['frames'][name] = _framed(c['p'][o:o + n])
                if has:
                    g['frames']['t_' + name] = _framed(c['target'][o:o + n])
                o += n
            assert o == c['p'].size == fo.group_size(*shape)
            g['grads'] = [_framed(gr) for gr in c['grads']]
            size = self.lib.atacom_offstep_state_size(self.code, *shape)
            assert size == 32 + 2 * o * (4 if dt == 'f32' else 8)
            g['frames']['state'] = _framed(np.full(size, 0xa5, dtype=np.uint8))      # init must overwrite every byte
            self.groups.append(g)

    def args(self, which, grads, tau=fo.TAU, lr=fo.LR):
        """`grads[i]`: the number of the gradient that group which[i] takes, or None."""
        from rl_on_manifold_amd._rows import stream as _stream
        ls = self.ls
        a = ls.new_args()
        a.device, a.dtype, a.n_groups = 0, self.code, len(which)
        a.beta1, a.beta2, a.eps, a.tau, a.stream = fo.BETAS[0], fo.BETAS[1], fo.EPS, tau, _stream(0)
        for s, k, t in zip(a.groups, which, grads):
            g, shape = self.groups[k], self.shapes[k]
            s.n_in, s.n_out, s.n_act, s.lr, s.grad_scale = shape[0], shape[1], shape[2], lr, SCALE
            for j, (name, _) in enumerate(fo.segments(*shape)):
                setattr(s, name, g['frames'][name][1].data_ptr())
                if self.targets[k]:
                    s.target[j] = g['frames']['t_' + name][1].data_ptr()
            s.state = g['frames']['state'][1].data_ptr()
            s.grad = None if t is None else g['grads'][t][1].data_ptr()
        return a

    def init(self):
        n = len(self.groups)
        self.ls.check(self.lib.atacom_offstep_adam_init(self.args(list(range(n)), [None] * n)))

    def step(self, t, which=None, tau=fo.TAU):
        """Step number t (its gradient) of the groups `which`; t = None: no group is stepped."""
        which = list(range(len(self.groups))) if which is None else which
        self.ls.check(self.lib.atacom_offstep_adam_step(self.args(which, [t] * len(which), tau)))

    def read(self, k):
        g, shape = self.groups[k], self.shapes[k]
        N = fo.group_size(*shape)
        st = g['frames']['state'][1].cpu().numpy().tobytes()
        step, b1p, b2p, reserved = struct.unpack('<qddq', st[:32])
        mv = np.frombuffer(st[32:], dtype=NP[self.dt])
        p = np.concatenate([g['frames'][name][1].cpu().numpy() for name, _ in fo.segments(*shape)])
        tg = np.concatenate([g['frames']['t_' + name][1].cpu().numpy() for name, _ in fo.segments(*shape)]) if self.targets[k] else None
        return dict(p=p, m=mv[:N].copy(), v=mv[N:].copy(), target=tg, head=(step, b1p, b2p), reserved=reserved)

    def bits(self):
        return [torch.cat([mid.view(torch.uint8).reshape(-1) for name, (_, mid) in g['frames'].items()]).clone() for g in self.groups]

    def check_frames(self):
        for k, (g, c) in enumerate(zip(self.groups, self.cases)):
            for name, (buf, mid) in g['frames'].items():
                assert _borders_intact(buf, mid), (k, name)
            for t, (buf, mid) in enumerate(g['grads']):                 # a gradient is an input: borders and contents
                assert _borders_intact(buf, mid), (k, 'grad', t)
                assert np.array_equal(mid.cpu().numpy().view(np.uint8), c['grads'][t].view(np.uint8)), (k, t)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------- plain groups: the bits of optim.Adam and soft_update
def _plain(dt, shape, c, what):
    from rl_on_manifold_amd import MlpPolicy
    ts, o = [], 0
    for name, shp in fo.segments(*shape):
        n = int(np.prod(shp))
        ts.append(torch.from_numpy(np.array(c[what][o:o + n])).reshape(shp).to(DEV))
        o += n
    return MlpPolicy(*ts)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_plain_groups_have_the_bits_of_optim_adam_and_soft_update(dt):
    """Three steps of the two plain shapes in one launch, targets attached: p, m, v and the whole head are bit-equal to three
    optim.Adam steps, the targets to soft_update called after each of them."""
    from rl_on_manifold_amd import Adam, TrackedAdam, soft_update, _lib_fit as lf
    from rl_on_manifold_amd.fit import Gradients
    shapes = [s for s in fo.SHAPES if s[2] == 0]
    cases = [fo.case(s, NP[dt]) for s in shapes]
    mine = [(_plain(dt, s, c, 'p'), _plain(dt, s, c, 'target')) for s, c in zip(shapes, cases)]
    theirs = [(_plain(dt, s, c, 'p'), _plain(dt, s, c, 'target')) for s, c in zip(shapes, cases)]
    grads = []
    for s in shapes:
        key = (s[0], s[1], lf.VALUE, DT[dt], torch.device(DEV))
        grads.append(Gradients(s[0], s[1], lf.VALUE, DT[dt], torch.device(DEV), 16, key))
    tracked = TrackedAdam([dict(net=n, target=t, scale=SCALE, lr=lr) for (n, t), lr in zip(mine, (1e-4, 3e-4))], tau=fo.TAU)
    adam = Adam([dict(net=n, scale=SCALE, lr=lr) for (n, _), lr in zip(theirs, (1e-4, 3e-4))])
    for step in range(3):
        for g, c in zip(grads, cases):
            g.flat.copy_(torch.from_numpy(np.array(c['grads'][step])))
        tracked.step(*grads)
        adam.step(*grads)
        soft_update([t for _, t in theirs], [n for n, _ in theirs], fo.TAU)
        for k, ((n, t), (rn, rt)) in enumerate(zip(mine, theirs)):
            for name in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
                assert torch.equal(n.tensors[name], rn.tensors[name]), (step, k, name)
                assert torch.equal(t.tensors[name], rt.tensors[name]), (step, k, 'target', name)
            assert torch.equal(tracked.groups[k]['state'], adam.groups[k]['state']), (step, k)      # head, m and v: every byte
    assert tracked.steps() == adam.steps() == [3, 3]
    for (n, t), s, c in zip(mine, shapes, cases):            # and both have moved
        assert not torch.equal(n.tensors['W2'], _plain(dt, s, c, 'p').tensors['W2'])
        assert not torch.equal(t.tensors['W2'], _plain(dt, s, c, 'target').tensors['W2'])


# ---------------------------------------------------------------------- all four shapes against the restatements
_torch_runs = {}


def _torch64(shape):
    """Three steps of torch.optim.Adam (fed SCALE * grad) and the torch target expression in float64, per step: made once."""
    if shape not in _torch_runs:
        c = fo.case(shape, np.float64)
        par = torch.nn.Parameter(torch.from_numpy(np.array(c['p'])))
        tgt = torch.from_numpy(np.array(c['target']))
        opt = torch.optim.Adam([par], lr=fo.LR, betas=fo.BETAS, eps=fo.EPS)
        out = []
        for t in range(3):
            before = par.detach().clone()
            par.grad = torch.from_numpy(SCALE * c['grads'][t])
            opt.step()
            with torch.no_grad():
                scale_t = fo.TAU * par.abs() + (1.0 - fo.TAU) * tgt.abs()
                tgt = fo.TAU * par + (1.0 - fo.TAU) * tgt
            st = opt.state[par]
            out.append(dict(p=par.detach().numpy().copy(), m=st['exp_avg'].numpy().copy(), v=st['exp_avg_sq'].numpy().copy(),
                            target=tgt.numpy().copy(),
                            scale=dict(p=before.abs().numpy() + (par.detach() - before).abs().numpy(),
                                       m=st['exp_avg'].abs().numpy() + np.abs(SCALE * c['grads'][t]), v=st['exp_avg_sq'].numpy().copy(),
                                       target=scale_t.numpy())))
        _torch_runs[shape] = out
    return _torch_runs[shape]


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_three_steps_of_every_shape_against_the_restatements(dt):
    """One launch of FOUR groups per step, from a state that atacom_offstep_adam_init made over a 0xa5 pattern.  float32: p, m, v
    and the target are bit-equal to the numpy float32 restatement (every operation is individually rounded, there is no exp, sqrt
    and the division are correctly rounded on both sides).  float64: within 1e-12 of scale + 1e-14 of torch.optim.Adam followed by
    the torch target expression.  The head is what the float64 running products give, bit for bit; borders and gradients are
    untouched."""
    raw = Raw(dt)
    raw.init()
    mine = []
    for c in raw.cases:
        N = c['p'].size
        mine.append(dict(p=c['p'], m=np.zeros(N, NP[dt]), v=np.zeros(N, NP[dt]), head=fo.fresh_head(), target=c['target']))
    for k in range(len(raw.groups)):
        got = raw.read(k)
        assert got['head'] == fo.fresh_head() and got['reserved'] == 0 and not got['m'].any() and not got['v'].any()
    tracked = fo.tracked32 if dt == 'f32' else fo.tracked64
    for t in range(3):
        raw.step(t)
        torch.cuda.synchronize()
        raw.check_frames()
        for k, (shape, c) in enumerate(zip(raw.shapes, raw.cases)):
            got, o = raw.read(k), mine[k]
            o = tracked(o['p'], c['grads'][t], o['m'], o['v'], o['head'], o['target'], scale=SCALE)
            mine[k] = o
            assert got['head'] == o['head'] and got['head'][0] == t + 1 and got['reserved'] == 0, (shape, t)
            if dt == 'f32':
                for q in ('p', 'm', 'v', 'target'):
                    differ = int((got[q].view(np.uint32) != o[q].view(np.uint32)).sum())
                    print('%s step %d %s: %d of %d elements differ in bits from the numpy float32 restatement' % (shape, t + 1, q, differ, got[q].size))
                    assert differ == 0, (shape, t, q, differ)
            else:
                ref = _torch64(shape)[t]
                for q in ('p', 'm', 'v', 'target'):
                    err, bound = np.abs(got[q] - ref[q]), 1e-12 * ref['scale'][q] + 1e-14
                    print('%s step %d %s: worst |error| / (1e-12 scale + 1e-14) against torch %.3g' % (shape, t + 1, q, (err / bound).max()))
                    assert np.isfinite(got[q]).all() and (err <= bound).all(), (shape, t, q, (err / bound).max())


# ---------------------------------------------------------------------- grad = NULL, the ends of tau, nothing else written
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_a_group_without_a_gradient_keeps_its_bits_while_its_target_moves(dt):
    """After one real step (so that m, v and the head are not the fresh ones): in ONE launch group 0 takes no gradient and has a
    target, group 1 takes none and has none, group 2 is stepped without a target, group 3 is stepped with one."""
    targets = [True, False, False, True]
    raw = Raw(dt, targets=targets)
    raw.init()
    raw.step(0)
    before = [raw.read(k) for k in range(4)]
    bits = raw.bits()
    n = raw.ls
    n.check(raw.lib.atacom_offstep_adam_step(raw.args([0, 1, 2, 3], [None, None, 1, 1])))
    torch.cuda.synchronize()
    raw.check_frames()
    after = [raw.read(k) for k in range(4)]
    for k in (0, 1):                                         # not stepped: p, m, v and the whole head keep their bits
        assert all(_same(after[k][q], before[k][q]) for q in ('p', 'm', 'v')) and after[k]['head'] == before[k]['head'] == (1, 0.9, 0.999)
    assert torch.equal(raw.bits()[1], bits[1])               # no gradient and no target: not one byte of the group changes
    assert _same(after[0]['target'], fo.follow(before[0]['p'], before[0]['target'], fo.TAU, NP[dt]))
    assert not _same(after[0]['target'], before[0]['target'])
    for k in (2, 3):                                         # stepped: the second step of the restatement
        b = before[k]
        tracked = fo.tracked32 if dt == 'f32' else fo.tracked64
        o = tracked(b['p'], raw.cases[k]['grads'][1], b['m'], b['v'], b['head'], b['target'], scale=SCALE)
        assert after[k]['head'] == o['head'] and after[k]['head'][0] == 2
        if dt == 'f32':
            assert all(_same(after[k][q], o[q]) for q in ('p', 'm', 'v'))
            assert o['target'] is None or _same(after[k]['target'], o['target'])
        assert not _same(after[k]['p'], b['p'])
        if targets[k]:                                       # the target follows the p JUST WRITTEN, in both precisions
            assert _same(after[k]['target'], fo.follow(after[k]['p'], b['target'], fo.TAU, NP[dt]))
    # the ends of tau on groups that take no gradient: 0 leaves the target's bits, 1 makes them the parameter's
    now = raw.read(0)
    raw.step(None, which=[0, 3], tau=0.0)
    assert _same(raw.read(0)['target'], now['target']) and _same(raw.read(3)['target'], after[3]['target'])
    raw.step(None, which=[0, 3], tau=1.0)
    for k in (0, 3):
        got = raw.read(k)
        assert _same(got['target'], got['p']) and _same(got['p'], after[k]['p']) and _same(got['m'], after[k]['m'])
        assert got['head'] == after[k]['head']
    torch.cuda.synchronize()
    raw.check_frames()


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_one_launch_of_four_groups_gives_the_bits_of_four_launches_of_one(dt):
    """A 4-group launch, four 1-group launches, two 2-group launches in another order: the same bits in every parameter,
    target, moment and head after two steps; a launch that names two of the four leaves the other two as they were."""
    runs = []
    for plan in ([[0, 1, 2, 3]], [[0], [1], [2], [3]], [[3, 0], [2, 1]]):
        raw = Raw(dt)
        raw.init()
        for t in range(2):
            for which in plan:
                raw.step(t, which)
        torch.cuda.synchronize()
        raw.check_frames()
        runs.append(raw.bits())
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    raw = Raw(dt)
    raw.init()
    before = raw.bits()
    for t in range(2):
        raw.step(t, [1, 2])
    after = raw.bits()
    assert torch.equal(before[0], after[0]) and torch.equal(before[3], after[3])
    assert torch.equal(after[1], runs[0][1]) and torch.equal(after[2], runs[0][2])


# ---------------------------------------------------------------------- GraphedFit
D, K, M, ROWS = 6, 2, 256, 1024
GAMMA, TAU, LR_A, LR_C = 0.99, 5e-3, 1e-4, 3e-4
# (policy_delay, critics, noise_std, noise_clip, bounded): a DDPG fit and a TD3 pair of fits
CONFIGS = {'ddpg': (1, 1, 0.0, 0.0, False), 'td3': (2, 2, 0.2, 0.5, True)}


class Actor(torch.nn.Module):              # tests/test_offgrad_oracle.py's Actor: relu, no normalisation, s * tanh
    def __init__(self, s):
        super().__init__()
        self._h1, self._h2, self._h3 = torch.nn.Linear(D, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, K)
        self.s = s

    def forward(self, x):
        return self.s * torch.tanh(self._h3(torch.relu(self._h2(torch.relu(self._h1(x))))))


class Critic(torch.nn.Module):             # tests/test_offgrad_oracle.py's Critic: relu, no normalisation, both kinds
    def __init__(self, s, kind):
        super().__init__()
        self._h1, self._h2_s = torch.nn.Linear(D + K if kind == 'td3' else D, 64), torch.nn.Linear(64, 64)
        self._h2_a, self._h3 = torch.nn.Linear(K, 64, bias=False), torch.nn.Linear(64, 1)
        self.s, self.kind = s, kind

    def forward(self, s, a):
        a = a / self.s
        h1 = torch.relu(self._h1(torch.cat((s, a), -1) if self.kind == 'td3' else s))
        return self._h3(torch.relu(self._h2_s(h1) + self._h2_a(a))).squeeze(-1)


_setups = {}


def _setup(name):
    """The float64 CPU modules, the rows of the memory and three replays' worth of row numbers and noise: made once per
    configuration and never written to (the tests work on copies)."""
    if name not in _setups:
        delay, nc, _, _, _ = CONFIGS[name]
        gen = torch.Generator().manual_seed(11 + delay)
        torch.manual_seed(5 + delay)
        s = torch.tensor([1.0, 0.5], dtype=torch.float64)
        actor = Actor(s).double()
        critics = [Critic(s, name).double() for _ in range(nc)]
        actor_t, critics_t = Actor(s).double(), [Critic(s, name).double() for _ in range(nc)]      # targets that DIFFER from the nets
        rows = dict(obs=torch.randn(ROWS, D, generator=gen, dtype=torch.float64), action=torch.rand(ROWS, K, generator=gen, dtype=torch.float64) * 2 - 1,
                    reward=torch.randn(ROWS, generator=gen, dtype=torch.float64), next_obs=torch.randn(ROWS, D, generator=gen, dtype=torch.float64),
                    absorbing=(torch.rand(ROWS, generator=gen) < 0.1).double(), last=torch.zeros(ROWS, dtype=torch.float64))
        rows['action'] = rows['action'] * s
        idx = torch.randint(0, ROWS, (3, delay, M), generator=gen)
        eps = torch.randn(3, delay, M, K, generator=gen, dtype=torch.float64)
        _setups[name] = dict(s=s, actor=actor, critics=critics, actor_t=actor_t, critics_t=critics_t, rows=rows, idx=idx, eps=eps)
    return _setups[name]


def _device_side(name, dt):
    """-> (mem, pol, pol_t, cri, cri_t, optimizer, idx, eps, kwargs of the target) on the device in `dt`, from copies."""
    from rl_on_manifold_amd import MlpPolicy, QCritic, ReplayMemory, TrackedAdam
    su = _setup(name)
    delay, nc, noise_std, noise_clip, bounded = CONFIGS[name]
    t = lambda x: x.detach().to(DT[dt]).to(DEV).contiguous().clone()      # noqa: E731
    s = t(su['s'])

    def policy(net):
        pol = MlpPolicy(*(t(p) for lay in (net._h1, net._h2, net._h3) for p in (lay.weight, lay.bias)))
        pol.mean_mode, pol.tensors['act_scale'] = 1, s
        return pol

    def critic(net):
        return QCritic(t(net._h1.weight), t(net._h1.bias), t(net._h2_s.weight), t(net._h2_s.bias), t(net._h2_a.weight), t(net._h3.weight),
                       t(net._h3.bias), kind=name, act_scale=s)

    pol, pol_t = policy(su['actor']), policy(su['actor_t'])
    cri, cri_t = [critic(c) for c in su['critics']], [critic(c) for c in su['critics_t']]
    mem = ReplayMemory(ROWS, D, K, dtype=DT[dt], device=DEV)
    r = su['rows']
    mem.add_fields(*(t(r[f]) for f in ('obs', 'action', 'reward', 'next_obs', 'absorbing', 'last')))
    assert mem.size == ROWS
    opt = TrackedAdam([dict(net=pol, target=pol_t, lr=LR_A)] + [dict(net=c, target=ct, lr=LR_C) for c, ct in zip(cri, cri_t)], tau=TAU)
    kw = dict(noise_std=noise_std, noise_clip=noise_clip)
    if bounded:
        kw.update(low=-s, high=s.clone())
    return mem, pol, pol_t, cri, cri_t, opt, su['idx'].to(DEV), t(su['eps']), kw


def _by_hand(mem, pol, pol_t, cri, cri_t, opt, idx, eps, kw):
    """One graph's worth of fits, written out with the existing calls and fresh buffers: MushroomRL's order."""
    for j in range(idx.shape[0]):
        y = mem.td_target(pol_t, cri_t, idx[j], GAMMA, eps=eps[j] if kw['noise_std'] > 0 else None, **kw)
        gq = mem.critic_gradient(cri, idx[j], y)
        if j == 0:                                           # fit_count % policy_delay == 0: the actor's fit
            opt.step(None, *gq, only=tuple(range(1, 1 + len(cri))))      # the critic fit and the critics' targets
            ga = mem.actor_gradient(pol, cri[0], idx[j])                 # through the UPDATED first critic
            opt.step(ga, *([None] * len(cri)), only=(0,))                # the actor's step, then its target
        else:
            opt.step(None, *gq)                              # the critic fit; every target follows


def _torch_loop(name):
    """Three replays' worth of fits as a torch module / autograd / torch.optim.Adam / torch soft-update loop in float64, in
    MushroomRL's order (DDPG.fit): critic fit, the actor's update through the updated critic when fit_count % policy_delay == 0,
    then both target updates -> {group: dict(params, targets, m, v)} as flat float64 arrays in the order of a group."""
    su = _setup(name)
    delay, nc, noise_std, noise_clip, bounded = CONFIGS[name]
    actor, critics = copy.deepcopy(su['actor']), copy.deepcopy(su['critics'])
    actor_t, critics_t = copy.deepcopy(su['actor_t']), copy.deepcopy(su['critics_t'])
    opt_a = torch.optim.Adam(actor.parameters(), lr=LR_A)
    opt_c = torch.optim.Adam([p for c in critics for p in c.parameters()], lr=LR_C)
    r, s = su['rows'], su['s']
    fit_count = 0
    for rep in range(3):
        for j in range(delay):
            idx, eps = su['idx'][rep, j], su['eps'][rep, j]
            obs, act, nxt = r['obs'][idx], r['action'][idx], r['next_obs'][idx]
            with torch.no_grad():
                a = actor_t(nxt)
                if noise_std > 0:
                    a = a + torch.clamp(noise_std * eps, -noise_clip, noise_clip)
                if bounded:
                    a = torch.minimum(torch.maximum(a, -s), s)
                q = critics_t[0](nxt, a)
                for c in critics_t[1:]:
                    q = torch.minimum(q, c(nxt, a))
                y = r['reward'][idx] + GAMMA * ((1.0 - r['absorbing'][idx]) * q)
            opt_c.zero_grad(set_to_none=True)
            sum(((c(obs, act) - y) ** 2).mean() for c in critics).backward()
            opt_c.step()
            if fit_count % delay == 0:
                opt_a.zero_grad(set_to_none=True)
                (-critics[0](obs, actor(obs)).mean()).backward()
                opt_a.step()
            with torch.no_grad():
                for net, tgt in zip([actor] + critics, [actor_t] + critics_t):
                    for p, tp in zip(net.parameters(), tgt.parameters()):
                        tp.copy_(TAU * p + (1.0 - TAU) * tp)
            fit_count += 1

    def order(net):                                          # W1, b1, W2, b2, W3, b3 (, W2a): the order of a group
        if isinstance(net, Actor):
            return [p for lay in (net._h1, net._h2, net._h3) for p in (lay.weight, lay.bias)]
        return [net._h1.weight, net._h1.bias, net._h2_s.weight, net._h2_s.bias, net._h3.weight, net._h3.bias, net._h2_a.weight]

    out = []
    for net, tgt, opt in zip([actor] + critics, [actor_t] + critics_t, [opt_a] + [opt_c] * nc):
        out.append(dict(params=[p.detach().numpy() for p in order(net)], targets=[p.detach().numpy() for p in order(tgt)],
                        m=np.concatenate([opt.state[p]['exp_avg'].numpy().reshape(-1) for p in order(net)]),
                        v=np.concatenate([opt.state[p]['exp_avg_sq'].numpy().reshape(-1) for p in order(net)]),
                        step=int(opt.state[order(net)[0]]['step'])))
    return out


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_graphed_fit_is_the_eager_body_the_hand_written_sequence_and_the_torch_loop(name, dt):
    from rl_on_manifold_amd import GraphedFit
    delay, nc, _, _, _ = CONFIGS[name]
    mem, pol, pol_t, cri, cri_t, opt, idx, eps, kw = _device_side(name, dt)
    start = opt.snapshot()
    fit = GraphedFit(mem, pol, pol_t, cri if nc == 2 else cri[0], cri_t if nc == 2 else cri_t[0], opt, M, GAMMA, policy_delay=delay, **kw)
    torch.cuda.synchronize()
    assert _equal(opt.snapshot(), start)                     # construction: warm-up and capture undone, bit for bit
    assert opt.steps() == [0] * (1 + nc)
    for rep in range(3):
        fit.replay(idx[rep], eps[rep])
    replayed = opt.snapshot()
    assert opt.steps() == [3] + [3 * delay] * nc and not _equal(replayed, start)
    assert all(not torch.equal(a, b) for a, b in zip(replayed, start))      # every state, parameter and target has moved
    opt.restore(start)
    for rep in range(3):
        fit.eager(idx[rep], eps[rep])
    assert _equal(opt.snapshot(), replayed)
    opt.restore(start)
    for rep in range(3):
        _by_hand(mem, pol, pol_t, cri, cri_t, opt, idx[rep], eps[rep], kw)
    assert _equal(opt.snapshot(), replayed)
    if dt == 'f64':                                          # within 1e-10 of each tensor's scale of the torch loop
        worst = 0.0
        for k, (g, ref) in enumerate(zip(opt.groups, _torch_loop(name))):
            assert int(g['step'].item()) == ref['step']
            pairs = [('p%d' % i, t, r) for i, (t, r) in enumerate(zip(g['params'], ref['params']))] + \
                    [('t%d' % i, t, r) for i, (t, r) in enumerate(zip(g['targets'], ref['targets']))] + \
                    [('m', g['m'], ref['m']), ('v', g['v'], ref['v'])]
            for what, t, r in pairs:
                got = t.cpu().numpy().reshape(-1)
                err, scale = np.abs(got - r.reshape(-1)).max(), np.abs(r).max()
                worst = max(worst, err / scale)
                assert np.isfinite(got).all() and err <= 1e-10 * scale, (k, what, err / scale)
        print('%s: worst |error| / scale against the torch loop %.3g' % (name, worst))
    # a static tensor that has been REPLACED (not refilled in place) is refused, by replay and by eager
    opt.restore(start)
    kept = pol.tensors['W2']
    pol.tensors['W2'] = kept.clone()
    for call in (fit.replay, fit.eager):
        with pytest.raises(RuntimeError, match='has moved since the capture'):
            call(idx[0], eps[0])
    pol.tensors['W2'] = kept
    torch.cuda.synchronize()
    assert _equal(opt.snapshot(), start)                     # the refused calls ran nothing
    fit.replay()                                             # fresh row numbers and noise, drawn into the static buffers
    torch.cuda.synchronize()
    assert int(fit.idx.min()) >= 0 and int(fit.idx.max()) < ROWS and bool(torch.isfinite(fit.critic_losses[0]))
    assert all(bool(torch.isfinite(t).all()) for t in opt.snapshot() if t.dtype != torch.uint8)
