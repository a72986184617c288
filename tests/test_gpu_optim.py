"""GPU tests of libatacom_optim.so (rl_on_manifold_amd/optim.py): the Adam step against the float64 oracle of
tests/optim_oracle.py -- single teacher-forced steps at t = 1, 2, 10 and 1000 in both dtypes (float32 inside the derived bound on
EVERY element of p, m, v and std, float64 to 1e-12 of the element's scale + 1e-14), twenty carried steps from a state that
atacom_optim_adam_init made, a zero gradient, patterned borders around every buffer, launches of 1, 2 and 4 groups of different
shapes, the interplay with the gradients of fit.py against torch.optim.Adam, and GraphedUpdate against the eager sequence of
the same calls.  The shapes are the four of optim_oracle.SHAPES: N = 4353 .. 6800, the smallest and the largest a group can
be (four to seven values a thread of the 1024), with and without log std."""
import copy
import os
import struct
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_oracle as oo                                     # noqa: E402

DEV = 'cuda:0'
DT = {'f32': torch.float32, 'f64': torch.float64}
NP = {'f32': np.float32, 'f64': np.float64}
PAD = 16                                                      # border elements on each side of a framed buffer
BORDER = 24680.0
BYTE = 0x5a


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


def _state_bytes(head, m, v):
    return np.frombuffer(struct.pack('<qddq', head[0], head[1], head[2], 0) + m.tobytes() + v.tobytes(), dtype=np.uint8)


class Raw:
    """Groups driven through the C ABI itself, every buffer framed: one per oracle case (p, grad, m, v, head)."""

    def __init__(self, dt, cases):
        from rl_on_manifold_amd import _lib_optim as lo
        self.lo, self.lib, self.dt, self.cases = lo, lo.load(), dt, cases
        self.groups = []
        for c in cases:
            n_in, n_out, has = c['shape']
            g, o = dict(frames={}, n_std=c['n_std']), 0
            for name, shape in oo.segments(*c['shape']):
                n = int(np.prod(shape))
                g['frames'][name] = _framed(c['p'][o:o + n])
                o += n
            assert o == c['p'].size
            if has:
                g['frames']['std'] = _framed(np.full(n_out, -1.0, dtype=NP[dt]))
            g['frames']['grad'] = _framed(c['grad'])
            g['frames']['state'] = _framed(_state_bytes(c['head'], c['m'], c['v']))
            assert g['frames']['state'][1].numel() == self.lib.atacom_optim_state_size(lo.F32 if dt == 'f32' else lo.F64, n_in, n_out, int(has))
            self.groups.append(g)

    def args(self, which, lr=oo.LR):
        from rl_on_manifold_amd._rows import stream as _stream
        lo = self.lo
        a = lo.new_args()
        a.device, a.dtype, a.n_groups = 0, lo.F32 if self.dt == 'f32' else lo.F64, len(which)
        a.beta1, a.beta2, a.eps, a.stream = oo.BETAS[0], oo.BETAS[1], oo.EPS, _stream(0)
        for s, k in zip(a.groups, which):
            g, c = self.groups[k], self.cases[k]
            s.n_in, s.n_out, s.lr, s.grad_scale = c['shape'][0], c['shape'][1], lr, c['scale']
            for name, (_, mid) in g['frames'].items():
                setattr(s, name, mid.data_ptr())
        return a

    def step(self, which=None):
        self.lo.check(self.lib.atacom_optim_adam_step(self.args(list(range(len(self.groups))) if which is None else which)))

    def init(self):
        self.lo.check(self.lib.atacom_optim_adam_init(self.args(list(range(len(self.groups))))))

    def read(self, k):
        g, c = self.groups[k], self.cases[k]
        N = c['p'].size
        st = g['frames']['state'][1].cpu().numpy().tobytes()
        step, b1p, b2p, reserved = struct.unpack('<qddq', st[:32])
        mv = np.frombuffer(st[32:], dtype=NP[self.dt])
        p = np.concatenate([g['frames'][name][1].cpu().numpy() for name, _ in oo.segments(*c['shape'])])
        std = g['frames']['std'][1].cpu().numpy() if 'std' in g['frames'] else np.zeros(0, dtype=NP[self.dt])
        return dict(p=p, m=mv[:N].copy(), v=mv[N:].copy(), std=std, head=(step, b1p, b2p), reserved=reserved)

    def bits(self):
        return [torch.cat([mid.view(torch.uint8).reshape(-1) for name, (_, mid) in g['frames'].items()]).clone() for g in self.groups]

    def check_frames(self):
        for k, (g, c) in enumerate(zip(self.groups, self.cases)):
            for name, (buf, mid) in g['frames'].items():
                assert _borders_intact(buf, mid), (k, name)
            assert np.array_equal(g['frames']['grad'][1].cpu().numpy().view(np.uint8), c['grad'].view(np.uint8)), k    # grad is an input


_worst = {}


@pytest.mark.parametrize('dt', ['f32', 'f64'])
@pytest.mark.parametrize('t', oo.STEPS)
def test_single_teacher_forced_steps(dt, t):
    """One launch of FOUR groups, the four shapes, each from the oracle's state before step t: p, m, v and std inside the
    bound on every element, the head what the float64 running products give bit for bit, the borders of every buffer and the
    whole of grad untouched.  Reported, not asserted: whether float32 is bit-equal to the numpy float32 restatement."""
    cases = [oo.case(shape, t, NP[dt]) for shape in oo.SHAPES]
    raw = Raw(dt, cases)
    raw.step()
    torch.cuda.synchronize()
    raw.check_frames()
    for k, c in enumerate(cases):
        got = raw.read(k)
        assert got['head'] == c['want']['head'] == oo.head_at(t + 1) and got['reserved'] == 0
        w = oo.inside(NP[dt], got, c, (c['shape'], t))
        _worst[dt] = max(_worst.get(dt, 0.0), w)
        if dt == 'f32':
            r = oo.step32(c['p'], c['grad'], c['m'], c['v'], c['head'], scale=c['scale'], n_std=c['n_std'])
            same = {q: int((got[q].view(np.uint32) != r[q].view(np.uint32)).sum()) for q in ('p', 'm', 'v', 'std')}
            print('%s t = %d: elements that differ in bits from the numpy float32 restatement: %s' % (c['shape'], t, same))
    print('%s: worst |error| / bound so far %.4g' % (dt, _worst[dt]))


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_launch_grouping_gives_the_same_bits(dt):
    """A 4-group launch, four 1-group launches, two 2-group launches in another order, and the 4-group launch again from an
    equal state: the same bits in every parameter, moment, head and std."""
    cases = [oo.case(shape, 10, NP[dt]) for shape in oo.SHAPES]
    runs = []
    for plan in ([[0, 1, 2, 3]], [[0], [1], [2], [3]], [[3, 0], [2, 1]], [[0, 1, 2, 3]]):
        raw = Raw(dt, cases)
        for which in plan:
            raw.step(which)
        torch.cuda.synchronize()
        raw.check_frames()
        runs.append(raw.bits())
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    # a launch that names two of the four leaves the other two as they were
    raw = Raw(dt, cases)
    before = raw.bits()
    raw.step([1, 2])
    after = raw.bits()
    assert torch.equal(before[0], after[0]) and torch.equal(before[3], after[3])
    assert torch.equal(after[1], runs[0][1]) and torch.equal(after[2], runs[0][2])


def test_twenty_carried_steps_in_float64_from_an_initialised_state():
    """A 2-group launch (18 -> 5 with log std and std, 25 -> 1 at scale 0.5).  The states start as garbage, adam_init makes them
    fresh (step 0, powers 1, zero moments, nothing outside them touched); twenty steps with new gradients each are those of
    the oracle, step == 20 and both powers bit-equal to the numpy running products."""
    shapes = (oo.SHAPES[2], oo.SHAPES[1])
    cases = [dict(oo.case(s, 1, np.float64)) for s in shapes]
    for c in cases:                                             # garbage where the state will be
        c['m'], c['v'], c['head'] = np.full_like(c['m'], np.nan), np.full_like(c['v'], -3.0), (77, 0.5, 0.25)
    raw = Raw('f64', cases)
    raw.init()
    torch.cuda.synchronize()
    raw.check_frames()
    ref = []
    for k, c in enumerate(cases):
        got = raw.read(k)
        assert got['head'] == oo.fresh_head() and got['reserved'] == 0 and not got['m'].any() and not got['v'].any()
        assert np.array_equal(got['p'], c['p'])
        ref.append(dict(p=c['p'], m=np.zeros_like(c['p']), v=np.zeros_like(c['p']), head=oo.fresh_head()))
    rng = np.random.default_rng(20)
    for t in range(1, 21):
        for k, c in enumerate(cases):
            grad = oo.gradients(rng, c['p'].size)
            raw.groups[k]['frames']['grad'][1].copy_(torch.from_numpy(grad))
            c['grad'] = grad
            o = oo.step64(ref[k]['p'], grad, ref[k]['m'], ref[k]['v'], ref[k]['head'], scale=c['scale'], n_std=c['n_std'])
            ref[k] = o
        raw.step()
    torch.cuda.synchronize()
    raw.check_frames()
    for k, c in enumerate(cases):
        got = raw.read(k)
        assert got['head'] == ref[k]['head'] == oo.head_at(21)
        assert got['head'][0] == 20
        assert got['head'][1] == float(np.multiply.accumulate(np.full(20, 0.9))[-1]) and got['head'][2] == float(np.multiply.accumulate(np.full(20, 0.999))[-1])
        oo.inside(np.float64, got, dict(want=ref[k], bound=None), (c['shape'], 'carried'))


def _nets(dt, n_in, k, seed):
    import torch.nn as nn

    class Net(nn.Module):
        def __init__(self, n_in, n_out):
            super().__init__()
            self._h1, self._h2, self._h3 = nn.Linear(n_in, 64), nn.Linear(64, 64), nn.Linear(64, n_out)

    torch.manual_seed(seed)
    return Net(n_in, k).to(DEV, dt), Net(n_in, 1).to(DEV, dt), torch.full((k,), -0.7, dtype=dt, device=DEV)


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_a_zero_gradient_from_a_fresh_state_leaves_every_parameter_bit_identical(dt):
    from rl_on_manifold_amd import Adam, MlpPolicy, fit
    actor, critic, log_std = _nets(DT[dt], 18, 5, 1)
    std = log_std.exp()
    pol, cri = MlpPolicy.from_module(actor, std=std), MlpPolicy.from_module(critic)
    opt = Adam([dict(net=pol, log_std=log_std, std=std), dict(net=cri, scale=0.5)])
    assert opt.steps() == [0, 0]
    before = [t.clone() for t in opt._tensors()]
    dev = torch.device(DEV)
    gp = fit.Gradients(18, 5, fit._lf.PPO_CLIP, DT[dt], dev, 256, (18, 5, fit._lf.PPO_CLIP, DT[dt], dev))
    gc = fit.Gradients(18, 1, fit._lf.VALUE, DT[dt], dev, 256, (18, 1, fit._lf.VALUE, DT[dt], dev))
    gp.flat.zero_()
    gc.flat.zero_()
    std.fill_(-1.0)
    opt.step(gp, gc)
    assert opt.steps() == [1, 1]
    for g in opt.groups:
        for a, name in zip(g['params'], ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')):
            assert a.data_ptr() == g['net'].tensors[name].data_ptr()
        assert not bool(g['m'].any()) and not bool(g['v'].any())
        assert g['pows'].tolist() == [0.9, 0.999]
    after = list(opt._tensors())
    for k, (a, b) in enumerate(zip(before, after)):
        if a.dtype != torch.uint8 and b.data_ptr() != std.data_ptr():
            assert torch.equal(a, b), k                           # the modules' own storage, unchanged in every bit
    assert torch.equal(actor._h2.weight.detach(), before[3]) and torch.equal(log_std, torch.full_like(log_std, -0.7))
    assert torch.equal(std, log_std.exp()) or float((std - log_std.exp()).abs().max()) <= 2 ** -22      # refreshed: exp(log_std)
    with pytest.raises(ValueError, match='one Gradients per group'):
        opt.step(gp)
    with pytest.raises(ValueError, match=r'grads\[0\] must be the Gradients of a PPO call'):
        opt.step(gc, gp)
    s = opt.snapshot()
    gp.flat.fill_(1.0)
    opt.step(gp, gc)
    assert opt.steps() == [2, 2] and not torch.equal(actor._h2.weight.detach(), before[3])
    opt.restore(s)
    assert opt.steps() == [1, 1] and all(torch.equal(a, b) for a, b in zip(s, opt._tensors()))


def _records(dt, T, B, D, k, pol, compact=False):
    from rl_on_manifold_amd import log_prob_from_records
    from rl_on_manifold_amd.rollout import CompactRecordLayout, RecordLayout
    lay = CompactRecordLayout([B], D, k, T) if compact else RecordLayout([B], D, k)
    g = torch.Generator(device='cpu').manual_seed(5)
    width = lay.Fc if compact else lay.F
    rec = torch.randn((T + compact, B, width), generator=g, dtype=torch.float64).to(DEV, dt)
    rec[..., lay.fields['action']] *= 0.3
    adv = torch.randn((T, B), generator=g, dtype=torch.float64).to(DEV, dt)
    ret = torch.randn((T, B), generator=g, dtype=torch.float64).to(DEV, dt)
    logp_old = log_prob_from_records(lay, rec, pol) + 0.1 * torch.randn((T, B), generator=g, dtype=torch.float64).to(DEV, dt)
    return lay, rec, adv, ret, logp_old.contiguous()


def test_five_updates_with_the_gradients_of_fit_are_those_of_torch_adam():
    """float64, tiny synthetic full records (T = 3, B = 50): five times policy_gradient_from_records +
    value_gradient_from_records + Adam.step, against the SAME Gradients handed to torch.optim.Adam through to_module (the
    critic's at half, the example's 0.5) on copies of the networks: every parameter to 1e-12 (|p| + lr) + 1e-14 after every
    update, std = exp(log_std)."""
    from rl_on_manifold_amd import Adam, MlpPolicy, fit
    dt, T, B, D, k, lr = torch.float64, 3, 50, 6, 2, 1e-2
    actor, critic, log_std = _nets(dt, D, k, 2)
    a_ref, c_ref, ls_ref = copy.deepcopy(actor), copy.deepcopy(critic), log_std.clone().requires_grad_(True)
    ref = torch.optim.Adam(list(a_ref.parameters()) + list(c_ref.parameters()) + [ls_ref], lr=lr)
    std = log_std.exp()
    pol, cri = MlpPolicy.from_module(actor, std=std), MlpPolicy.from_module(critic)
    opt = Adam([dict(net=pol, log_std=log_std, std=std), dict(net=cri, scale=0.5)], lr=lr)
    lay, rec, adv, ret, logp_old = _records(dt, T, B, D, k, pol)
    gp = gc = half = None
    for it in range(5):
        gp = fit.policy_gradient_from_records(lay, rec, adv, logp_old, pol, out=gp)
        gc = fit.value_gradient_from_records(lay, rec, ret, cri, out=gc)
        assert float(gp.flat.abs().max()) > 0 and float(gc.flat.abs().max()) > 0
        half = half or fit.Gradients(D, 1, fit._lf.VALUE, dt, gc.flat.device, 256, gc.key)
        half.flat.copy_(gc.flat * 0.5)
        gp.to_module(a_ref, ls_ref)
        half.to_module(c_ref)
        ref.step()
        opt.step(gp, gc)
        for p0, p1 in zip(list(a_ref.parameters()) + list(c_ref.parameters()) + [ls_ref],
                          list(actor.parameters()) + list(critic.parameters()) + [log_std]):
            err = (p0 - p1).detach().abs()
            assert bool((err <= 1e-12 * (p0.detach().abs() + lr) + 1e-14).all()), (it, float(err.max()))
        assert bool(((std - ls_ref.detach().exp()).abs() <= 1e-12 * std + 1e-14).all())
        assert not torch.equal(log_std, torch.full_like(log_std, -0.7))
    assert opt.steps() == [5, 5]


@pytest.mark.parametrize('compact', [False, True], ids=['full', 'compact'])
def test_graphed_update_is_the_eager_sequence(compact):
    """150 rows in minibatches of 64 (slices of 64, 64 and 22), float32.  Construction leaves parameters and optimiser state
    bit-equal to what they were (the warm-up is undone); two replays with two given permutations are bit-equal to the eager
    sequence of the same calls from the same start -- parameters, log std, std, moments, and step == 6."""
    from rl_on_manifold_amd import Adam, GraphedUpdate, MlpPolicy, fit
    dt, T, B, D, k, mb = torch.float32, 3, 50, 6, 2, 64
    actor, critic, log_std = _nets(dt, D, k, 4)
    std = log_std.exp()
    pol, cri = MlpPolicy.from_module(actor, std=std), MlpPolicy.from_module(critic)
    opt = Adam([dict(net=pol, log_std=log_std, std=std), dict(net=cri, scale=0.5)], lr=1e-2)
    lay, rec, adv, ret, logp_old = _records(dt, T, B, D, k, pol, compact)
    start = opt.snapshot()
    upd = GraphedUpdate(lay, rec, adv, ret, logp_old, pol, cri, opt, mb)
    torch.cuda.synchronize()
    assert upd.n_rows == 150 and [s.numel() for s in upd._slices] == [64, 64, 22] and upd.perm.dtype == torch.int64
    assert all(torch.equal(a, b) for a, b in zip(start, opt._tensors())) and opt.steps() == [0, 0]
    gen = torch.Generator(device='cpu').manual_seed(9)
    perms = [torch.randperm(150, generator=gen).to(DEV) for _ in range(2)]
    for p in perms:
        upd.replay(p)
    torch.cuda.synchronize()
    graphed = opt.snapshot()
    assert opt.steps() == [6, 6] and not torch.equal(graphed[1], start[1])
    opt.restore(start)
    gp = gc = None
    for p in perms:
        for i in range(0, 150, mb):
            idx = p[i:i + mb]
            gp = fit.policy_gradient_from_records(lay, rec, adv, logp_old, pol, clip=0.2, idx=idx, out=gp)
            gc = fit.value_gradient_from_records(lay, rec, ret, cri, idx=idx, out=gc)
            opt.step(gp, gc)
    assert opt.steps() == [6, 6]
    for j, (a, b) in enumerate(zip(graphed, opt._tensors())):
        assert torch.equal(a, b), j
    assert torch.equal(actor._h1.weight.detach(), graphed[1])      # the modules' own storage moved
    # a fresh permutation is drawn into the static buffer; a static tensor that moved is refused
    upd.replay()
    torch.cuda.synchronize()
    assert opt.steps() == [9, 9] and sorted(upd.perm.tolist()) == list(range(150))
    with pytest.raises(ValueError, match='perm must be an int64 tensor of 150'):
        upd.replay(perms[0][:100])
    upd.adv = adv.clone()
    with pytest.raises(RuntimeError, match='has moved since the capture'):
        upd.replay()
