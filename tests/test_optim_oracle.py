"""CPU-only checks of the oracle of libatacom_optim.so (tests/optim_oracle.py): its float64 restatement IS torch.optim.Adam (to
the project's float64 rule, 1e-12 of each value's scale + 1e-14), and its float32 restatement -- the header's order of
operations in numpy float32 -- stays inside the derived bound on every element of every input that the GPU tests use, so the
reference alone satisfies what the device is held to."""
import numpy as np
import pytest

import optim_oracle as oo


def test_the_float64_restatement_is_torch_adam():
    """50 steps of two groups, a 18 -> 5 policy with log std (scale 1) and a 18 -> 1 critic (scale 0.5, torch is fed 0.5 g),
    gradient magnitudes 1e-12 .. 1e3 drawn anew at every step."""
    torch = pytest.importorskip('torch')
    rng = np.random.default_rng(3)
    groups = []
    for shape, scale in (((18, 5, True), 1.0), ((18, 1, False), 0.5)):
        N = oo.group_size(*shape)
        p = rng.normal(0.0, 0.3, N)
        groups.append(dict(shape=shape, scale=scale, p=p, m=np.zeros(N), v=np.zeros(N), head=oo.fresh_head(),
                           par=torch.nn.Parameter(torch.from_numpy(p.copy()))))
    opt = torch.optim.Adam([g['par'] for g in groups], lr=oo.LR, betas=oo.BETAS, eps=oo.EPS)
    worst = 0.0
    for t in range(1, 51):
        for g in groups:
            grad = oo.gradients(rng, g['p'].size)
            g['par'].grad = torch.from_numpy(g['scale'] * grad)
            o = oo.step64(g['p'], grad, g['m'], g['v'], g['head'], scale=g['scale'])
            g['scale_p'] = o['scale']['p']
            g['p'], g['m'], g['v'], g['head'] = o['p'], o['m'], o['v'], o['head']
        opt.step()
        for g in groups:
            st = opt.state[g['par']]
            for got, ref, scale in ((g['par'].detach().numpy(), g['p'], g['scale_p']),
                                    (st['exp_avg'].numpy(), g['m'], np.abs(g['m'])), (st['exp_avg_sq'].numpy(), g['v'], g['v'])):
                err = np.abs(got - ref)
                assert (err <= 1e-12 * scale + 1e-14).all(), (t, (err / (scale + 1e-300)).max())
                worst = max(worst, float((err / (1e-12 * scale + 1e-14)).max()))
            assert int(st['step']) == g['head'][0] == t
    print('worst |error| / (1e-12 scale + 1e-14) over 50 steps: %.3g' % worst)
    assert groups[0]['head'][1] == np.cumprod(np.full(50, 0.9))[-1] and groups[0]['head'][2] == np.cumprod(np.full(50, 0.999))[-1]


@pytest.mark.parametrize('shape', oo.SHAPES, ids=str)
def test_the_float32_restatement_is_inside_the_bound_on_every_gpu_input(shape):
    for t in oo.STEPS:
        c = oo.case(shape, t, np.float32)
        got = oo.step32(c['p'], c['grad'], c['m'], c['v'], c['head'], scale=c['scale'], n_std=c['n_std'])
        assert got['head'] == c['want']['head'] and got['head'][0] == t
        oo.inside(np.float32, got, c, (shape, t))
        # the bound is no licence: it stays a rounding-sized share of what the step handles (for p: of |p| and of the step
        # that |g| + |m| would make, which is what the cancellation in g - m is charged to)
        b, w = c['bound'], c['want']
        moved = np.abs(w['p']) + w['step_size'] * (np.abs(w['g']) + np.abs(c['m'].astype(np.float64)) + np.abs(w['m'])) / w['den']
        assert (b['p'] <= 64 * oo.U * moved + 1e-40).all()
        assert (b['m'] <= 8 * oo.U * c['want']['scale']['m'] + 1e-40).all() and (b['v'] <= 16 * oo.U * c['want']['v'] + 1e-40).all()


def test_a_zero_gradient_from_a_fresh_state_moves_nothing():
    p = np.random.default_rng(0).normal(0, 1, 100)
    z = np.zeros(100)
    for step in (oo.step64, oo.step32):
        o = step(p.astype(np.float32), z, z, z, oo.fresh_head())
        assert np.array_equal(o['p'], p.astype(np.float32)) and not o['m'].any() and not o['v'].any()
    assert oo.head_at(1) == oo.fresh_head() and oo.head_at(3) == (2, 0.9 * 0.9, 0.999 * 0.999)
