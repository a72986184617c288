"""CPU-only checks of the oracle of libatacom_offstep.so (tests/offstep_oracle.py): its float64 restatement IS torch.optim.Adam
followed by  tau * p + (1 - tau) * t  (to the project's float64 rule, 1e-12 of each value's scale + 1e-14, the standard of
optim_oracle.inside), a group without a gradient keeps its bits while its target moves, and the ends of tau do what the header
says, in both precisions."""
import numpy as np
import pytest

import offstep_oracle as fo


@pytest.mark.parametrize('shape', fo.SHAPES, ids=str)
def test_the_float64_restatement_is_torch_adam_then_the_target_expression(shape):
    torch = pytest.importorskip('torch')
    c = fo.case(shape, np.float64)
    N = fo.group_size(*shape)
    assert c['p'].shape == (N,) and sum(int(np.prod(s)) for _, s in fo.segments(*shape)) == N
    par = torch.nn.Parameter(torch.from_numpy(c['p'].copy()))
    tgt = torch.from_numpy(c['target'].copy())
    opt = torch.optim.Adam([par], lr=fo.LR, betas=fo.BETAS, eps=fo.EPS)
    p, m, v, head, target = c['p'], np.zeros(N), np.zeros(N), fo.fresh_head(), c['target']
    worst = 0.0
    for t in range(3):
        par.grad = torch.from_numpy(0.5 * c['grads'][t])
        opt.step()
        with torch.no_grad():
            tgt = fo.TAU * par + (1.0 - fo.TAU) * tgt
        o = fo.tracked64(p, c['grads'][t], m, v, head, target, scale=0.5)
        st = opt.state[par]
        for name, got, ref, scale in (('p', par.detach().numpy(), o['p'], o['scale']['p']), ('m', st['exp_avg'].numpy(), o['m'], np.abs(o['m'])),
                                      ('v', st['exp_avg_sq'].numpy(), o['v'], o['v']),
                                      ('target', tgt.numpy(), o['target'], fo.TAU * np.abs(o['p']) + (1.0 - fo.TAU) * np.abs(target))):
            err = np.abs(got - ref)
            assert (err <= 1e-12 * scale + 1e-14).all(), (t, name, (err / (scale + 1e-300)).max())
            worst = max(worst, float((err / (1e-12 * scale + 1e-14)).max()))
        assert int(st['step']) == o['head'][0] == t + 1
        p, m, v, head, target = o['p'], o['m'], o['v'], o['head'], o['target']
    print('%s: worst |error| / (1e-12 scale + 1e-14) over 3 steps: %.3g' % (shape, worst))


@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=('float32', 'float64'))
def test_an_unstepped_group_keeps_its_bits_and_tau_has_two_exact_ends(dtype):
    shape = fo.SHAPES[2]
    c = fo.case(shape, dtype)
    N = fo.group_size(*shape)
    tracked = fo.tracked32 if dtype == np.float32 else fo.tracked64
    m, v = np.full(N, 0.25, dtype), np.full(N, 0.5, dtype)
    head = (7, 0.9 ** 7, 0.999 ** 7)
    o = tracked(c['p'], None, m, v, head, c['target'])
    assert o['head'] == head and all(o[k].dtype == dtype and o[k].tobytes() == a.tobytes() for k, a in (('p', c['p']), ('m', m), ('v', v)))
    assert o['target'].dtype == dtype and (o['target'] != c['target']).any()
    assert o['target'].tobytes() == fo.follow(c['p'], c['target'], fo.TAU, dtype).tobytes()
    # tau = 0: 0 * p + 1 * t = t; tau = 1: 1 * p + 0 * t = p, both bit for bit on finite values that are no negative zeros
    assert tracked(c['p'], None, m, v, head, c['target'], tau=0.0)['target'].tobytes() == c['target'].tobytes()
    assert tracked(c['p'], None, m, v, head, c['target'], tau=1.0)['target'].tobytes() == c['p'].tobytes()
    # a stepped group's target follows the NEW p, and a group without a target has none
    o = tracked(c['p'], c['grads'][0], np.zeros(N, dtype), np.zeros(N, dtype), fo.fresh_head(), c['target'])
    assert o['target'].tobytes() == fo.follow(o['p'], c['target'], fo.TAU, dtype).tobytes() and (o['p'] != c['p']).any()
    assert tracked(c['p'], c['grads'][0], np.zeros(N, dtype), np.zeros(N, dtype), fo.fresh_head())['target'] is None


def test_the_float32_restatement_rounds_each_operation_once():
    """The float32 target update differs from the float64 one rounded at the end: the three roundings are there."""
    c = fo.case(fo.SHAPES[0], np.float32)
    got = fo.follow(c['p'], c['target'], fo.TAU, np.float32)
    exact = fo.TAU * c['p'].astype(np.float64) + (1.0 - fo.TAU) * c['target'].astype(np.float64)
    assert got.dtype == np.float32 and (got != exact.astype(np.float32)).any()
    assert (np.abs(got - exact) <= 4 * 2.0 ** -24 * (fo.TAU * np.abs(c['p']) + np.abs(c['target'])) + 1e-45).all()
