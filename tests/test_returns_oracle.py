"""CPU tests of tests/returns_oracle.py, the float64 restatement libatacom_returns.so is held to: its two forms agree, it equals
the loop the PPO example ran before the library existed, compute_J equals a hand-computed dataset, the v_next rule of
gae_from_compact reproduces V(next_obs) of CompactRecordLayout.unpack, a float32 run of the recurrence stays inside the error
bound, and four wrong implementations posing as the device do not."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import returns_oracle as ro                                  # noqa: E402
from returns_cases import GAMMA_LAM, PATTERNS, make_case, ragged_sizes      # noqa: E402

F32 = 2.0 ** -24


@pytest.mark.parametrize('pattern', PATTERNS[:5])
@pytest.mark.parametrize('gl', GAMMA_LAM)
def test_the_two_restatements_agree(pattern, gl):
    c = make_case(33, 9, pattern, seed=1)
    two = {k: x[0] for k, x in c.items()}
    ret_l, adv_l = ro.gae_loops(gamma=gl[0], lam=gl[1], **two)
    ret_v, adv_v = ro.gae(gamma=gl[0], lam=gl[1], **two)
    assert np.abs(adv_l - adv_v).max() <= 1e-12 * max(1.0, np.abs(adv_v).max())
    assert np.abs(ret_l - ret_v).max() <= 1e-12 * max(1.0, np.abs(ret_v).max())
    js_l = ro.episodes_loops(two['reward'], two['last'], gl[0])
    js_v, _ = ro.episodes_in_dtype(two['reward'], two['last'], gl[0])
    assert len(js_l) == len(js_v)
    assert np.abs(np.array(js_l) - np.array(js_v)).max() <= 1e-12 * max(1.0, np.abs(js_v).max())


def test_the_recurrence_is_mushroom_rls_compute_gae_where_absorbing_implies_last():
    c = {k: x[0] for k, x in make_case(40, 7, 'consecutive_ends', seed=2).items()}
    assert not (c['absorbing'] & ~c['last']).any()
    flat = {k: ro.flatten(x) for k, x in c.items()}
    flat['last'] = ro.flat_last(c['last'])
    ret_m, adv_m = ro.gae_mushroom_flat(flat['reward'], flat['absorbing'], flat['last'], flat['v'], flat['v_next'], 0.99, 0.95)
    ret, adv = ro.gae(gamma=0.99, lam=0.95, **c)
    assert np.abs(ro.flatten(adv) - adv_m).max() <= 1e-12 * np.abs(adv_m).max()
    assert np.abs(ro.flatten(ret) - ret_m).max() <= 1e-12 * np.abs(ret_m).max()


def test_the_oracle_is_the_loop_the_ppo_example_ran():
    """examples/ppo_air_hockey.py before it called compute_gae, in float64: the loop this library replaces."""
    torch = pytest.importorskip('torch')
    c = {k: x[0] for k, x in make_case(25, 11, 'consecutive_ends', seed=3).items()}
    rew, v, nv = (torch.from_numpy(c[k]) for k in ('reward', 'v', 'v_next'))
    ab, last = torch.from_numpy(c['absorbing']), torch.from_numpy(c['last'])
    T, B = rew.shape
    gamma, lam = 0.99, 0.95
    nv = torch.where(ab, torch.zeros_like(nv), nv)
    adv = torch.zeros_like(rew)
    g = torch.zeros(B, dtype=torch.float64)
    for t in reversed(range(T)):
        delta = rew[t] + gamma * nv[t] - v[t]
        g = delta + gamma * lam * torch.where(last[t], torch.zeros_like(g), g)
        adv[t] = g
    ret = adv + v
    norm = (adv - adv.mean()) / (adv.std() + 1e-8)           # torch's std is the sample form: the example's, not PPO's
    ret_o, adv_o = ro.gae(gamma=gamma, lam=lam, **c)
    assert np.abs(adv.numpy() - adv_o).max() <= 1e-12 * np.abs(adv_o).max()
    assert np.abs(ret.numpy() - ret_o).max() <= 1e-12 * np.abs(ret_o).max()
    norm_o, stats = ro.normalize(adv_o[None])
    n = stats[0]
    assert stats[2] == pytest.approx(float(adv.std()) * np.sqrt((n - 1) / n), rel=1e-12)      # population against sample
    assert np.abs(norm.numpy() * np.sqrt(n / (n - 1)) - norm_o[0]).max() <= 1e-9


def test_compute_j_on_a_hand_computed_dataset():
    """One environment, three episodes, the last one unfinished; gamma = 0.5."""
    r = np.array([[1.0], [2.0], [4.0], [3.0], [8.0], [16.0], [5.0]])
    last = np.array([[0], [0], [1], [0], [1], [0], [0]], dtype=bool)
    want = [1 + 0.5 * 2 + 0.25 * 4, 3 + 0.5 * 8, 16 + 0.5 * 5]
    assert ro.episodes_loops(r, last, 0.5) == want
    assert ro.episodes_in_dtype(r, last, 0.5)[0] == want
    assert ro.episodes_in_dtype(r, last, 0.5, np.float32)[0] == want
    assert ro.episodes_loops(r, last, 1.0) == [7.0, 11.0, 21.0]
    sums, js = ro.episode_sums(r[None], last[None], 0.5)
    assert list(sums) == [sum(want), 3.0, sum(j * j for j in want)] and list(js) == want
    # two environments, the second one padding
    r2, l2 = np.concatenate([r, 100 + r], 1)[None], np.concatenate([last, last], 1)[None]
    assert list(ro.episode_sums(r2, l2, 0.5, sizes=[1])[0]) == list(sums)
    # an episode already running at t = 0 starts with exponent 0: the first emitted j does not know how old the episode is
    assert ro.episodes_loops(r[1:], last[1:], 0.5)[0] == 2 + 0.5 * 4


def test_the_v_next_rule_of_gae_from_compact_is_the_critic_on_unpacked_next_obs():
    """Synthetic compact records with shuffled, duplicated and superfluous exception rows, ragged blocks, and an elementwise
    'critic': compact_v_next(critic(obs incl. tail), critic(terminal obs)) == critic(unpack(...)['next_obs'])."""
    torch = pytest.importorskip('torch')
    from rl_on_manifold_amd.returns import compact_v_next
    from rl_on_manifold_amd.rollout import CompactRecordLayout
    W, T, Bm, D, k = 3, 9, 5, 4, 2
    lay = CompactRecordLayout([5, 4, 4], D, k, T)
    g = torch.Generator().manual_seed(4)
    rec = torch.randn((W, T + 1, Bm, lay.Fc), generator=g, dtype=torch.float64)
    last = torch.rand((W, T, Bm), generator=g) < 0.3
    rec[:, :T, :, lay.compact_fields['last']] = last.double()
    rec[:, :T, :, lay.compact_fields['absorbing']] = (last & (torch.rand((W, T, Bm), generator=g) < 0.5)).double()
    critic = lambda obs: 0.5 * obs[..., 0] + obs[..., 1] * obs[..., 2]          # noqa: E731
    blocks, counts = [], []
    for w in range(W):
        tb = torch.nonzero(last[w, :T - 1])                    # the necessary rows: ends before the last step
        extra = torch.nonzero(last[w, T - 1:]) + torch.tensor([T - 1, 0])      # superfluous: an end at the last step ...
        rows = torch.cat([tb, tb[:2], extra])                  # ... and duplicates
        rows = rows[torch.randperm(rows.shape[0], generator=g)]
        term = torch.randn((T, Bm, D), generator=g, dtype=torch.float64)        # the terminal observation of every (t, b)
        e = torch.cat([rows.double(), term[rows[:, 0], rows[:, 1]]], 1)
        if extra.shape[0]:                                      # a superfluous row must say what the records say
            tail = (rows[:, 0] == T - 1)
            e[tail, 2:] = rec[w, T, rows[tail, 1]][:, lay.compact_fields['obs']]
        blocks.append(e)
        counts.append(e.shape[0])
    M = max(counts) + 2
    ends = torch.full((W, M, lay.E), float('nan'), dtype=torch.float64)        # rows past the count are never read
    for w, e in enumerate(blocks):
        ends[w, :e.shape[0]] = e
    want = critic(lay.unpack(rec, ends, counts)['next_obs'])
    v = critic(rec[..., lay.compact_fields['obs']])
    v_ends = critic(ends[..., 2:])
    got = compact_v_next(lay, rec, ends, counts, v, v_ends)
    assert torch.equal(got, want)
    assert torch.equal(compact_v_next(lay, rec[1], ends[1], counts[1], v[1], v_ends[1]), want[1])      # one rank
    assert torch.equal(compact_v_next(lay, rec, None, None, v, None), v[:, 1:])
    bad = ends.clone()
    bad[0, 0, 0] = T
    with pytest.raises(ValueError, match='outside'):
        compact_v_next(lay, rec, bad, counts, v, v_ends)


@pytest.mark.parametrize('T,B', [(1, 5), (7, 65), (120, 512)])
@pytest.mark.parametrize('gl', [(0.99, 0.95), (1.0, 1.0), (0.99, 0.0)])
def test_a_float32_run_stays_inside_the_bound(T, B, gl):
    c = {k: x[0].astype(np.float32) for k, x in make_case(T, B, 'consecutive_ends', seed=5).items()}
    ret32, adv32 = ro.gae_in_dtype(gamma=gl[0], lam=gl[1], dtype=np.float32, **c)
    ret64, adv64 = ro.gae(gamma=gl[0], lam=gl[1], **c)          # the reference receives the inputs rounded to float32
    b_ret, b_adv = ro.gae_bound(gamma=gl[0], lam=gl[1], eps=F32, **c)
    ratio_adv = np.abs(adv32 - adv64) / b_adv
    ratio_ret = np.abs(ret32 - ret64) / b_ret
    print('T %d B %d gamma %.2f lam %.2f: worst |error| / bound: adv %.3f ret %.3f' % (T, B, gl[0], gl[1], ratio_adv.max(), ratio_ret.max()))
    assert ratio_adv.max() <= 0.6 and ratio_ret.max() <= 0.6


def _share_outside(got, want, bound):
    return float((np.abs(got - want) > bound).mean())


def test_negative_controls_leave_the_bound():
    """Wrong recurrences run in float32, posing as the device: each must exceed the bound on at least 5 % of the samples.  lam > 0
    and a 10 % `last` rate: with lam = 0 ignoring `last` is invisible, as it should be."""
    gamma, lam = 0.99, 0.95
    c = {k: x[0].astype(np.float32) for k, x in make_case(40, 65, 'absorbing_with_and_without_last', seed=6, last_rate=0.1).items()}
    _, want = ro.gae(gamma=gamma, lam=lam, **c)
    _, bound = ro.gae_bound(gamma=gamma, lam=lam, eps=F32, **c)
    run = lambda **kw: ro.gae_in_dtype(gamma=gamma, lam=lam, dtype=np.float32, **dict(c, **kw))[1]      # noqa: E731
    assert _share_outside(run(), want, bound) == 0.0
    shares = {'ignores last': _share_outside(run(last=np.zeros_like(c['last'])), want, bound),
              'ignores absorbing': _share_outside(run(absorbing=np.zeros_like(c['absorbing'])), want, bound)}
    # the value of the reset observation at an episode end: v_next = v[t + 1] where the truth is the terminal observation's value
    reset_value = np.concatenate([c['v'][1:], c['v_next'][-1:]], 0)
    shares['reset observation at an end'] = _share_outside(run(v_next=np.where(c['last'], reset_value, c['v_next'])), want, bound)
    # statistics over the padding rows too
    W, Bm = 3, 65
    c3 = {k: x.astype(np.float32) for k, x in make_case(40, Bm, 'consecutive_ends', seed=7, W=W).items()}
    sizes = ragged_sizes(W, Bm - 20)
    pad = ~ro.valid_rows(c3['reward'].shape, sizes)
    for k in c3:
        c3[k] = np.where(pad, np.zeros_like(c3[k]), c3[k])      # padding rows of a gathered buffer are zero
    _, adv = ro.gae(gamma=gamma, lam=lam, **c3)
    _, b3 = ro.gae_bound(gamma=gamma, lam=lam, eps=F32, **c3)
    norm, stats = ro.normalize(adv, sizes)
    wrong, _ = ro.normalize(adv, None)
    tol = b3 / (stats[2] + 1e-8) + 4 * F32 * np.abs(norm)
    real = ~pad
    shares['normalises over the padding'] = _share_outside(wrong[real], norm[real], tol[real])
    print(shares)
    for name, share in shares.items():
        assert share >= 0.05, (name, share)
