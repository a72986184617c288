"""CPU checks of tests/offpolicy_oracle.py, the float64 restatement that tests/test_gpu_offpolicy.py holds libatacom_offpolicy.so
to: it equals modules composed from torch.nn.Linear and the MushroomRL target expression written out in torch (float64, 1e-12);
torch's own float32 evaluation lies inside the float32 bound on every sample of every case; the soft-update restatement is
bit-equal to numpy's  tau * w + (1 - tau) * t;  and the shared target cases exercise every regime of the noise clamp, the action
clamp, the minimum and the absorbing flag."""
import numpy as np
import pytest
import torch

import offpolicy_oracle as oo


class _Critic(torch.nn.Module):
    """The two critic classes of the reference, composed from their attribute names: the action enters layer 2 through a
    bias-free Linear and is divided by _action_scaling; TD3's first layer also sees it."""

    def __init__(self, c, dtype):
        super().__init__()
        t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64)).to(dtype)      # noqa: E731
        k = c['W2a'].shape[1]
        self._h1 = torch.nn.Linear(c['W1'].shape[1], 64)
        self._h2_s = torch.nn.Linear(64, 64)
        self._h2_a = torch.nn.Linear(k, 64, bias=False)
        self._h3 = torch.nn.Linear(64, 1)
        self.to(dtype)
        with torch.no_grad():
            for lin, W, b in ((self._h1, 'W1', 'b1'), (self._h2_s, 'W2', 'b2'), (self._h3, 'W3', 'b3')):
                lin.weight.copy_(t(c[W]))
                lin.bias.copy_(t(c[b]))
            self._h2_a.weight.copy_(t(c['W2a']))
        self._action_scaling = t(np.ones(k) if c['act_scale'] is None else c['act_scale'])
        self.kind, self.act = c['kind'], (torch.relu if c['activation'] == 'relu' else torch.tanh)
        self.shift = None if c['obs_shift'] is None else t(c['obs_shift'])
        self.scale = None if c['obs_scale'] is None else t(c['obs_scale'])

    def forward(self, state, action):
        if self.shift is not None:
            state = (state - self.shift) * self.scale
        action = action / self._action_scaling
        x1 = torch.cat((state, action), 1) if self.kind == oo.TD3 else state
        h1 = self.act(self._h1(x1))
        h2 = self.act(self._h2_s(h1) + self._h2_a(action))
        return torch.squeeze(self._h3(h2), 1)


def _actor(a, x, mean_mode, dtype):
    t = lambda v: torch.tensor(np.asarray(v, dtype=np.float64)).to(dtype)          # noqa: E731
    act = torch.relu if a['activation'] == 'relu' else torch.tanh
    if a['obs_shift'] is not None:
        x = (x - t(a['obs_shift'])) * t(a['obs_scale'])
    lin = torch.nn.functional.linear
    m = lin(act(lin(act(lin(x, t(a['W1']), t(a['b1']))), t(a['W2']), t(a['b2']))), t(a['W3']), t(a['b3']))
    return t(a['act_scale']) * torch.tanh(m) if mean_mode else m


def _torch_target(c, dtype):
    """MushroomRL's TD3._next_q / DDPG._next_q and  reward + gamma * q_next  in torch at `dtype` -> (y, a'', [q_j])."""
    t = lambda v: torch.tensor(np.asarray(v, dtype=np.float64)).to(dtype)          # noqa: E731
    with torch.no_grad():
        x = t(c['next_obs'])
        a = _actor(c['actor'], x, c['mean_mode'], dtype)
        if c['eps'] is not None:
            std, clip = torch.tensor(c['noise_std'], dtype=dtype), torch.tensor(c['noise_clip'], dtype=dtype)
            a = a + torch.clamp(std * t(c['eps']), -clip, clip)
        if c['low'] is not None:
            a = torch.minimum(torch.maximum(a, t(c['low'])), t(c['high']))
        qs = [_Critic(cr, dtype)(x, a) for cr in c['critics']]
        q = qs[0] if len(qs) == 1 else torch.minimum(qs[0], qs[1])
        q = q * (1.0 - t(c['absorbing']))
        y = t(c['reward']) + torch.tensor(c['gamma'], dtype=dtype) * q
    return y.numpy().astype(np.float64), a.numpy().astype(np.float64), [v.numpy().astype(np.float64) for v in qs]


def _cases():
    out = []
    for i, shape in enumerate(oo.SHAPE_CASES):
        out.append(('shape%d' % i, dict(zip(oo.SHAPE_KEYS, shape)), dict(rows=65, seed=oo.SHAPE_SEEDS[i])))
    for name, nc, eps, bounds, mm in oo.MODE_CASES:
        out.append((name, dict(zip(oo.SHAPE_KEYS, oo.ROW_SHAPE)),
                    dict(rows=200, seed=7, n_critics=nc, with_eps=eps, with_bounds=bounds, mean_mode=mm)))
    return out


@pytest.mark.parametrize('name,shape,kw', _cases(), ids=[c[0] for c in _cases()])
def test_the_restatement_is_the_torch_modules_and_float32_torch_is_inside_the_bound(name, shape, kw):
    c64 = oo.case(dtype=np.float64, **shape, **kw)
    ref = oo.case_target(c64)
    y, a, qs = _torch_target(c64, torch.float64)
    assert np.abs(ref['y'] - y).max() <= 1e-12 and np.abs(ref['a'] - a).max() <= 1e-12
    for j, q in enumerate(qs):
        assert np.abs(ref['q'][:, j] - q).max() <= 1e-12
    # the Q-value of the recorded actions, the other entry point
    for cr in c64['critics']:
        q, _, _ = oo.critic_q(cr, c64['next_obs'], c64['action'])
        with torch.no_grad():
            qt = _Critic(cr, torch.float64)(torch.tensor(c64['next_obs']), torch.tensor(c64['action'])).numpy()
        assert np.abs(q - qt).max() <= 1e-12
    # float32: every sample inside the bound, none left out
    c32 = oo.case(dtype=np.float32, **shape, **kw)
    ref = oo.case_target(c32)
    y, a, _ = _torch_target(c32, torch.float32)
    assert (np.abs(y - ref['y']) <= ref['e_y']).all(), (np.abs(y - ref['y']) / ref['e_y']).max()
    assert (np.abs(a - ref['a']) <= ref['e_a']).all(), (np.abs(a - ref['a']) / ref['e_a']).max()
    assert np.isfinite(ref['e_y']).all()
    # the critic half from torch's own a'': the sharper bound, which does not carry the actor's error through the critics' norms
    y2, e2 = oo.target_from_action(c32['critics'], c32['next_obs'], a, c32['reward'], c32['absorbing'], c32['gamma'])
    assert (np.abs(y - y2) <= e2).all() and e2.max() < 5e-3, e2.max()
    for cr in c32['critics']:
        q, e, _ = oo.critic_q(cr, c32['next_obs'], c32['action'])
        with torch.no_grad():
            qt = _Critic(cr, torch.float32)(torch.tensor(c32['next_obs']), torch.tensor(c32['action'])).numpy()
        assert (np.abs(qt - q) <= e).all()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_the_full_td3_cases_exercise_every_regime(dtype):
    shape = dict(zip(oo.SHAPE_KEYS, oo.ROW_SHAPE))
    for rows, _ in oo.ROW_CASES:
        if rows >= 200:
            oo.assert_regimes(oo.case(seed=7, rows=rows, dtype=dtype, **shape))
    for i, s in enumerate(oo.SHAPE_CASES):
        oo.assert_regimes(oo.case(seed=oo.SHAPE_SEEDS[i], rows=65, dtype=dtype, **dict(zip(oo.SHAPE_KEYS, s))))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('tau', [1e-3, 0.005, 0.5, 0.0, 1.0])
def test_the_soft_update_restatement_is_numpy_in_the_arrays_precision(dtype, tau):
    rng = np.random.default_rng(3)
    t, w = rng.normal(0, 1, 5000).astype(dtype), rng.normal(0, 1, 5000).astype(dtype)
    got = oo.soft_update(t, w, tau)
    want = tau * w + (1 - tau) * t
    assert got.dtype == want.dtype == dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    if tau == 0.0:
        assert np.array_equal(got, t)
    if tau == 1.0:
        assert np.array_equal(got, w)
