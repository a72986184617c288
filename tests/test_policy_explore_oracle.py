"""CPU checks of the TD3 / DDPG exploration policies: the float64 restatement (tests/policy_explore_oracle.py) against the
reference's own actor networks (tests/golden/policy_td3_ddpg.npz), a property of its Ornstein-Uhlenbeck process, the new
atacom_mlp fields of include/atacom_hip.h against the ctypes mirror, and the host-side construction of the policies."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from policy_explore_oracle import ExplorePolicy, ou_stationary_variance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FIELDS = ('mean_mode', 'explore', 'act_scale', 'act_low', 'act_high', 'ou_theta', 'ou_dt', 'ou_x0', 'ou_state')


def _weights(g, env):
    return [g['%s._h%d.%s' % (env, i, w)] for i in (1, 2, 3) for w in ('weight', 'bias')]


@pytest.mark.parametrize('sc', ['unit', 'vec'])
@pytest.mark.parametrize('env', ['iiwa', 'planar'])
@pytest.mark.parametrize('algo', ['td3', 'ddpg'])
def test_restatement_reproduces_the_reference_actor_networks(golden, algo, env, sc):
    g = golden('policy_td3_ddpg')
    pol = ExplorePolicy(*_weights(g, env), act_scale=g['%s_%s.action_scaling' % (env, sc)], kind=algo)
    y = g['%s_%s_%s.y' % (algo, env, sc)]
    mine = pol.mean(g[env + '.x'].astype(np.float64))
    assert np.abs(mine - y).max() < 2e-5                    # the reference computes in float32
    assert np.abs(np.tanh(pol.network(g[env + '.x']))).max() > 0.5      # the squash is really exercised


def test_td3_draw_is_the_clipped_gaussian():
    rng = np.random.default_rng(0)
    W = [rng.normal(0, 0.5, s) for s in ((64, 6), (64,), (64, 64), (64,), (3, 64), (3,))]
    pol = ExplorePolicy(*W, act_scale=[1.0, 0.5, 2.0], kind='td3', std=0.5, low=[-1, -0.2, -1], high=[1, 0.3, 0.5])
    obs, eps = rng.normal(0, 1, (200, 6)), rng.normal(0, 1, (200, 3))
    a = pol.draw(obs, eps, np.zeros(200))
    assert np.array_equal(a, np.clip(pol.mean(obs) + 0.5 * eps, pol.low, pol.high))
    assert (a == pol.low).any() and (a == pol.high).any()


def test_ou_restarts_at_x0_and_has_the_stationary_variance():
    k, B = 3, 4000
    W = [np.zeros(s) for s in ((64, 4), (64,), (64, 64), (64,), (k, 64), (k,))]   # mean 0: the action is x itself
    sigma, theta, dt = np.array([0.2, 0.5, 1.0]), 0.15, 0.5
    pol = ExplorePolicy(*W, kind='ddpg', std=sigma, theta=theta, dt=dt, x0=[0.3, -0.2, 0.1])
    rng = np.random.default_rng(1)
    obs = np.zeros((B, 4))
    t = np.arange(B) % 7
    a = pol.draw(obs, np.zeros((B, k)), t)
    # an episode start restarts at x0, then one noise-free decay step
    assert np.allclose(a[t == 0], pol.x0 * (1 - theta * dt))
    # stationary variance: iterate long past the decay time 1 / (theta dt) ~ 13 steps
    pol.x = np.zeros((B, k))
    for _ in range(300):
        a = pol.draw(obs, rng.standard_normal((B, k)), np.ones(B))
    var = a.var(0)
    want = ou_stationary_variance(sigma, theta, dt)
    # sampling error of a variance estimate: sd = var sqrt(2 / B) ~ 2.2 % at B = 4000; 5 sd
    assert np.all(np.abs(var / want - 1) < 5 * np.sqrt(2.0 / B)), (var, want)


@pytest.mark.skipif(shutil.which('gcc') is None, reason='needs a C compiler')
def test_header_offsets_of_the_new_atacom_mlp_fields_match_ctypes(tmp_path):
    from rl_on_manifold_amd import _lib
    src = tmp_path / 'mlp.c'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "atacom_hip.h"', 'int main(void) {',
             '    printf("sizeof %zu\\n", sizeof(atacom_mlp));', '    printf("v1 %d\\n", (int)ATACOM_MLP_SIZE_V1);']
    lines += ['    printf("%s %%zu %%zu\\n", offsetof(atacom_mlp, %s), sizeof(((atacom_mlp*)0)->%s));' % (f, f, f)
              for f in ('reserved1',) + NEW_FIELDS]
    lines += ['    return 0;', '}']
    src.write_text('\n'.join(lines) + '\n')
    exe = tmp_path / 'mlp'
    subprocess.check_call(['gcc', '-std=c11', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        name, *vals = ln.split()
        got[name] = tuple(int(v) for v in vals)
    M = _lib.AtacomMlp
    assert got['sizeof'] == (ctypes.sizeof(M),)
    assert got['v1'] == (_lib.MLP_SIZE_V1,) == (M.reserved1.offset + 4,)
    for f in ('reserved1',) + NEW_FIELDS:
        assert got[f] == (getattr(M, f).offset, getattr(M, f).size), f
    assert [f[0] for f in M._fields_][-len(NEW_FIELDS):] == list(NEW_FIELDS)      # appended, nothing moved


class _Actor:
    """Stand-in with the attribute names of the reference's TD3ActorNetwork / DDPGActorNetwork."""

    def __init__(self, n_in=12, k=3, scaling=(1.0, 0.5, 2.0)):
        import torch
        self._h1, self._h2, self._h3 = torch.nn.Linear(n_in, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, k)
        self._action_scaling = torch.tensor(scaling, dtype=torch.float64)


def test_from_td3_reads_the_covariance_and_the_action_scaling():
    from rl_on_manifold_amd import MlpPolicy, _lib
    pol = MlpPolicy.from_td3(_Actor(), 0.25, low=-1.0, high=[1.0, 0.5, 1.0])
    assert pol.explore == _lib.EXPLORE_CLIPPED and pol.mean_mode == 1
    assert np.allclose(pol.tensors['std'].numpy(), 0.5)                  # sqrt of the diagonal of eye(k) * 0.25
    assert np.allclose(pol.tensors['act_scale'].numpy(), [1.0, 0.5, 2.0])
    assert np.allclose(pol.tensors['act_high'].numpy(), [1.0, 0.5, 1.0])
    pol = MlpPolicy.from_td3(_Actor(), np.diag([0.04, 0.09, 0.16]))
    assert np.allclose(pol.tensors['std'].numpy(), [0.2, 0.3, 0.4])
    cov = np.eye(3) * 0.25
    cov[0, 1] = cov[1, 0] = 0.01
    with pytest.raises(ValueError):
        MlpPolicy.from_td3(_Actor(), cov)
    with pytest.raises(ValueError):
        MlpPolicy.from_td3(_Actor(), np.eye(2))


def test_from_ddpg_broadcasts_sigma_and_owns_no_state_before_an_env():
    from rl_on_manifold_amd import MlpPolicy, _lib
    pol = MlpPolicy.from_ddpg(_Actor(), np.ones(1) * 0.2, theta=0.15, dt=1e-2)
    assert pol.explore == _lib.EXPLORE_OU and pol.mean_mode == 1
    assert np.allclose(pol.tensors['std'].numpy(), [0.2, 0.2, 0.2])
    assert pol.noise_state is None
    pol.reset_noise()                                     # nothing to reset yet
    with pytest.raises(ValueError):
        MlpPolicy.from_ddpg(_Actor(), 0.2, theta=0.15, dt=0.0)


def test_plain_constructors_keep_the_gaussian_mode():
    from rl_on_manifold_amd import MlpPolicy
    pol = MlpPolicy.from_module(_Actor())
    assert pol.explore == 0 and pol.mean_mode == 0 and 'act_scale' not in pol.tensors
