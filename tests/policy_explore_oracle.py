"""Float64 restatement of the TD3 / DDPG exploration policies of the fused policy rollout (row N2; test infrastructure only).

Networks: TD3ActorNetwork / DDPGActorNetwork of the reference (examples/network.py:112-147, :197-232) -- Linear(n_in, h) ->
ReLU -> Linear(h, h) -> ReLU -> Linear(h, n_out), then  mean = action_scaling * tanh(.).  Pinned by
tests/golden/policy_td3_ddpg.npz (written from the reference's own modules by profiles/tools/gen_policy_td3_ddpg.py).

Exploration, as the reference's experiment scripts build it (examples/iiwa_air_hockey_exp.py:213-217,256-263):

* TD3 -- MushroomRL 1.x `mushroom_rl.policy.ClippedGaussianPolicy.draw_action`:
      np.clip(np.random.multivariate_normal(mu(s), sigma), low, high)
  with sigma the covariance (the reference passes np.eye(k) * 0.25).  For a diagonal sigma that is
  clip(mu + sqrt(diag(sigma)) * eps, low, high), eps standard normal.
* DDPG -- MushroomRL 1.x `mushroom_rl.policy.OrnsteinUhlenbeckPolicy`:
      draw_action: x = x_prev - theta * x_prev * dt + sigma * sqrt(dt) * N(0, 1);  x_prev = x;  return mu(s) + x
      reset:       x_prev = x0 if x0 is not None else zeros
  and mushroom_rl.core.Core calls policy.reset() at every episode start.  Here the state is per environment, and an episode
  starts wherever the environment's step counter t is 0 (an explicit, masked or automatic reset).

UNPINNED: MushroomRL is not available to this project's tests, so the two noise processes above are restated from its 1.x
source, not checked against it (the status DESIGN.md section 2 gives Bullet and Pinocchio).  Only the networks are pinned.
"""
import numpy as np


class ExplorePolicy:
    """mean = act_scale * tanh(MLP((obs - shift) * scale)); explore 'td3' (clipped Gaussian) or 'ddpg' (OU)."""

    def __init__(self, W1, b1, W2, b2, W3, b3, act_scale=1.0, obs_shift=None, obs_scale=None, kind='td3', std=0.5,
                 low=-1.0, high=1.0, theta=0.15, dt=1e-2, x0=None):
        self.W1, self.b1, self.W2, self.b2, self.W3, self.b3 = (np.asarray(a, dtype=np.float64)
                                                                for a in (W1, b1, W2, b2, W3, b3))
        n_in, k = self.W1.shape[1], self.W3.shape[0]
        self.k = k
        self.shift = np.zeros(n_in) if obs_shift is None else np.asarray(obs_shift, dtype=np.float64)
        self.scale = np.ones(n_in) if obs_scale is None else np.asarray(obs_scale, dtype=np.float64)
        self.act_scale = np.broadcast_to(np.asarray(act_scale, dtype=np.float64), (k,)).copy()
        self.kind = kind
        self.std = np.broadcast_to(np.asarray(std, dtype=np.float64), (k,)).copy()
        self.low = np.broadcast_to(np.asarray(low, dtype=np.float64), (k,)).copy()
        self.high = np.broadcast_to(np.asarray(high, dtype=np.float64), (k,)).copy()
        self.theta, self.dt = float(theta), float(dt)
        self.x0 = np.zeros(k) if x0 is None else np.broadcast_to(np.asarray(x0, dtype=np.float64), (k,)).copy()
        self.x = None                                       # [B, k] OU state

    def network(self, obs):
        x = (np.asarray(obs, dtype=np.float64) - self.shift) * self.scale
        h1 = np.maximum(x @ self.W1.T + self.b1, 0.0)
        h2 = np.maximum(h1 @ self.W2.T + self.b2, 0.0)
        return h2 @ self.W3.T + self.b3

    def mean(self, obs):
        return self.act_scale * np.tanh(self.network(obs))

    def draw(self, obs, eps, t):
        """One draw for a batch: obs [B, n_in], eps [B, k] standard normals, t [B] episode step counters."""
        mu = self.mean(obs)
        if self.kind == 'td3':
            return np.clip(mu + self.std * eps, self.low, self.high)
        if self.x is None:
            self.x = np.zeros_like(mu)
        start = np.asarray(t) == 0
        self.x[start] = self.x0                             # policy.reset() at the episode start
        self.x = self.x - self.theta * self.x * self.dt + self.std * np.sqrt(self.dt) * eps
        return mu + self.x


def ou_stationary_variance(sigma, theta, dt):
    """Var of x_{n+1} = (1 - theta dt) x_n + sigma sqrt(dt) eps in its stationary state."""
    a = 1.0 - theta * dt
    return sigma ** 2 * dt / (1.0 - a * a)


def rollout(env, policy, n_steps, noise, auto_reset=True):
    """T steps of an oracle.atacom_batched.BatchedAtacomEnv driven by an ExplorePolicy, time-major outputs like
    atacom_rollout_mlp (the action recorded is the one handed to the env, before its own clip to [-1, 1])."""
    out = {k: [] for k in ('obs', 'action', 'reward', 'next_obs', 'absorbing', 'last')}
    for t in range(n_steps):
        o = env.observation()
        a = policy.draw(o, noise[t], env.t.copy())
        no, r, ab, _ = env.step(a)
        last = ab | (env.t >= env.spec.horizon)
        for k, v in zip(out, (o, a, r, no, ab, last)):
            out[k].append(np.array(v).copy())
        if auto_reset and last.any():
            env.reset(last)
    return {k: np.stack(v) for k, v in out.items()}
