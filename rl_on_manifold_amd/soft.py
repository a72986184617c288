"""A SAC update on the device -- the host side of libatacom_soft.so (include/atacom_soft_hip.h states the arithmetic): the fused
soft TD target, the gradients of the two critics' mean-squared TD error, the gradients of the squashed-Gaussian actor's loss
with respect to its mu and sigma networks, and Adam on the temperature log_alpha, each over a minibatch gathered through row
numbers from a replay memory in place.  They replace, in a learner's inner loop,

    a', logp' = policy.compute_action_and_log_prob_t(next_obs[idx]);  y = r + gamma (1 - absorbing) (min_j Q'_j(s', a') - alpha logp')
    ((critic_j(obs[idx], action[idx]) - y) ** 2).mean().backward()                         # j = 1, 2
    (alpha * logp - min_j critic_j(obs[idx], a)).mean().backward()                         # the actor's step; the critics are only read
    (-(log_alpha * (logp + target_entropy).detach()).mean()).backward();  alpha_optim.step()

The policy is an engine.MlpPolicy of from_sac; a critic is a SoftCritic, the plain 2 x 64 network on [obs | action].  The
gradients are fit.Gradients with the value head's key, which the device Adam of optim.py accepts: one Adam of four groups
(an MlpPolicy over the mu tensors, one over the sigma tensors, SoftCritic.as_policy() of each critic) steps all four networks
in one launch, and offpolicy.soft_update moves the target critics as plain pairs.

Every call is enqueued on the current stream of the tensors' device and nothing synchronises.  With `out=` (and parameters that
already live on the device in the call's dtype) a call allocates nothing and can be captured in a graph.  No numerics here,
and no fall-back: a missing library is an error.
"""
import torch

from . import _lib_fit as _lf
from . import _lib_soft as _ls
from . import _rows
from ._rows import (DTYPES, TARGET_ROWS, bound, check_rows, checked_blocks, checked_idx, fill, inputs, n_rows, needs_gpu, network_struct,
                    no_overlap, one_launch, optional_rows, reuse, rows_of, rows_out, run, sized, stream, target_rows)
from .fit import Gradients


class SoftCritic:
    """Weights of the critic of the reference's SAC agent (examples/network.py: SACCriticNetwork):
    q = W3 act(W2 act(W1 [xn | a] + b1) + b2) + b3 with xn the normalised observation and the action raw; W1 [64, D + k].
    `SoftCritic.from_module(net, obs_dim)` accepts any module with `_h1`, `_h2`, `_h3`."""

    def __init__(self, W1, b1, W2, b2, W3, b3, n_act, obs_shift=None, obs_scale=None, activation='relu'):
        self.tensors = dict(W1=W1, b1=b1, W2=W2, b2=b2, W3=W3, b3=b3, obs_shift=obs_shift, obs_scale=obs_scale)
        self.activation = {'relu': 0, 'tanh': 1}[activation]
        self.n_act = int(n_act)
        self.n_obs = int(torch.as_tensor(W1).shape[1]) - self.n_act
        if self.n_act < 1 or self.n_obs < 1:
            raise ValueError("a SAC critic's first layer takes the observation and the %d action elements, got %d inputs" % (
                self.n_act, self.n_obs + self.n_act))
        self._keep = None

    @classmethod
    def from_module(cls, net, obs_dim, obs_low=None, obs_high=None, activation='relu'):
        k = net._h1.in_features - int(obs_dim)
        shift = scale = None
        if obs_low is not None and obs_high is not None:          # MinMaxPreprocessor, as MlpPolicy.from_module forms it
            lo, hi = torch.as_tensor(obs_low, dtype=torch.float64), torch.as_tensor(obs_high, dtype=torch.float64)
            finite = torch.isfinite(lo) & torch.isfinite(hi)
            shift = torch.where(finite, (hi + lo) / 2, torch.zeros_like(lo))
            scale = torch.where(finite, 2.0 / (hi - lo).clamp_min(1e-12), torch.ones_like(lo))
        g = lambda lin: (lin.weight.detach(), lin.bias.detach())      # noqa: E731
        return cls(*g(net._h1), *g(net._h2), *g(net._h3), n_act=k, obs_shift=shift, obs_scale=scale, activation=activation)

    def as_policy(self):
        """An MlpPolicy over the same six tensors (n_in = D + k, n_out = 1): what a group of optim.Adam and a pair of
        offpolicy.soft_update take."""
        from .engine import MlpPolicy
        t = self.tensors
        return MlpPolicy(t['W1'], t['b1'], t['W2'], t['b2'], t['W3'], t['b3'], activation='tanh' if self.activation else 'relu')

    def as_struct_on(self, device, dtype):
        """The atacom_soft_critic of this network on `device` in `dtype`.  Tensors that are already there are used as they are (no
        copy, so the call can be captured in a graph); the copies live as long as the critic or until the next call."""
        D, k = self.n_obs, self.n_act
        c = network_struct(self, (('W1', (64, D + k)), ('b1', (64,)), ('W2', (64, 64)), ('b2', (64,)), ('W3', (1, 64)), ('b3', (1,)),
                                  ('obs_shift', (D,)), ('obs_scale', (D,))), _ls.Critic, device, dtype)
        c.n_obs, c.n_act, c.activation = D, k, self.activation
        return c


class ActorGradients:
    """What soft_actor_gradient writes: `mu` and `sigma`, the fit.Gradients of the two networks (they share one workspace), and
    `stats` [4] = the loss mean(alpha logp - min q), mean(logp), -(mean(logp) + target_entropy) -- the gradient of the alpha loss
    with respect to log_alpha, what AlphaAdam.step takes -- and the share of rows with a clamped log sigma."""

    def __init__(self, mu, sigma):
        self.mu, self.sigma, self.stats = mu, sigma, mu.stats
        self.key, self.workspace = mu.key, mu.workspace               # what the rule of `out=` reads

    @property
    def loss(self):
        return self.stats[0]

    @property
    def alpha_grad(self):
        return self.stats[2:3]


def _pair(critics):
    critics = tuple(critics) if isinstance(critics, (list, tuple)) else ()
    if len(critics) != 2 or not all(isinstance(c, SoftCritic) for c in critics):
        raise ValueError("critics must be a pair of SoftCritic")
    if (critics[0].n_obs, critics[0].n_act) != (critics[1].n_obs, critics[1].n_act):
        raise ValueError("the two critics differ in observation or action size")
    return critics


def _sizes(c):
    D, k = c.n_obs, c.n_act
    if not 1 <= k <= _ls.MAX_ACT or D < 1 or D + k > _ls.MAX_IN:
        raise ValueError("a critic of %d observation and %d action elements is outside k 1 .. %d, D + k <= %d" % (D, k, _ls.MAX_ACT, _ls.MAX_IN))
    return D, k


def _policy_checks(policy, D, k):
    from .engine import MlpPolicy
    if not isinstance(policy, MlpPolicy):
        raise ValueError("policy must be an MlpPolicy (MlpPolicy.from_sac)")
    if policy.tensors.get('sW1') is None or not policy.squash:
        raise ValueError("policy must carry a sigma network and squash (MlpPolicy.from_sac): SAC samples a squashed Gaussian")
    W1, W3 = policy.tensors['W1'], policy.tensors['W3']
    if (int(W1.shape[1]), int(W3.shape[0])) != (D, k):
        raise ValueError("the policy maps %d to %d where the critics take %d observation and %d action elements" % (
            W1.shape[1], W3.shape[0], D, k))


def _log_alpha(log_alpha, x):
    if not isinstance(log_alpha, torch.Tensor) or log_alpha.numel() != 1 or log_alpha.dtype != x.dtype or log_alpha.device != x.device:
        raise ValueError("log_alpha must be a tensor of one %s value on %s" % (x.dtype, x.device))
    return log_alpha


def _squash_args(a, keep, x, k, M, eps, log_alpha, act_scale, act_shift, ins):
    """eps, log_alpha, act_scale and act_shift of a call into its argument struct; the tensors join `ins` and `keep`."""
    if eps is None:
        raise ValueError("eps must be a tensor of shape (%d, %d): the caller draws the standard normals" % (M, k))
    optional_rows(a, ins, x, M, [('eps', eps, k)])
    a.log_alpha = _log_alpha(log_alpha, x).data_ptr()
    ins.append((log_alpha, 'log_alpha'))
    for name, v in (('act_scale', act_scale), ('act_shift', act_shift)):
        if v is not None:
            t = bound(v, k, x, name)
            keep.append(t)
            setattr(a, name, t.data_ptr())
            ins.append((t, name))


def soft_td_target(policy, critics, next_obs, reward, absorbing, gamma, log_alpha, eps, *, act_scale=None, act_shift=None, idx=None,
                   out=None, action_out=None, logp_out=None, n_blocks=0):
    """SAC's TD target in one launch, for next_obs [..., D], reward [...] and absorbing [...] (0.0 / 1.0 in the dtype; a bool
    tensor is converted) sharing their leading dimensions:

        a', logp' = the squashed Gaussian of `policy` at next_obs with the caller's eps [M, k]
        y = reward + gamma * ((1 - absorbing) * (min_j Q'_j(next_obs, a') - exp(log_alpha) * logp'))

    `critics` is the pair of TARGET SoftCritic, log_alpha a one-value tensor on the device, act_scale / act_shift scalars or [k]
    (MushroomRL's _delta_a and _central_a; None: 1 and 0).  eps row r belongs to row r of the call, not to idx[r].
    -> y [M]; action_out [M, k] and logp_out [M], if given, receive a' and logp'."""
    critics = _pair(critics)
    D, k = _sizes(critics[0])
    _policy_checks(policy, D, k)
    lead = rows_of(next_obs, 'next_obs')
    if float(gamma) != float(gamma) or abs(float(gamma)) == float('inf'):
        raise ValueError("gamma must be finite, got %r" % (gamma,))
    ts, launch, idx, M = target_rows(next_obs, reward, absorbing, lead, D, idx)
    n_blocks = checked_blocks(n_blocks, _ls.MAX_BLOCKS)
    a = _ls.new_args(_ls.TargetArgs)
    keep, ins = [], inputs(ts, TARGET_ROWS, idx)
    _squash_args(a, keep, next_obs, k, M, eps, log_alpha, act_scale, act_shift, ins)
    y, a.y_stride = rows_out(out, 'out', M, 1, next_obs)
    outs = [(y, 'out')]
    optional_rows(a, outs, next_obs, M, [('action_out', action_out, k), ('logp_out', logp_out, 1)])
    no_overlap(outs, ins)
    needs_gpu(next_obs, 'soft')
    fill(a, next_obs, n_blocks, launch, TARGET_ROWS, ts, idx)
    a.n_critics, a.policy = 2, policy.as_struct_on(next_obs.device, next_obs.dtype)
    for j, c in enumerate(critics):
        a.critics[j] = c.as_struct_on(next_obs.device, next_obs.dtype)
    a.gamma, a.y = float(gamma), y.data_ptr()
    run(a, _ls.load().atacom_soft_target, _ls.check, next_obs)
    return y


def _fresh(n, need, key):
    """n fit.Gradients of `key` = (n1, 1, the value head, dtype, device); the first holds the workspace of `need` bytes."""
    return tuple(Gradients(*key, need if j == 0 else 0, key) for j in range(n))


def soft_critic_gradient(critics, obs, action, target, *, idx=None, out=None, n_blocks=0):
    """The gradient of  ((Q_j(obs, action) - target) ** 2).mean()  for the pair of SoftCritic (or one), over the rows of obs
    [..., D] and action [..., k] (strided views with contiguous rows, sharing their leading dimensions: the columns of a replay
    memory, read in place) -- or, with `idx`, over the rows it names.  target [M] belongs to row r of the CALL.
    -> a pair of fit.Gradients (n_in = D + k, n_out = 1, the value head's key; stats: the loss, 0, 0, 0), or one for one critic;
    `out`: the result of an earlier call of the same kind."""
    single = isinstance(critics, SoftCritic)
    critics = (critics,) if single else _pair(critics)
    D, k = _sizes(critics[0])
    outs = _rows.critic_gradient(_ls, 'soft', critics, (D, k), obs, action, target, idx, out, n_blocks, (
        Gradients, (D + k, 1, _lf.VALUE), (D + k, 1), _fresh, SoftCritic.as_struct_on,
        "Gradients (one per critic) of a soft_critic_gradient call for critics of %d first-layer inputs" % (D + k)))
    return outs[0] if single else outs


def soft_actor_gradient(policy, critics, obs, eps, log_alpha, target_entropy, *, act_scale=None, act_shift=None, idx=None, out=None,
                        action_out=None, logp_out=None, q_out=None, dqda_out=None, n_blocks=0):
    """The gradient of  (exp(log_alpha) * logp - min_j Q_j(obs, a)).mean()  over the rows of obs [..., D] (or those `idx` names),
    a and logp the squashed Gaussian of `policy` with the caller's eps [M, k], with respect to the six tensors of the mu network
    and the six of the sigma network; the pair of ONLINE SoftCritic is only read.  -> ActorGradients (.mu, .sigma: fit.Gradients
    of the value head's key; .stats; .loss; .alpha_grad).  action_out [M, k], logp_out [M], q_out [M, 2] and dqda_out [M, k]
    (of the critic with the smaller q) are optional."""
    critics = _pair(critics)
    D, k = _sizes(critics[0])
    _policy_checks(policy, D, k)
    lead = rows_of(obs, 'obs')
    te = float(target_entropy)
    if te != te or abs(te) == float('inf'):
        raise ValueError("target_entropy must be finite, got %r" % (target_entropy,))
    ts = [check_rows(obs, 'obs', lead, D, obs)]
    launch = one_launch(ts, ('obs',), lead)
    idx = checked_idx(idx, obs)
    M = n_rows(idx, launch)
    n_blocks = checked_blocks(n_blocks, _ls.MAX_BLOCKS)
    a = _ls.new_args(_ls.ActorArgs)
    keep, ins = [], inputs(ts, ('obs',), idx)
    _squash_args(a, keep, obs, k, M, eps, log_alpha, act_scale, act_shift, ins)
    needs_gpu(obs, 'soft')
    lib = _ls.load()
    need = sized(_ls, lib.atacom_soft_workspace_size(DTYPES[obs.dtype], 2, D, k, M, n_blocks))
    key = (D, k, _lf.VALUE, obs.dtype, obs.device)
    if out is None:
        out = ActorGradients(*_fresh(2, need, key))
    else:
        reuse((out,), ActorGradients, key, need, lambda: "ActorGradients of a soft_actor_gradient call for a %d -> %d policy in %s on %s" % (
            D, k, obs.dtype, obs.device))
    outs = [(out.mu.flat, 'out.mu.flat'), (out.sigma.flat, 'out.sigma.flat'), (out.stats, 'out.stats'), (out.workspace, 'out.workspace')]
    optional_rows(a, outs, obs, M, [('action_out', action_out, k), ('logp_out', logp_out, 1), ('q_out', q_out, 2), ('dqda_out', dqda_out, k)])
    no_overlap(outs, ins)
    fill(a, obs, n_blocks, launch, ('obs',), ts, idx)
    a.policy = policy.as_struct_on(obs.device, obs.dtype)
    for j, c in enumerate(critics):
        a.critics[j] = c.as_struct_on(obs.device, obs.dtype)
    a.target_entropy = te
    a.grad_mu, a.grad_sigma, a.stats = out.mu.flat.data_ptr(), out.sigma.flat.data_ptr(), out.stats.data_ptr()
    run(a, lib.atacom_soft_actor_gradient, _ls.check, obs, out.workspace)
    return out


class AlphaAdam:
    """torch.optim.Adam's default step on the one value `log_alpha` (a contiguous CUDA tensor of one float32 or float64 value,
    updated in place), its step count, running beta powers, m and v in device memory: step(grad) is one tiny launch that reads
    the gradient from a one-value device tensor (ActorGradients.alpha_grad) -- the host reads nothing."""

    def __init__(self, log_alpha, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
        if not isinstance(log_alpha, torch.Tensor) or log_alpha.numel() != 1 or log_alpha.dtype not in DTYPES or not log_alpha.is_contiguous():
            raise ValueError("log_alpha must be a contiguous tensor of one float32 or float64 value")
        if not (isinstance(betas, (list, tuple)) and len(betas) == 2 and all(0.0 <= float(b) < 1.0 for b in betas)):
            raise ValueError("betas must be two numbers in [0, 1), got %r" % (betas,))
        if not float(lr) >= 0.0 or float(lr) == float('inf'):
            raise ValueError("lr must be >= 0 and finite, got %r" % (lr,))
        if not float(eps) > 0.0 or float(eps) == float('inf'):
            raise ValueError("eps must be > 0 and finite, got %r" % (eps,))
        needs_gpu(log_alpha, 'soft')
        self.log_alpha, self.lr, self.betas, self.eps = log_alpha.detach(), float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.state = torch.zeros(_ls.ALPHA_STATE, dtype=torch.uint8, device=log_alpha.device)
        self.step_count = self.state[:8].view(torch.int64)
        self.pows = self.state[8:24].view(torch.float64)
        self.moments = self.state[32:32 + 2 * log_alpha.element_size()].view(log_alpha.dtype)
        self._lib = _ls.load()
        self.zero_state()

    def zero_state(self):
        """A fresh state: step 0, beta powers 1, zero moments (device fills, no synchronisation)."""
        self.state.zero_()
        self.pows.fill_(1.0)

    def step(self, grad):
        if not isinstance(grad, torch.Tensor) or grad.numel() != 1 or grad.dtype != self.log_alpha.dtype or grad.device != self.log_alpha.device:
            raise ValueError("grad must be a tensor of one %s value on %s" % (self.log_alpha.dtype, self.log_alpha.device))
        a = _ls.new_args(_ls.AlphaArgs)
        a.device, a.dtype = self.log_alpha.device.index, DTYPES[self.log_alpha.dtype]
        a.log_alpha, a.grad, a.state = self.log_alpha.data_ptr(), grad.data_ptr(), self.state.data_ptr()
        a.lr, a.beta1, a.beta2, a.eps = self.lr, self.betas[0], self.betas[1], self.eps
        a.stream = stream(a.device)
        _ls.check(self._lib.atacom_soft_alpha_step(a))

    def snapshot(self):
        """Device clones of the state and of log_alpha.  Not capturable: it allocates."""
        return [self.state.clone(), self.log_alpha.clone()]

    def restore(self, s):
        if not isinstance(s, (list, tuple)) or len(s) != 2 or s[0].shape != self.state.shape or s[1].shape != self.log_alpha.shape:
            raise ValueError("not a snapshot of this optimiser")
        self.state.copy_(s[0])
        self.log_alpha.copy_(s[1])
