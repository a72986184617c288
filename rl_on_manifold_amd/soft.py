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
from .evaluate import _check_rows
from .fit import Gradients
from .offpolicy import _bound, _idx, _one_launch, _rows_out
from .returns import _overlap, _stream

_DTYPES = {torch.float32: _ls.F32, torch.float64: _ls.F64}
_CRITIC_KEYS = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'obs_shift', 'obs_scale')


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
        device = torch.device(device)
        dev = {k: (None if v is None else torch.as_tensor(v).detach().to(device=device, dtype=dtype).contiguous())
               for k, v in self.tensors.items()}
        self._keep = dev
        D, k = self.n_obs, self.n_act
        for name, shape in (('W1', (64, D + k)), ('b1', (64,)), ('W2', (64, 64)), ('b2', (64,)), ('W3', (1, 64)), ('b3', (1,)),
                            ('obs_shift', (D,)), ('obs_scale', (D,))):
            if dev[name] is not None and tuple(dev[name].shape) != shape:
                raise ValueError("%s has the shape %s where the critic needs %s" % (name, tuple(dev[name].shape), shape))
        c = _ls.Critic()
        c.n_obs, c.n_act, c.activation = D, k, self.activation
        for name in _CRITIC_KEYS:
            setattr(c, name, None if dev[name] is None else dev[name].data_ptr())
        return c


class ActorGradients:
    """What soft_actor_gradient writes: `mu` and `sigma`, the fit.Gradients of the two networks (they share one workspace), and
    `stats` [4] = the loss mean(alpha logp - min q), mean(logp), -(mean(logp) + target_entropy) -- the gradient of the alpha loss
    with respect to log_alpha, what AlphaAdam.step takes -- and the share of rows with a clamped log sigma."""

    def __init__(self, mu, sigma):
        self.mu, self.sigma, self.stats = mu, sigma, mu.stats

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


def _checked_blocks(n_blocks):
    if not isinstance(n_blocks, int) or not 0 <= n_blocks <= _ls.MAX_BLOCKS:
        raise ValueError("n_blocks must be 0 (the library chooses) or 1 .. %d" % _ls.MAX_BLOCKS)
    return n_blocks


def _obs_checks(obs, what='obs'):
    if not isinstance(obs, torch.Tensor) or obs.dim() < 1:
        raise ValueError("%s must be a tensor [..., n]" % what)
    if obs.dtype not in _DTYPES:
        raise ValueError("%s must be float32 or float64, got %s" % (what, obs.dtype))
    lead = tuple(obs.shape[:-1])
    if any(n == 0 for n in lead) or not lead:
        raise ValueError("%s holds no rows: %s" % (what, tuple(obs.shape)))
    return lead


def _needs_gpu(x):
    if x.device.type != 'cuda':                            # the last check that needs no device
        raise ValueError("the kernels of libatacom_soft.so run on a GPU; got tensors on %s" % x.device)


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
    eps, a.eps_stride = _rows_out(eps, 'eps', M, k, x)
    a.eps = eps.data_ptr()
    a.log_alpha = _log_alpha(log_alpha, x).data_ptr()
    ins += [(eps, 'eps'), (log_alpha, 'log_alpha')]
    for name, v in (('act_scale', act_scale), ('act_shift', act_shift)):
        if v is not None:
            t = _bound(v, k, x, name)
            keep.append(t)
            setattr(a, name, t.data_ptr())
            ins.append((t, name))


def _no_overlap(outs, ins):
    for o, oname in outs:
        for t, name in ins + [p for p in outs if p[0] is not o]:
            if _overlap(o, t):
                raise ValueError("%s overlaps %s: the call does not work in place" % (oname, name))


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
    lead = _obs_checks(next_obs, 'next_obs')
    if float(gamma) != float(gamma) or abs(float(gamma)) == float('inf'):
        raise ValueError("gamma must be finite, got %r" % (gamma,))
    if isinstance(absorbing, torch.Tensor) and absorbing.dtype == torch.bool:
        absorbing = absorbing.to(next_obs.dtype)
    one = lambda t: t.unsqueeze(-1) if isinstance(t, torch.Tensor) else t           # noqa: E731
    names = ('next_obs', 'reward', 'absorbing')
    ts = [_check_rows(next_obs, 'next_obs', lead, D, next_obs), _check_rows(one(reward), 'reward', lead, 1, next_obs),
          _check_rows(one(absorbing), 'absorbing', lead, 1, next_obs)]
    offs, n_outer, n_inner, strides = _one_launch(ts, names, lead)
    idx = _idx(idx, next_obs)
    M = idx.numel() if idx is not None else n_outer * n_inner
    n_blocks = _checked_blocks(n_blocks)
    a = _ls.new_args(_ls.TargetArgs)
    keep, ins = [], list(zip(ts, names)) + ([(idx, 'idx')] if idx is not None else [])
    _squash_args(a, keep, next_obs, k, M, eps, log_alpha, act_scale, act_shift, ins)
    y, a.y_stride = _rows_out(out, 'out', M, 1, next_obs)
    outs = [(y, 'out')]
    if action_out is not None:
        action_out, a.action_out_stride = _rows_out(action_out, 'action_out', M, k, next_obs)
        a.action_out = action_out.data_ptr()
        outs.append((action_out, 'action_out'))
    if logp_out is not None:
        logp_out, a.logp_out_stride = _rows_out(logp_out, 'logp_out', M, 1, next_obs)
        a.logp_out = logp_out.data_ptr()
        outs.append((logp_out, 'logp_out'))
    _no_overlap(outs, ins)
    _needs_gpu(next_obs)
    a.device, a.dtype, a.n_blocks, a.n_critics, a.n_outer, a.n_inner = next_obs.device.index, _DTYPES[next_obs.dtype], n_blocks, 2, n_outer, n_inner
    a.policy = policy.as_struct_on(next_obs.device, next_obs.dtype)
    for j, c in enumerate(critics):
        a.critics[j] = c.as_struct_on(next_obs.device, next_obs.dtype)
    size = next_obs.element_size()
    for t, name, off, st in zip(ts, names, offs, strides):
        setattr(a, name, _ls.View(t.data_ptr() + off * size, *st))
    if idx is not None:
        a.idx, a.n_idx = idx.data_ptr(), idx.numel()
    a.gamma, a.y, a.stream = float(gamma), y.data_ptr(), _stream(next_obs.device.index)
    _ls.check(_ls.load().atacom_soft_target(a))
    return y


def soft_critic_gradient(critics, obs, action, target, *, idx=None, out=None, n_blocks=0):
    """The gradient of  ((Q_j(obs, action) - target) ** 2).mean()  for the pair of SoftCritic (or one), over the rows of obs
    [..., D] and action [..., k] (strided views with contiguous rows, sharing their leading dimensions: the columns of a replay
    memory, read in place) -- or, with `idx`, over the rows it names.  target [M] belongs to row r of the CALL.
    -> a pair of fit.Gradients (n_in = D + k, n_out = 1, the value head's key; stats: the loss, 0, 0, 0), or one for one critic;
    `out`: the result of an earlier call of the same kind."""
    single = isinstance(critics, SoftCritic)
    critics = (critics,) if single else _pair(critics)
    D, k = _sizes(critics[0])
    n1 = D + k
    lead = _obs_checks(obs)
    ts = [_check_rows(obs, 'obs', lead, D, obs), _check_rows(action, 'action', lead, k, obs)]
    offs, n_outer, n_inner, strides = _one_launch(ts, ('obs', 'action'), lead)
    idx = _idx(idx, obs)
    M = idx.numel() if idx is not None else n_outer * n_inner
    if not isinstance(target, torch.Tensor) or tuple(target.shape) != (M,):
        raise ValueError("target must be a tensor of shape (%d,): one value per row of the call" % M)
    if target.dtype != obs.dtype or target.device != obs.device:
        raise ValueError("target must be a %s tensor on %s" % (obs.dtype, obs.device))
    n_blocks = _checked_blocks(n_blocks)
    _needs_gpu(obs)
    lib = _ls.load()
    need = lib.atacom_soft_workspace_size(_DTYPES[obs.dtype], len(critics), n1, 1, M, n_blocks)
    if need == 0:
        _ls.check(_ls.E_INVALID)
    key = (n1, 1, _lf.VALUE, obs.dtype, obs.device)
    if out is None:
        outs = tuple(Gradients(n1, 1, _lf.VALUE, obs.dtype, obs.device, need if j == 0 else 0, key) for j in range(len(critics)))
    else:
        outs = (out,) if isinstance(out, Gradients) else tuple(out)
        if len(outs) != len(critics) or not all(isinstance(o, Gradients) and o.key == key for o in outs):
            raise ValueError("out must be the Gradients (one per critic) of a soft_critic_gradient call for critics of %d first-layer "
                             "inputs in %s on %s" % (n1, obs.dtype, obs.device))
        if outs[0].workspace.numel() < need:
            raise ValueError("out was made for fewer workgroups: its workspace holds %d bytes where this call needs %d" % (
                outs[0].workspace.numel(), need))
    ins = list(zip(ts, ('obs', 'action'))) + [(target, 'target')] + ([(idx, 'idx')] if idx is not None else [])
    bufs = [(outs[0].workspace, 'the workspace')]
    for o in outs:
        bufs += [(o.flat, 'the gradients'), (o.stats, 'the statistics')]
    _no_overlap(bufs, ins)
    a = _ls.new_args(_ls.CriticArgs)
    a.device, a.dtype, a.n_blocks, a.n_critics, a.n_outer, a.n_inner = obs.device.index, _DTYPES[obs.dtype], n_blocks, len(critics), n_outer, n_inner
    for j, c in enumerate(critics):
        a.critics[j] = c.as_struct_on(obs.device, obs.dtype)
        a.grad[j], a.stats[j] = outs[j].flat.data_ptr(), outs[j].stats.data_ptr()
    size = obs.element_size()
    a.obs = _ls.View(ts[0].data_ptr() + offs[0] * size, *strides[0])
    a.action = _ls.View(ts[1].data_ptr() + offs[1] * size, *strides[1])
    a.target, a.target_stride = target.data_ptr(), (target.stride(0) if M > 1 else 1)
    if idx is not None:
        a.idx, a.n_idx = idx.data_ptr(), idx.numel()
    a.workspace, a.workspace_bytes = outs[0].workspace.data_ptr(), outs[0].workspace.numel()
    a.stream = _stream(obs.device.index)
    _ls.check(lib.atacom_soft_critic_gradient(a))
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
    lead = _obs_checks(obs)
    te = float(target_entropy)
    if te != te or abs(te) == float('inf'):
        raise ValueError("target_entropy must be finite, got %r" % (target_entropy,))
    ts = [_check_rows(obs, 'obs', lead, D, obs)]
    offs, n_outer, n_inner, strides = _one_launch(ts, ('obs',), lead)
    idx = _idx(idx, obs)
    M = idx.numel() if idx is not None else n_outer * n_inner
    n_blocks = _checked_blocks(n_blocks)
    a = _ls.new_args(_ls.ActorArgs)
    keep, ins = [], [(ts[0], 'obs')] + ([(idx, 'idx')] if idx is not None else [])
    _squash_args(a, keep, obs, k, M, eps, log_alpha, act_scale, act_shift, ins)
    _needs_gpu(obs)
    lib = _ls.load()
    need = lib.atacom_soft_workspace_size(_DTYPES[obs.dtype], 2, D, k, M, n_blocks)
    if need == 0:
        _ls.check(_ls.E_INVALID)
    key = (D, k, _lf.VALUE, obs.dtype, obs.device)
    if out is None:
        out = ActorGradients(Gradients(D, k, _lf.VALUE, obs.dtype, obs.device, need, key), Gradients(D, k, _lf.VALUE, obs.dtype, obs.device, 0, key))
    elif not isinstance(out, ActorGradients) or out.mu.key != key:
        raise ValueError("out must be the ActorGradients of a soft_actor_gradient call for a %d -> %d policy in %s on %s" % (D, k, obs.dtype, obs.device))
    elif out.mu.workspace.numel() < need:
        raise ValueError("out was made for fewer workgroups: its workspace holds %d bytes where this call needs %d" % (
            out.mu.workspace.numel(), need))
    outs = [(out.mu.flat, 'the gradients of mu'), (out.sigma.flat, 'the gradients of sigma'), (out.stats, 'the statistics'),
            (out.mu.workspace, 'the workspace')]
    for name, t, width in (('action_out', action_out, k), ('logp_out', logp_out, 1), ('q_out', q_out, 2), ('dqda_out', dqda_out, k)):
        if t is not None:
            t, stride = _rows_out(t, name, M, width, obs)
            setattr(a, name, t.data_ptr())
            setattr(a, name + '_stride', stride)
            outs.append((t, name))
    _no_overlap(outs, ins)
    a.device, a.dtype, a.n_blocks, a.n_outer, a.n_inner = obs.device.index, _DTYPES[obs.dtype], n_blocks, n_outer, n_inner
    a.policy = policy.as_struct_on(obs.device, obs.dtype)
    for j, c in enumerate(critics):
        a.critics[j] = c.as_struct_on(obs.device, obs.dtype)
    a.obs = _ls.View(ts[0].data_ptr() + offs[0] * obs.element_size(), *strides[0])
    if idx is not None:
        a.idx, a.n_idx = idx.data_ptr(), idx.numel()
    a.target_entropy = te
    a.grad_mu, a.grad_sigma, a.stats = out.mu.flat.data_ptr(), out.sigma.flat.data_ptr(), out.stats.data_ptr()
    a.workspace, a.workspace_bytes = out.mu.workspace.data_ptr(), out.mu.workspace.numel()
    a.stream = _stream(obs.device.index)
    _ls.check(lib.atacom_soft_actor_gradient(a))
    return out


class AlphaAdam:
    """torch.optim.Adam's default step on the one value `log_alpha` (a contiguous CUDA tensor of one float32 or float64 value,
    updated in place), its step count, running beta powers, m and v in device memory: step(grad) is one tiny launch that reads
    the gradient from a one-value device tensor (ActorGradients.alpha_grad) -- the host reads nothing."""

    def __init__(self, log_alpha, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
        if not isinstance(log_alpha, torch.Tensor) or log_alpha.numel() != 1 or log_alpha.dtype not in _DTYPES or not log_alpha.is_contiguous():
            raise ValueError("log_alpha must be a contiguous tensor of one float32 or float64 value")
        if not (isinstance(betas, (list, tuple)) and len(betas) == 2 and all(0.0 <= float(b) < 1.0 for b in betas)):
            raise ValueError("betas must be two numbers in [0, 1), got %r" % (betas,))
        if not float(lr) >= 0.0 or float(lr) == float('inf'):
            raise ValueError("lr must be >= 0 and finite, got %r" % (lr,))
        if not float(eps) > 0.0 or float(eps) == float('inf'):
            raise ValueError("eps must be > 0 and finite, got %r" % (eps,))
        _needs_gpu(log_alpha)
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
        a.device, a.dtype = self.log_alpha.device.index, _DTYPES[self.log_alpha.dtype]
        a.log_alpha, a.grad, a.state = self.log_alpha.data_ptr(), grad.data_ptr(), self.state.data_ptr()
        a.lr, a.beta1, a.beta2, a.eps = self.lr, self.betas[0], self.betas[1], self.eps
        a.stream = _stream(a.device)
        _ls.check(self._lib.atacom_soft_alpha_step(a))

    def snapshot(self):
        """Device clones of the state and of log_alpha.  Not capturable: it allocates."""
        return [self.state.clone(), self.log_alpha.clone()]

    def restore(self, s):
        if not isinstance(s, (list, tuple)) or len(s) != 2 or s[0].shape != self.state.shape or s[1].shape != self.log_alpha.shape:
            raise ValueError("not a snapshot of this optimiser")
        self.state.copy_(s[0])
        self.log_alpha.copy_(s[1])
