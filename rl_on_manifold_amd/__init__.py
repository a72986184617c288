"""rl_on_manifold_amd -- MI355X-native batched ATACOM environment-step engine.

The hot path (constraint Jacobian assembly, null-space basis, pseudo-inverse solve, error correction,
slack integration, acceleration truncation, forward kinematics / Jacobians, dynamics, reward,
termination, constraint statistics) is hand-written HIP for gfx950 in `csrc/`, behind the C ABI of
`include/atacom_hip.h`; the Python here mirrors the reference's env surface and moves pointers only.
"""
from ._lib import AtacomError, LIB_PATH  # noqa: F401


def __getattr__(name):
    # torch is imported lazily so that `import rl_on_manifold_amd` (and the build) stay cheap
    if name in ('BatchedAtacomEnv', 'nullspace', 'constraint_terms', 'MlpPolicy', 'inverse_dynamics', 'forward_dynamics',
                'GraphedRollout', 'canonical_mu'):
        from . import engine
        return getattr(engine, name)
    if name in ('CircleEnvAtacom', 'AirHockeyPlanarAtacom', 'AirHockeyIiwaAtacom', 'CircleEnvErrorCorrection',
                'CircleEnvTerminated', 'VectorizedAtacomEnv', 'VectorizedPointReachEnv'):
        from . import envs
        return getattr(envs, name)
    if name in ('RolloutCollector', 'RecordLayout', 'CompactRecordLayout'):
        from . import rollout
        return getattr(rollout, name)
    if name in ('compute_gae', 'compute_J', 'episode_returns', 'normalize_advantages', 'gae_from_records', 'gae_from_compact'):
        from . import returns
        return getattr(returns, name)
    if name in ('evaluate_mlp', 'gaussian_log_prob', 'values_from_records', 'values_from_compact', 'log_prob_from_records',
                'evaluate_rows'):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ('value_gradient', 'policy_gradient', 'value_gradient_from_records', 'policy_gradient_from_records', 'Gradients'):
        from . import fit
        return getattr(fit, name)
    if name in ('Adam', 'GraphedUpdate'):
        from . import optim
        return getattr(optim, name)
    if name in ('fisher_vector_product', 'fisher_vector_product_from_records', 'natural_gradient', 'trpo_step', 'FisherProduct',
                'CgWork'):
        from . import trust
        return getattr(trust, name)
    if name in ('QCritic', 'q_values', 'td_target', 'soft_update', 'ReplayMemory'):
        from . import offpolicy
        return getattr(offpolicy, name)
    if name in ('critic_gradient', 'actor_gradient', 'QGradients'):
        from . import offgrad
        return getattr(offgrad, name)
    if name in ('TrackedAdam', 'GraphedFit'):
        from . import offstep
        return getattr(offstep, name)
    if name in ('SoftCritic', 'soft_td_target', 'soft_critic_gradient', 'soft_actor_gradient', 'AlphaAdam', 'ActorGradients'):
        from . import soft
        return getattr(soft, name)
    if name in ('BatchedPointReachEnv', 'PointReachAtacom'):
        from . import point
        return getattr(point, name)
    raise AttributeError(name)
