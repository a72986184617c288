/* libatacom_point_policy.so -- the collision-avoidance task (PointReachAtacom) collected with the actor network evaluated
 * inside the rollout kernel.  Plain C11.  The third library of the project: it works on the handles of libatacom_point.so
 * (include/atacom_point_hip.h, which creates, resets, inspects and destroys them) and takes the network description of
 * libatacom_hip.so (include/atacom_hip.h: atacom_mlp, semantics unchanged).  Both libraries must come from the same build of
 * this tree: a handle whose layout number is not the one this library was compiled with is refused (E_INVALID).
 *
 * Conventions of the two other headers: every pointer named d_* is DEVICE memory owned by the caller, of the handle's dtype
 * unless stated; launches go to the caller's stream (a hipStream_t passed as void*, NULL = the default stream); no call
 * synchronises; return codes are 0 or negative (ATACOM_POINT_E_*), atacom_point_policy_last_error() gives the message of the
 * calling thread's last failure.  Argument validation happens before any device call.
 *
 * Reference lines: examples/collision_avoidance_exp.py (the five agents' policies, cited per entry),
 * examples/network.py (the actor networks), atacom/environments/collision_avoidance/ (the task). */
#ifndef ATACOM_POINT_POLICY_HIP_H
#define ATACOM_POINT_POLICY_HIP_H

#include "atacom_hip.h"
#include "atacom_point_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char* atacom_point_policy_last_error(void);
const char* atacom_point_policy_version(void);

/* n_steps consecutive steps in ONE launch with the policy evaluated in the kernel: per step
 *   obs -> MLP((obs - obs_shift) * obs_scale) -> exploration -> the env step of atacom_point_rollout.
 * Replaces the loop of mushroom_rl.core.Core that examples/collision_avoidance_exp.py:56,73 runs around
 * agent.policy.draw_action and PointReachAtacom.step (collision_avoidance_atacom.py:30-52), for the policies that script
 * builds: GaussianTorchPolicy on PPONetwork / TRPONetwork (:145-217), SAC's squashed Gaussian on two SACActorNetworks
 * (:309-348), ClippedGaussianPolicy on TD3ActorNetwork (:265-306), OrnsteinUhlenbeckPolicy on DDPGActorNetwork (:220-262).
 *
 * The layout is that of atacom_point_rollout with d_actions [n_steps, batch, 2] an OUTPUT (the action the policy drew, which
 * is what the step received: TD3's is the clipped one, DDPG's mean + x is unclipped):
 *   d_noise  [n_steps, batch, 2] standard-normal draws supplied by the caller, NULL = zeros (the kernel draws none);
 *   d_draws  [n_steps, batch, n_objects, 2] values of U(-1, 1) for the random walk, NULL = the device generator with the keys
 *            of atacom_point_rollout;
 *   d_obs, d_next_obs (may be NULL) [n_steps, batch, 4 (1 + n_objects)], aligned to four elements;
 *   d_reward [n_steps, batch]; d_absorbing, d_last [n_steps, batch] (uint8).
 * net: atacom_mlp as documented in atacom_hip.h -- struct_size (ATACOM_MLP_SIZE_V1 accepted), n_in = 4 (1 + n_objects),
 * n_out = 2, hidden = 64, activation 0 / 1, obs_shift / obs_scale, std, the sigma network with its clamp and squash,
 * mean_mode, explore 0 / 1 / 2 with act_scale / act_low / act_high, ou_theta / ou_dt / ou_x0 and ou_state [batch, 2], which is
 * set to ou_x0 before the draw of any step at which the environment's episode step counter is 0 (after an explicit, masked
 * or in-kernel reset).  Weights are device memory of the handle's dtype.  A value outside this list is
 * ATACOM_POINT_E_UNSUPPORTED with a message that names it.
 * The constraint statistics of the steps taken accumulate into the handle (atacom_point_get_stats sees them); the in-kernel
 * auto-reset at the horizon and the recorded terminal observation are those of atacom_point_rollout. */
int atacom_point_policy_rollout(atacom_point_handle* h, int32_t n_steps, const atacom_mlp* net, const void* d_noise,
                                const void* d_draws, void* d_obs, void* d_next_obs, void* d_actions, void* d_reward,
                                uint8_t* d_absorbing, uint8_t* d_last, void* stream);

/* The same rollout writing ONE packed record per (step, env) instead of six arrays -- the contract of atacom_rollout_packed:
 *   d_records [n_steps, record_batch_stride, record_dim],  record_dim = 2 * 4 (1 + n_objects) + 5,
 *   record = [obs | action(2) | reward | next_obs | absorbing (0/1) | last (0/1)]
 * (the (s, a, r, s', absorbing, last) tuple of mushroom_rl.Core's dataset, examples/collision_avoidance_exp.py:73), laid out
 * so that a sharded collector all-gathers the buffer as it is.  Exactly one of d_actions ([n_steps, batch, 2], pre-generated
 * actions as in atacom_point_rollout; d_noise is then ignored) and net must be given.  record_batch_stride >= batch; rows
 * batch..stride-1 are never written.  d_records needs the alignment of one element only. */
int atacom_point_policy_rollout_packed(atacom_point_handle* h, int32_t n_steps, const void* d_actions, const atacom_mlp* net,
                                       const void* d_noise, const void* d_draws, void* d_records,
                                       int32_t record_batch_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
