/* libatacom_point_compact.so -- the collision-avoidance task (PointReachAtacom) collected in the COMPACT record format, which
 * does not repeat next_obs.  Plain C11.  The fourth library of the project: like libatacom_point_policy.so it works on the
 * handles of libatacom_point.so (include/atacom_point_hip.h) and takes the network description of libatacom_hip.so
 * (include/atacom_hip.h: atacom_mlp).  All of them must come from the same build of this tree: a handle whose layout number is
 * not the one this library was compiled with is refused (E_INVALID).
 *
 * Conventions of the other headers: every pointer named d_* is DEVICE memory owned by the caller, of the handle's dtype unless
 * stated; launches go to the caller's stream (a hipStream_t passed as void*, NULL = the default stream); no call synchronises;
 * return codes are 0 or negative (ATACOM_POINT_E_*), atacom_point_compact_last_error() gives the message of the calling
 * thread's last failure.  Argument validation happens before any device call. */
#ifndef ATACOM_POINT_COMPACT_HIP_H
#define ATACOM_POINT_COMPACT_HIP_H

#include "atacom_hip.h"
#include "atacom_point_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char* atacom_point_compact_last_error(void);
const char* atacom_point_compact_version(void);

/* atacom_point_policy_rollout_packed (include/atacom_point_policy_hip.h) in the compact record format -- the contract of
 * atacom_rollout_compact (include/atacom_hip.h).  next_obs of step t is the obs of step t + 1 except where an in-kernel reset
 * came between, so it is not stored per record.  With T = n_steps, Bm = record_batch_stride, D = 4 (1 + n_objects):
 *   d_records [T + 1, Bm, D + 5]: rows 0..T-1 = [obs | action(2) | reward | absorbing (0/1) | last (0/1)]; row T is the tail
 *            [obs after step T-1, before that step's auto-reset | five zeros] (the zeros are written by the kernel).  Rows
 *            batch..Bm-1 are never written.  Needs the alignment of one element only.
 *   d_ends   [ends_capacity, D + 2]: one row [t, b, terminal obs] per t < T-1 at which environment b of a handle with
 *            cfg.auto_reset reached last = 1 (its next record holds the reset state); t and b are exact integers in the
 *            handle's float type.  Rows are appended through an atomic counter: their order is unspecified.  Without
 *            auto_reset no row is written.  May be NULL only when ends_capacity == 0.
 *   d_n_ends device int32, required: zeroed on `stream` (hipMemsetAsync) at the start of the call, it counts EVERY episode
 *            end, those past the capacity included; rows at an index >= ends_capacity are not written.
 * Exactly one of d_actions ([T, batch, 2], pre-generated actions as in atacom_point_rollout; d_noise is then ignored) and net
 * (the variants and messages of atacom_point_policy_rollout_packed) must be given; d_noise [T, batch, 2] or NULL = zeros;
 * d_draws [T, batch, n_objects, 2] values of U(-1, 1) for the random walk, NULL = the device generator with the keys of
 * atacom_point_rollout.  n_steps and record_batch_stride must be < 2^24.  The call never synchronises the host (it can be
 * captured in a HIP graph); the state, the constraint statistics and the generator keys advance exactly as in
 * atacom_point_rollout. */
int atacom_point_compact_rollout(atacom_point_handle* h, int32_t n_steps, const void* d_actions, const atacom_mlp* net,
                                 const void* d_noise, const void* d_draws, void* d_records, int32_t record_batch_stride,
                                 void* d_ends, int32_t ends_capacity, int32_t* d_n_ends, void* stream);

#ifdef __cplusplus
}
#endif
#endif
