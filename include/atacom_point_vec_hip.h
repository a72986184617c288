/* libatacom_point_vec.so -- the collision-avoidance task (PointReachAtacom) driven step by step without the host in the loop:
 * a masked step (the vectorised surface of MushroomRL 2: step_all(env_mask, action)) and a checkpoint of the whole handle.
 * Plain C11.  The fifth library of the project: like libatacom_point_policy.so and libatacom_point_compact.so it works on the
 * handles of libatacom_point.so (include/atacom_point_hip.h) and adds nothing to that library.  Both must come from the same
 * build of this tree: a handle whose layout number is not the one this library was compiled with is refused (E_INVALID).
 *
 * Conventions of atacom_point_hip.h: every pointer named d_* is DEVICE memory owned by the caller, of the handle's dtype unless
 * stated; all work is enqueued on `stream` (a hipStream_t passed as void*, NULL = the null stream); return codes are 0 or
 * negative (ATACOM_POINT_E_*), atacom_point_vec_last_error() gives the message of the calling thread's last failure.  Argument
 * validation happens before any device call.  Only atacom_point_vec_snapshot_inspect and atacom_point_vec_snapshot_restore
 * synchronise `stream` (once, to read 64 bytes); every other call is enqueue-only and can be captured in a HIP graph. */
#ifndef ATACOM_POINT_VEC_HIP_H
#define ATACOM_POINT_VEC_HIP_H

#include "atacom_point_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char* atacom_point_vec_last_error(void);
const char* atacom_point_vec_version(void);

/* atacom_point_step for the environments whose byte of d_mask (uint8 [batch]; NULL = everybody) is not zero.  One launch
 * whatever the mask; the mask is read on the device only.
 *   masked in   exactly atacom_point_step, bit for bit: the action, the supplied draws or the generator, the reward, last = 1
 *               at the horizon, the constraint statistics, and the reset inside the call of a handle with cfg.auto_reset.
 *   masked out  nothing of the environment is written: not its state, not its step and episode counters, not its constraint
 *               statistics.  It reports the observation of its current state, reward 0, absorbing 0, last 0.  Its rows of
 *               d_action and d_draws are not read.
 * The generator is keyed (seed, environment, the environment's OWN episode counter, a draw index made from its OWN step
 * counter): sitting a call out consumes no random numbers, and an environment that has taken j steps has drawn what it would
 * have drawn in j calls of atacom_point_step, whatever the other environments did meanwhile.
 * d_action [batch, 2]; d_draws (nullable) [batch, N, 2]; d_obs [batch, 4 (1 + N)], aligned to four elements; d_reward [batch];
 * d_absorbing uint8 [batch]; d_last (nullable) uint8 [batch]. */
int atacom_point_vec_step_masked(atacom_point_handle* h, const uint8_t* d_mask, const void* d_action, const void* d_draws,
                                 void* d_obs, void* d_reward, uint8_t* d_absorbing, uint8_t* d_last, void* stream);

/* Checkpoint of the whole handle.  An image is opaque: a 64-byte header (a format number, dtype, n_objects, batch and the
 * generator key) followed by the handle's two device buffers verbatim -- the state, the step and episode counters AND the
 * constraint statistics, which atacom_point_get_state / atacom_point_set_state leave out.  Its size depends on dtype, n_objects
 * and batch only; d_image must be aligned to 16 bytes.  Returns the size in bytes, or a negative code. */
int64_t atacom_point_vec_snapshot_bytes(const atacom_point_handle* h);

/* Writes an image of atacom_point_vec_snapshot_bytes(h) bytes.  One launch, no host staging and no synchronisation: the header
 * is written on the device from the launch arguments.  The generator key recorded is the handle's at the time of the CALL
 * (a captured save keeps the key it was captured with, like every captured step). */
int atacom_point_vec_snapshot_save(atacom_point_handle* h, void* d_image, void* stream);

/* Reads the header of an image (synchronises `stream` once) and checks ALL of it against the handle: format, dtype, n_objects,
 * batch.  Writes nothing to the handle.  *seed (nullable) receives the image's generator key.  A mismatch is E_INVALID and the
 * message names the field, e.g. "image n_objects = 2, handle 4".  For a caller that knows the size of its buffer: an image
 * that passes has exactly atacom_point_vec_snapshot_bytes(h) bytes. */
int atacom_point_vec_snapshot_inspect(atacom_point_handle* h, const void* d_image, int32_t* seed, void* stream);

/* The checks of atacom_point_vec_snapshot_inspect first, BEFORE anything is written: a rejected image leaves the state, the
 * statistics and the generator key of the handle exactly as they were.  Then the two buffers are copied back on `stream` (one
 * launch) and the handle adopts the image's generator key, as atacom_point_set_seed would.  Everything else of the
 * configuration -- horizon, dt, the obstacle mode, auto_reset -- is not part of an image and stays the handle's. */
int atacom_point_vec_snapshot_restore(atacom_point_handle* h, const void* d_image, void* stream);

#ifdef __cplusplus
}
#endif
#endif
