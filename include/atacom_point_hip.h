/* atacom_point_hip.h -- C ABI of libatacom_point.so: the reference's collision-avoidance task, PointReachAtacom
 * (atacom/environments/collision_avoidance/collision_avoidance_atacom.py:8 on collision_avoidance_base.py:6), batched for the
 * MI355X (gfx950), one environment per lane.
 *
 * A library of its own beside libatacom_hip.so (atacom_hip.h): the task has moving constraints (obstacle positions and
 * velocities enter psi and c), no sub-steps, no puck and its own state layout, so it has its own handle type.  The
 * conventions are those of atacom_hip.h: plain C types; every d_* pointer is DEVICE memory owned by the caller; `stream`
 * is a hipStream_t (NULL = the null stream); all work is enqueued asynchronously on `stream` except
 * atacom_point_get_stats, which synchronises that stream to return three numbers.  Every float buffer of a handle has the
 * element type chosen at creation (cfg.dtype).  Buffers of observation rows (d_obs, d_next_obs) must be aligned to four
 * elements (16 bytes float32, 32 bytes float64).
 *
 * Return value: 0 on success, negative on error; atacom_point_last_error() gives the message of the last failing call
 * on the calling thread.  A handle must not be used from two threads at once; distinct handles are independent.
 *
 * Layouts (N = n_objects):
 *   observation row   4 (1 + N):  q(2), dq(2), then p_i(2), dp_i(2) per obstacle      (collision_avoidance_base.py:11,28-37)
 *   action            2:          the null-space coordinates alpha (not clipped; the resulting acceleration is)
 *   state row         7 N + 8:    observation row, s(N), first-reset circle centres (N x 2), _time, steps taken in the
 *                                 episode, episodes started, 1 if the centres are set
 *   draws             the values np.random.uniform returned: reset [batch, N, 2] of U(2, 8); step [batch, N, 2] of U(-1, 1).
 *                     A NULL d_draws selects the counter-based generator of the engine keyed (seed, env, episode, draw):
 *                     reset draw 2 i + c -> 2 + 6 u; step t, draw 2 N + 2 (N t + i) + c -> -1 + 2 u.
 */
#ifndef ATACOM_POINT_HIP_H
#define ATACOM_POINT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ATACOM_POINT_F32 0
#define ATACOM_POINT_F64 1

#define ATACOM_POINT_OK 0
#define ATACOM_POINT_E_INVALID (-1)     /* bad argument / inconsistent config */
#define ATACOM_POINT_E_HIP (-2)         /* a HIP runtime call failed */
#define ATACOM_POINT_E_UNSUPPORTED (-3) /* n_objects other than 2 and 4 */

typedef struct atacom_point_config {
    int32_t struct_size; /* = sizeof(atacom_point_config); checked by atacom_point_create */
    int32_t batch;       /* number of independent environments held by the handle */
    int32_t dtype;       /* ATACOM_POINT_F32 / ATACOM_POINT_F64 */
    int32_t n_objects;   /* obstacles: 2 or 4 (class default 4, collision_avoidance_atacom.py:9) */
    int32_t random_walk; /* 1 = obstacles random-walk (the example's default); 0 = they circle (the class default) */
    int32_t horizon;     /* MDPInfo.horizon (1000); the only thing that ends an episode */
    int32_t auto_reset;  /* 1 = an env whose step returned last=1 is reset inside the same call with generator draws;
                            the returned observation is still the terminal one */
    int32_t seed;        /* key of the counter-based generator */
    double dt;           /* time_step (0.01) */
    double gamma;        /* MDPInfo.gamma (0.99); carried for the binding, no kernel reads it */
} atacom_point_config;

typedef struct atacom_point_handle atacom_point_handle;

/* the reference's defaults: batch 1, float32, n_objects 4, random_walk 0, horizon 1000, auto_reset 1, dt 0.01, gamma 0.99 */
int atacom_point_default_config(atacom_point_config* cfg);

/* Allocates the state of cfg->batch environments on `device`.  The reference's constructor does not call reset() and
 * neither does this: the state is zero and no circle centres are set until the first atacom_point_reset. */
int atacom_point_create(const atacom_point_config* cfg, int device, atacom_point_handle** out);
int atacom_point_destroy(atacom_point_handle* h);

/* PointReachAtacom.reset (collision_avoidance_atacom.py:19-28).  d_mask (nullable): uint8 [batch], environments with a
 * zero byte keep their state.  d_draws (nullable): [batch, N, 2].  d_obs (nullable): [batch, 4 (1 + N)]. */
int atacom_point_reset(atacom_point_handle* h, const uint8_t* d_mask, const void* d_draws, void* d_obs, void* stream);

/* PointReachAtacom.step (:30-52).  d_action [batch, 2]; d_draws (nullable) [batch, N, 2]; d_obs [batch, 4 (1 + N)];
 * d_reward [batch]; d_absorbing uint8 [batch] (always 0); d_last (nullable) uint8 [batch]. */
int atacom_point_step(atacom_point_handle* h, const void* d_action, const void* d_draws, void* d_obs, void* d_reward,
                      uint8_t* d_absorbing, uint8_t* d_last, void* stream);

/* n_steps steps in one launch, in the layout of atacom_rollout: d_actions [n_steps, batch, 2]; d_draws (nullable)
 * [n_steps, batch, N, 2]; d_obs / d_next_obs (nullable) [n_steps, batch, 4 (1 + N)]; d_reward, d_absorbing, d_last
 * [n_steps, batch].  Equal to n_steps calls of atacom_point_step bit for bit. */
int atacom_point_rollout(atacom_point_handle* h, int32_t n_steps, const void* d_actions, const void* d_draws, void* d_obs,
                         void* d_next_obs, void* d_reward, uint8_t* d_absorbing, uint8_t* d_last, void* stream);

/* get_constraints_logs (:133-139) over every step of every environment since the last clear: out = {mean of the
 * per-step max_i c_i, max of it, 0}.  Synchronises `stream`. */
int atacom_point_get_stats(atacom_point_handle* h, double out[3], int32_t clear, void* stream);

/* d_state: [batch, 7 N + 8] state rows */
int atacom_point_get_state(atacom_point_handle* h, void* d_state, void* stream);
int atacom_point_set_state(atacom_point_handle* h, const void* d_state, void* stream);

int atacom_point_set_seed(atacom_point_handle* h, int32_t seed);

const char* atacom_point_last_error(void);
const char* atacom_point_version(void);

#ifdef __cplusplus
}
#endif
#endif
