/* libatacom_returns.so -- what an on-policy learner computes from a finished collection, on the device and in one launch
 * per quantity: generalised advantage estimates with their returns, the optional advantage normalisation of PPO, and the
 * discounted episode returns J.  Plain C11.  The sixth library of the project and the only one without a handle: it keeps no
 * state, belongs to no environment and reads the records of any of them where they lie.
 *
 * Conventions of atacom_hip.h: every pointer named d_* or held by a view is DEVICE memory owned by the caller; all work is
 * enqueued on `stream` (a hipStream_t passed as void*, NULL = the null stream) of device `device`; return codes are 0 or
 * negative (ATACOM_RETURNS_E_*), atacom_returns_last_error() gives the message of the calling thread's last failure.
 * Argument validation happens before any device call.  Nothing synchronises and nothing is allocated: every call can be
 * captured in a HIP graph.
 *
 * Arithmetic.  MushroomRL is the specification (mushroom_rl/utils/value_functions.py: compute_gae; mushroom_rl/utils/dataset.py:
 * compute_J; mushroom_rl/algorithms/actor_critic/deep_actor_critic/ppo.py for the normalisation), restated from its published
 * 1.x source and not pinned against an installed copy.  The contraction is fixed, not left to the compiler: fma(a, b, c) below
 * is one fused multiply-add of the call's dtype (one rounding), every other operation a single IEEE operation rounded to
 * nearest, in the order written. */
#ifndef ATACOM_RETURNS_HIP_H
#define ATACOM_RETURNS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ATACOM_RETURNS_F32 0
#define ATACOM_RETURNS_F64 1

#define ATACOM_RETURNS_FLAG_U8 0    /* flags are bytes, true = non-zero (bool / uint8 tensors) */
#define ATACOM_RETURNS_FLAG_VALUE 1 /* flags have the call's dtype, true = greater than 0.5 (the columns of packed records) */

#define ATACOM_RETURNS_OK 0
#define ATACOM_RETURNS_E_INVALID (-1)     /* bad argument */
#define ATACOM_RETURNS_E_HIP (-2)         /* a HIP runtime call failed */
#define ATACOM_RETURNS_E_UNSUPPORTED (-3) /* no kernel for the dtype, or a shape the launch cannot express */

/* Doubles of device workspace a call needs for n_blocks x batch environments (per-environment partial sums and the first
 * reduction stage). */
#define ATACOM_RETURNS_WORKSPACE_DOUBLES(n_blocks, batch) (3 * ((int64_t)(n_blocks) * (int64_t)(batch) + 256))

/* One array of a collection, addressed where it lies: element (t, b, w) -- step, environment of a block, block -- is
 * ptr[t * stride_t + b * stride_b + w * stride_w], strides in ELEMENTS, any sign, 0 allowed for inputs.  This reads a
 * contiguous [T, B] array (stride_t = B, stride_b = 1), a column of full records [W, T, Bm, 2 D + k + 3], a column of compact
 * records [W, T + 1, Bm, D + k + 3] and a shifted view v[:, 1:] alike. */
typedef struct atacom_returns_view {
    void* ptr;
    int64_t stride_t, stride_b, stride_w;
} atacom_returns_view;

/* The shape every call shares. */
typedef struct atacom_returns_shape {
    int32_t device;         /* HIP device index of every pointer of the call */
    int32_t dtype;          /* ATACOM_RETURNS_F32 / ATACOM_RETURNS_F64: rewards, values and outputs */
    int32_t flag_dtype;     /* ATACOM_RETURNS_FLAG_*: absorbing and last */
    int32_t n_steps;        /* T >= 1 */
    int32_t batch;          /* Bm >= 1: environments per block (the padded size of ragged shards) */
    int32_t n_blocks;       /* W >= 1: blocks (ranks of a gathered collection); 1 for plain [T, B] arrays */
    const int32_t* d_sizes; /* device int32 [W]: block w holds d_sizes[w] <= Bm real environments, the rest is padding;
                               NULL = every row is real.  Read on the device only. */
} atacom_returns_shape;

typedef struct atacom_returns_gae_args {
    uint32_t struct_size; /* = sizeof(atacom_returns_gae_args) */
    int32_t normalize;    /* 1 = follow the recurrence with atacom_returns_normalize on `adv` */
    atacom_returns_shape shape;
    double gamma, lam; /* both in [0, 1]; rounded to the dtype, and gamma * lam formed once, on the host, in the dtype */
    atacom_returns_view reward, absorbing, last;
    atacom_returns_view v, v_next; /* both pointers NULL = zeros (with lam = 1: the discounted return-to-go) */
    atacom_returns_view ret, adv;  /* outputs */
    double* d_workspace;           /* normalize only: ATACOM_RETURNS_WORKSPACE_DOUBLES(n_blocks, batch) doubles */
    double* d_stats;               /* normalize only: receives [count, mean, std] */
    void* stream;
} atacom_returns_gae_args;

typedef struct atacom_returns_normalize_args {
    uint32_t struct_size; /* = sizeof(atacom_returns_normalize_args) */
    int32_t reserved;
    atacom_returns_shape shape; /* flag_dtype is not read */
    atacom_returns_view adv;    /* normalised in place */
    double* d_workspace;        /* ATACOM_RETURNS_WORKSPACE_DOUBLES(n_blocks, batch) doubles */
    double* d_stats;            /* receives [count, mean, std] */
    void* stream;
} atacom_returns_normalize_args;

typedef struct atacom_returns_episodes_args {
    uint32_t struct_size; /* = sizeof(atacom_returns_episodes_args) */
    int32_t reserved;
    atacom_returns_shape shape;
    double gamma; /* in [0, 1]; 1 gives the undiscounted return R */
    atacom_returns_view reward, last;
    double* d_workspace; /* ATACOM_RETURNS_WORKSPACE_DOUBLES(n_blocks, batch) doubles */
    double* d_result;    /* receives [sum of j over the episodes, number of episodes, sum of j * j] */
    void* stream;
} atacom_returns_episodes_args;

const char* atacom_returns_version(void);
const char* atacom_returns_last_error(void);

/* MushroomRL's compute_gae(V, s, ss, r, absorbing, last, gamma, lam) with the critic already evaluated: replaces the loop
 * `for t in reversed(range(T))` of an on-policy learner.  Per environment, for t = T-1 ... 0 with A[T] = 0:
 *     vn     = absorbing[t] ? 0 : v_next[t]          a select: v_next may hold anything (NaN, Inf) under an absorbing flag
 *     d      = fma(gamma, vn, reward[t]) - v[t]
 *     A[t]   = fma(gamma * lam, last[t] ? 0 : A[t+1], d)
 *     ret[t] = A[t] + v[t]
 * which is compute_gae wherever absorbing implies last (every engine of this project guarantees it, atacom_hip.h:
 * atacom_step).  One lane per (block, environment), the time axis walked backwards with the loads of later iterations issued
 * ahead of their use; padding rows are computed like any other (from whatever the inputs hold there).
 * normalize = 1 then runs atacom_returns_normalize on `adv`; `ret` is not affected.
 * The outputs must not overlap any input or each other: a lane loads several steps ahead of the step it stores. */
int atacom_returns_gae(const atacom_returns_gae_args* args);

/* PPO's advantage normalisation, adv <- (adv - mean) / (std + 1e-8) (ppo.py: _update_policy's caller), std in the population
 * form, the statistics over the real rows only (d_sizes).  Sum and sum of squares are accumulated in double: per environment
 * over time, then by a two-stage tree of fixed shape -- no atomics, the same bits on every run.  The application is a launch of
 * its own that reads mean and std from d_stats on the device and computes ((double)adv - mean) / (std + 1e-8) in double from
 * the statistics exactly as they are returned, rounded once to the dtype.  Padding rows are left as they are.  With no real row
 * at all (every d_sizes[w] = 0) the statistics are [0, 0, 0] and nothing is written.
 * adv is read and written in place, element by element; d_workspace and d_stats must not overlap it. */
int atacom_returns_normalize(const atacom_returns_normalize_args* args);

/* MushroomRL's compute_J(dataset, gamma) as the reference's experiment scripts use it after every epoch (compute_metrics of
 * examples/collision_avoidance_exp.py and its three siblings: J = mean(compute_J(dataset, gamma)), R = mean(compute_J(dataset))).
 * Per real environment, forward in time, with j = 0 and p = 1:
 *     j = fma(p, reward[t], j);  p = p * gamma
 * and at last[t], or at t = T-1 (the unfinished episode counts, as in MushroomRL), the episode's j is emitted and j, p start
 * again.  An episode that was already running at t = 0 starts with exponent 0, as a flat dataset would.  The episodes' j, j * j
 * and their number are summed in double by the reduction of atacom_returns_normalize; the mean is d_result[0] / d_result[1]. */
int atacom_returns_episodes(const atacom_returns_episodes_args* args);

#ifdef __cplusplus
}
#endif
#endif
