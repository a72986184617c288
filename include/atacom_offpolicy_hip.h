/* libatacom_offpolicy.so -- the forward half of an off-policy update (DDPG, TD3), on the device: the Q-value of the
 * reference's two-branch critic, the fused TD target  r + gamma (1 - absorbing) min_j Q'_j(s', clip(pi'(s') + clip(sigma eps)))
 * of a minibatch gathered through a list of row numbers from a replay memory in place, and the soft update of the target
 * networks; one launch each.  Plain C11.  Like libatacom_fit.so it has no handle, keeps no state, belongs to no environment
 * and reads records where they lie.
 *
 * Conventions of atacom_hip.h: every pointer of a network or held by a view is DEVICE memory owned by the caller; all work is
 * enqueued on `stream` (a hipStream_t passed as void*, NULL = the null stream) of device `device`; return codes are 0 or
 * negative (ATACOM_OFFPOLICY_E_*), atacom_offpolicy_last_error() gives the message of the calling thread's last failure.
 * Argument validation happens before any device call.  Nothing synchronises and nothing is allocated -- no call needs a
 * workspace -- so a call can be captured in a HIP graph. */
#ifndef ATACOM_OFFPOLICY_HIP_H
#define ATACOM_OFFPOLICY_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "atacom_evaluate_hip.h" /* atacom_evaluate_view; atacom_mlp through atacom_hip.h */

#ifdef __cplusplus
extern "C" {
#endif

#define ATACOM_OFFPOLICY_F32 0
#define ATACOM_OFFPOLICY_F64 1

#define ATACOM_OFFPOLICY_OK 0
#define ATACOM_OFFPOLICY_E_INVALID (-1)     /* bad argument */
#define ATACOM_OFFPOLICY_E_HIP (-2)         /* a HIP runtime call failed */
#define ATACOM_OFFPOLICY_E_UNSUPPORTED (-3) /* no kernel for the dtype or the network, or a grid the launch cannot express */

#define ATACOM_OFFPOLICY_DDPG 0 /* first layer on the observation: W1 [64, D] */
#define ATACOM_OFFPOLICY_TD3 1  /* first layer on [observation | action / act_scale]: W1 [64, D + k] */

#define ATACOM_OFFPOLICY_MAX_IN 32 /* the first layer's inputs n1, and D */
#define ATACOM_OFFPOLICY_MAX_ACT 8
#define ATACOM_OFFPOLICY_HIDDEN 64
#define ATACOM_OFFPOLICY_MAX_BLOCKS 65535
#define ATACOM_OFFPOLICY_MAX_ROWS 2147483647 /* n_outer * n_inner of one call, and n_idx */
#define ATACOM_OFFPOLICY_MAX_PAIRS 4
#define ATACOM_OFFPOLICY_TENSORS 7

/* The critic of the reference's DDPG and TD3 agents (examples/network.py: DDPGCriticNetwork, TD3CriticNetwork): the action
 * enters the second layer through a bias-free Linear(k, 64) and is divided by act_scale first.  With D = n_obs, k = n_act,
 * xn = (x - obs_shift) * obs_scale and as = a / act_scale (one IEEE division per element):
 *     x1 = xn (DDPG)  |  [xn | as] (TD3)                 n1 = D  |  D + k  <=  32
 *     a1 = W1 x1 + b1,           h1 = act(a1)
 *     a2 = W2 h1 + W2a as + b2,  h2 = act(a2)
 *     q  = W3 h2 + b3
 * Every matrix is row-major like a torch.nn.Linear weight. */
typedef struct atacom_offpolicy_critic {
    int32_t kind;       /* ATACOM_OFFPOLICY_DDPG / ATACOM_OFFPOLICY_TD3 */
    int32_t n_obs;      /* D, 1 .. 32 */
    int32_t n_act;      /* k, 1 .. 8 */
    int32_t activation; /* 0 = ReLU, 1 = tanh */
    const void *W1, *b1; /* [64, n1], [64] */
    const void *W2, *b2; /* [64, 64], [64] */
    const void *W2a;     /* [64, k] */
    const void *W3, *b3; /* [1, 64], [1] */
    const void *obs_shift, *obs_scale; /* [D], may be NULL (identity) */
    const void *act_scale;             /* [k], the divisor; NULL = 1 */
} atacom_offpolicy_critic;

/* Rows are addressed as in atacom_evaluate_hip.h: row (o, i) of a view starts at ptr[o * stride_outer + i * stride_inner],
 * strides in ELEMENTS, the elements of a row contiguous; the flat number of that row is o * n_inner + i.  The M rows of a call
 * are the rows idx[r], r < n_idx, or every row once in order without idx; the contract of idx is that of atacom_fit_args.idx:
 * repeats are allowed and THE KERNEL DOES NOT GUARD AN INDEX OUT OF RANGE.  An output, and eps, hold one row per row r of the
 * CALL (not per row of the views): row r starts at ptr[r * stride], stride in elements and at least the row's width. */
typedef struct atacom_offpolicy_q_args {
    uint32_t struct_size; /* = sizeof(atacom_offpolicy_q_args) */
    int32_t device;       /* HIP device index of every pointer of the call */
    int32_t dtype;        /* ATACOM_OFFPOLICY_F32 / ATACOM_OFFPOLICY_F64: the network, the rows and the outputs */
    int32_t n_blocks;     /* workgroups of the launch; 0 = the library chooses */
    int64_t n_outer, n_inner; /* both >= 1; n_outer * n_inner rows in the views, at most ATACOM_OFFPOLICY_MAX_ROWS */
    atacom_offpolicy_critic critic;
    atacom_evaluate_view obs;    /* rows of D */
    atacom_evaluate_view action; /* rows of k */
    const int64_t* idx;          /* n_idx flat row numbers in [0, n_outer * n_inner); NULL = every row once, in order */
    int64_t n_idx;               /* >= 1 with idx, ignored without */
    void* q;                     /* OUT M rows of 1 */
    int64_t q_stride;
    void* stream;
} atacom_offpolicy_q_args;

typedef struct atacom_offpolicy_target_args {
    uint32_t struct_size; /* = sizeof(atacom_offpolicy_target_args) */
    int32_t device;
    int32_t dtype;
    int32_t n_blocks;
    int32_t n_critics;    /* 1 (DDPG) or 2 (TD3: the minimum of the two); both have the same kind, n_obs and n_act */
    int32_t reserved;     /* 0 */
    int64_t n_outer, n_inner;
    atacom_mlp actor;     /* the target actor: hidden = 64, n_in = D, n_out = k, mean_mode 0 or 1 with act_scale; obs_shift and
                             obs_scale are honoured; std, explore, act_low, act_high and the ou_* fields are NOT READ (a policy
                             built for the rollout passes as it is); a sigma network or squash is refused */
    atacom_offpolicy_critic critics[2];
    atacom_evaluate_view next_obs;  /* rows of D */
    atacom_evaluate_view reward;    /* rows of 1 */
    atacom_evaluate_view absorbing; /* rows of 1: 0.0 / 1.0 in the dtype, read as > 0.5 */
    const void* eps;      /* M rows of k standard normals drawn by the caller, row r for row r of the call; NULL = no noise */
    int64_t eps_stride;
    double noise_std, noise_clip, gamma; /* each rounded once to the dtype; noise_std, noise_clip >= 0, gamma finite */
    const void *act_low, *act_high;      /* [k], both or neither: the bounds the noisy action is clamped to */
    const int64_t* idx;
    int64_t n_idx;
    void* y;              /* OUT M rows of 1: the target */
    int64_t y_stride;
    void* action_out;     /* OUT M rows of k: a'' below; NULL = not wanted (y holds the same bits either way) */
    int64_t action_out_stride;
    void* stream;
} atacom_offpolicy_target_args;

/* One (target, online) pair of parameter sets of the soft update.  Tensor order: W1 [64, n_in], b1 [64], W2 [64, 64], b2 [64],
 * W3 [n_out, 64], b3 [n_out], W2a [64, n_act]; n_act = 0 for a plain network (entry 6 is not read), k for a critic. */
typedef struct atacom_offpolicy_pair {
    int32_t n_in, n_out, n_act, reserved;
    void* target[ATACOM_OFFPOLICY_TENSORS];       /* read and written */
    const void* online[ATACOM_OFFPOLICY_TENSORS]; /* only read */
} atacom_offpolicy_pair;

typedef struct atacom_offpolicy_soft_update_args {
    uint32_t struct_size; /* = sizeof(atacom_offpolicy_soft_update_args) */
    int32_t device;
    int32_t dtype;
    int32_t n_pairs;      /* 1 .. ATACOM_OFFPOLICY_MAX_PAIRS */
    double tau;           /* in [0, 1] */
    void* stream;
    atacom_offpolicy_pair pairs[ATACOM_OFFPOLICY_MAX_PAIRS];
} atacom_offpolicy_soft_update_args;

const char* atacom_offpolicy_version(void);
const char* atacom_offpolicy_last_error(void);

/* q[r] = Q(obs[row], action[row]) of the critic above for the M rows of the call, in one launch.
 *
 * Float32 runs the three layers on the matrix cores (v_mfma_f32_16x16x4_f32, one wavefront = 64 rows as four blocks of 16):
 * layer 2 accumulates the 16 K-steps of W2 h1 and then ceil(k / 4) more of W2a as.  Float64 runs on the vector unit with four
 * lanes per row and fused multiply-adds.  The weights are staged in LDS by the workgroup, which walks the row tiles
 * b, b + n_blocks, ...  The result of a row does not depend on n_blocks, on the strides or on the row's position in the call.
 * q must not overlap obs, action or idx (their byte extents are compared); rows that the call does not name and the padding
 * between rows are neither read nor written. */
int atacom_offpolicy_q(const atacom_offpolicy_q_args* args);

/* MushroomRL's DDPG._next_q / TD3._next_q followed by  reward + gamma * q_next, in one launch.  Per row of the call:
 *     m   = actor(next_obs);   a' = act_scale * tanh(m)  (mean_mode 1;  a' = m for mean_mode 0)
 *     n   = min(max(noise_std * eps, -noise_clip), +noise_clip)        (only with eps; 0 otherwise)
 *     a'' = min(max(a' + n, act_low), act_high)                        (the clamp only with bounds)
 *     q   = min_j Q_j(next_obs, a'')
 *     y   = reward + gamma * ((1 - absorbing) * q)
 * Every operation of these lines is individually rounded (no contraction); 1 - absorbing is 0 or 1.  action_out receives a''.
 * The kernel shape is that of atacom_offpolicy_q; one network is resident in LDS at a time, and a workgroup walks actor ->
 * critic 1 -> critic 2 as phases over its rows (one tile of 64 per wavefront in float32, of 16 in float64), restaging between
 * phases behind a barrier, with a'' and q_1 of a row in the registers of the lane that owns it.  Nothing per row but y and
 * action_out is written to memory.
 * y and action_out must not overlap next_obs, reward, absorbing, eps, idx or each other. */
int atacom_offpolicy_target(const atacom_offpolicy_target_args* args);

/* MushroomRL's _update_target,  target = tau * online + (1 - tau) * target,  for 1 to 4 pairs in one launch (one workgroup per
 * pair).  With a = (T) tau and b = (T)(1.0 - tau), the subtraction in double and rounded once:
 *     target = fl(fl(a * online) + fl(b * target))
 * three individually rounded operations in the arrays' own precision.  Online tensors are only read.  A target tensor must
 * overlap no other tensor of the call, within or across pairs (byte extents are compared). */
int atacom_offpolicy_soft_update(const atacom_offpolicy_soft_update_args* args);

#ifdef __cplusplus
}
#endif
#endif
