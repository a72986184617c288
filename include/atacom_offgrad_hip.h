/* libatacom_offgrad.so -- the backward half of an off-policy update (DDPG, TD3), on the device: the gradient of the critics'
 * mean-squared TD error and the deterministic policy gradient of the actor, over a minibatch gathered through a list of row
 * numbers from a replay memory in place.  One launch per call, plus a small one that adds the workgroups' partial sums.  Plain
 * C11.  Like libatacom_fit.so it has no handle, keeps no state, belongs to no environment and reads records where they lie.
 *
 * Conventions of atacom_hip.h: every pointer of a network or held by a view is DEVICE memory owned by the caller; all work is
 * enqueued on `stream` (a hipStream_t passed as void*, NULL = the null stream) of device `device`; return codes are 0 or
 * negative (ATACOM_OFFGRAD_E_*), atacom_offgrad_last_error() gives the message of the calling thread's last failure.  Argument
 * validation happens before any device call.  Nothing synchronises and nothing is allocated: the caller passes a workspace of
 * atacom_offgrad_workspace_size() bytes, so a call can be captured in a HIP graph.  There are no atomics: with the same
 * n_blocks a repeated call gives the same bits. */
#ifndef ATACOM_OFFGRAD_HIP_H
#define ATACOM_OFFGRAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "atacom_evaluate_hip.h" /* atacom_evaluate_view; atacom_mlp through atacom_hip.h */

#ifdef __cplusplus
extern "C" {
#endif

#define ATACOM_OFFGRAD_F32 0
#define ATACOM_OFFGRAD_F64 1

#define ATACOM_OFFGRAD_OK 0
#define ATACOM_OFFGRAD_E_INVALID (-1)     /* bad argument */
#define ATACOM_OFFGRAD_E_HIP (-2)         /* a HIP runtime call failed */
#define ATACOM_OFFGRAD_E_UNSUPPORTED (-3) /* no kernel for the dtype or the network, or a grid the launch cannot express */

#define ATACOM_OFFGRAD_DDPG 0 /* first layer on the observation: W1 [64, D] */
#define ATACOM_OFFGRAD_TD3 1  /* first layer on [observation | action / act_scale]: W1 [64, D + k] */

#define ATACOM_OFFGRAD_MAX_IN 32 /* the first layer's inputs n1, and D */
#define ATACOM_OFFGRAD_MAX_ACT 8
#define ATACOM_OFFGRAD_HIDDEN 64
#define ATACOM_OFFGRAD_MAX_BLOCKS 65535
#define ATACOM_OFFGRAD_MAX_ROWS 2147483647 /* n_outer * n_inner of one call, and n_idx */
#define ATACOM_OFFGRAD_STATS 4

/* The critic of the reference's DDPG and TD3 agents, field for field the atacom_offpolicy_critic of atacom_offpolicy_hip.h
 * (a struct filled for one library passes to the other by a cast).  With D = n_obs, k = n_act, xn = (x - obs_shift) * obs_scale
 * and as = a / act_scale (one IEEE division per element):
 *     x1 = xn (DDPG)  |  [xn | as] (TD3)                 n1 = D  |  D + k  <=  32
 *     a1 = W1 x1 + b1,           h1 = act(a1)
 *     a2 = W2 h1 + W2a as + b2,  h2 = act(a2)
 *     q  = W3 h2 + b3
 * Every matrix is row-major like a torch.nn.Linear weight. */
typedef struct atacom_offgrad_critic {
    int32_t kind;       /* ATACOM_OFFGRAD_DDPG / ATACOM_OFFGRAD_TD3 */
    int32_t n_obs;      /* D, 1 .. 32 */
    int32_t n_act;      /* k, 1 .. 8 */
    int32_t activation; /* 0 = ReLU, 1 = tanh */
    const void *W1, *b1; /* [64, n1], [64] */
    const void *W2, *b2; /* [64, 64], [64] */
    const void *W2a;     /* [64, k] */
    const void *W3, *b3; /* [1, 64], [1] */
    const void *obs_shift, *obs_scale; /* [D], may be NULL (identity) */
    const void *act_scale;             /* [k], the divisor; NULL = 1 */
} atacom_offgrad_critic;

/* Rows are addressed as in atacom_evaluate_hip.h: row (o, i) of a view starts at ptr[o * stride_outer + i * stride_inner],
 * strides in ELEMENTS, the elements of a row contiguous; the flat number of that row is o * n_inner + i.  The M rows of a call
 * are the rows idx[r], r < n_idx, or every row once in order without idx; repeats are allowed and THE KERNEL DOES NOT GUARD AN
 * INDEX OUT OF RANGE.  target, action_out and dqda_out hold one row per row r of the CALL (not per row of the views): row r
 * starts at ptr[r * stride], stride in elements and at least the row's width.
 *
 * The gradient of a critic, `grad`, is one buffer of 64 n1 + 64 + 4096 + 64 + 64 + 1 + 64 k values in the order dW1 [64, n1],
 * db1, dW2, db2, dW3 [1, 64], db3, dW2a [64, k]; `stats` holds ATACOM_OFFGRAD_STATS values, the loss first and zeros after it. */
typedef struct atacom_offgrad_critic_args {
    uint32_t struct_size; /* = sizeof(atacom_offgrad_critic_args) */
    int32_t device;       /* HIP device index of every pointer of the call */
    int32_t dtype;        /* ATACOM_OFFGRAD_F32 / ATACOM_OFFGRAD_F64: the networks, the rows and the outputs */
    int32_t n_blocks;     /* workgroups per critic; 0 = the library chooses */
    int32_t n_critics;    /* 1 (DDPG) or 2 (TD3); both have the same kind, n_obs and n_act */
    int32_t reserved;     /* 0 */
    int64_t n_outer, n_inner; /* both >= 1; n_outer * n_inner rows in the views, at most ATACOM_OFFGRAD_MAX_ROWS */
    atacom_offgrad_critic critics[2];
    atacom_evaluate_view obs;    /* rows of D */
    atacom_evaluate_view action; /* rows of k */
    const void* target;          /* M rows of 1: row r for row r of the call */
    int64_t target_stride;
    const int64_t* idx;          /* n_idx flat row numbers in [0, n_outer * n_inner); NULL = every row once, in order */
    int64_t n_idx;               /* >= 1 with idx, ignored without */
    void* grad[2];               /* OUT per critic, see above */
    void* stats[2];              /* OUT per critic */
    void* workspace;             /* atacom_offgrad_workspace_size() bytes, aligned to 16; its content is of no meaning afterwards */
    size_t workspace_bytes;
    void* stream;
} atacom_offgrad_critic_args;

typedef struct atacom_offgrad_actor_args {
    uint32_t struct_size; /* = sizeof(atacom_offgrad_actor_args) */
    int32_t device;
    int32_t dtype;
    int32_t n_blocks;
    int64_t n_outer, n_inner;
    atacom_mlp actor;     /* hidden = 64, n_in = D, n_out = k, mean_mode 0 or 1 with act_scale; obs_shift and obs_scale are
                             honoured; std, explore, act_low, act_high and the ou_* fields are NOT READ; a sigma network or
                             squash is refused */
    atacom_offgrad_critic critic; /* only read */
    atacom_evaluate_view obs;     /* rows of D */
    const int64_t* idx;
    int64_t n_idx;
    void* grad;           /* OUT 64 D + 64 + 4096 + 64 + 64 k + k values: dW1, db1, dW2, db2, dW3, db3 of the ACTOR */
    void* stats;          /* OUT ATACOM_OFFGRAD_STATS values: the loss -mean(q), then zeros */
    void* action_out;     /* OUT M rows of k: a below; NULL = not wanted (the gradient holds the same bits either way) */
    int64_t action_out_stride;
    void* dqda_out;       /* OUT M rows of k: dq/da below; NULL = not wanted */
    int64_t dqda_out_stride;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} atacom_offgrad_actor_args;

const char* atacom_offgrad_version(void);
const char* atacom_offgrad_last_error(void);

/* Bytes of workspace of a call: n_nets (the critics of a critic call, 1 for an actor call) times the effective number of
 * workgroups times the values of one partial -- those of the gradient, with n_in the first layer's inputs (n1 of the critics, D
 * of the actor), n_out = 1 and n_act = k for critics and n_out = k, n_act = 0 for the actor, plus ATACOM_OFFGRAD_STATS -- in the
 * dtype, rounded up to a multiple of 256.  `rows` = M.  0 for arguments that no call accepts (last_error says which). */
size_t atacom_offgrad_workspace_size(int32_t dtype, int32_t n_nets, int32_t n_in, int32_t n_out, int32_t n_act, int64_t rows,
                                     int32_t n_blocks);

/* For each critic j, the gradient of  L_j = mean_r (Q_j(obs[row], action[row]) - target[r])^2  with respect to W1, b1, W2, b2,
 * W3, b3 and W2a, and stats[j][0] = L_j.  Per row, each line one individually rounded operation (no contraction):
 *     d  = q - target[r];   dy = 2 d;   loss term d * d
 *     delta2 = (W3^T dy) * act'(h2),   delta1 = (W2^T delta2) * act'(h1)       act' from the activation's value:
 *                                                                              h > 0 (ReLU), fma(-h, h, 1) (tanh)
 *     dW3 += dy h2^T, db3 += dy, dW2 += delta2 h1^T, db2 += delta2, dW2a += delta2 as^T, dW1 += delta1 x1^T, db1 += delta1
 * and the sums over the M rows are divided by M once, at the end.
 *
 * Float32 runs forward and backward on the matrix cores (v_mfma_f32_16x16x4_f32, a wavefront takes 64 rows as four blocks of
 * 16, transposed so that a layer's accumulators are the next layer's B operands); the weight-gradient accumulators stay in
 * registers for a wavefront's whole walk, wavefronts 1 - 3 hand theirs to wavefront 0 through LDS, each workgroup writes one
 * partial to the workspace and a second kernel adds the partials in a fixed order.  Float64 runs on the vector unit: one
 * record per row in LDS, fused multiply-adds.  The two critics of a pair are independent workgroups of one launch (the grid's
 * second dimension): the result of each is that of a call with it alone, bit for bit.
 * No output may overlap an input, the workspace or another output (byte extents are compared). */
int atacom_offgrad_critic_gradient(const atacom_offgrad_critic_args* args);

/* The deterministic policy gradient: the gradient of  L = -mean_r Q(obs[row], pi(obs[row]))  with respect to the ACTOR's W1, b1,
 * W2, b2, W3, b3; stats[0] = L.  Per row, each line individually rounded:
 *     m  = actor(obs);   t = tanh(m), a = act_scale_pi * t  (mean_mode 1;  a = m for mean_mode 0)
 *     as = a / act_scale_Q;   q = Q(obs, a)
 *     delta2 = W3^T * act'(h2),   delta1 = (W2^T delta2) * act'(h1)                        of the critic, from dq = 1
 *     dq/das = W2a^T delta2  (+ W1[:, D:]^T delta1 for TD3);   dq/da = (dq/das) / act_scale_Q
 *     dm = -(dq/da * (act_scale_pi * fma(-t, t, 1)))   (mean_mode 1;  dm = -dq/da for mean_mode 0)
 * then the actor's backward pass from dm as in atacom_offgrad_critic_gradient, the sums divided by M at the end.  One network is
 * resident in LDS at a time: a workgroup walks actor forward -> critic forward and input gradient -> actor forward again and
 * backward as phases over a tile of 64 rows per wavefront (float32), restaging behind a barrier; a row's action and dq/da
 * travel between the phases in the registers of the lane that owns it.  The actor's activations are recomputed in the last
 * phase rather than kept.  Float64 reads the weights from memory and needs no phases.
 * action_out receives a and dqda_out receives dq/da. */
int atacom_offgrad_actor_gradient(const atacom_offgrad_actor_args* args);

#ifdef __cplusplus
}
#endif
#endif
