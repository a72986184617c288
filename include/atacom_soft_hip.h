/* libatacom_soft.so -- a SAC update on the device: the fused soft TD target, the gradients of the two critics' mean-squared
 * TD error, the gradients of the squashed-Gaussian actor's loss with respect to its mu and sigma networks, and the Adam step of
 * the temperature log_alpha, over a minibatch gathered through a list of row numbers from a replay memory in place.  Plain C11.
 * Like libatacom_offgrad.so it has no handle, keeps no state, belongs to no environment and reads records where they lie.
 *
 * Conventions of atacom_hip.h: every pointer of a network or held by a view is DEVICE memory owned by the caller; all work is
 * enqueued on `stream` (a hipStream_t passed as void*, NULL = the null stream) of device `device`; return codes are 0 or
 * negative (ATACOM_SOFT_E_*), atacom_soft_last_error() gives the message of the calling thread's last failure.  Argument
 * validation happens before any device call.  Nothing synchronises and nothing is allocated: the caller passes a workspace of
 * atacom_soft_workspace_size() bytes, so a call can be captured in a HIP graph.  There are no atomics: with the same n_blocks a
 * repeated call gives the same bits, and a row's own outputs (y, action_out, logp_out, q_out, dqda_out) do not depend on the
 * grid, the strides or the row's position.
 *
 * THE ROW ARITHMETIC (MushroomRL's SACPolicy.compute_action_and_log_prob_t restated).  The policy is an atacom_mlp as
 * MlpPolicy.from_sac fills it: the mu network W1 .. b3, the sigma network sW1 .. sb3, log_std_min, log_std_max, squash = 1;
 * obs_shift and obs_scale are honoured; std, explore, mean_mode and the ou_* fields are NOT READ; a policy without a sigma
 * network or without squash is refused.  For a row with observation x, xn = (x - obs_shift) * obs_scale and the caller's standard
 * normals eps[k], each line one individually rounded operation per element (no contraction), i = 0 .. k - 1 in order:
 *     m = Mu(xn),  l_raw = Sig(xn)                       (2 x 64 networks; float32 on the matrix cores, float64 by explicit fma)
 *     l = min(max(l_raw, log_std_min), log_std_max)
 *     s = exp(l)
 *     p = s * eps;   u = m + p
 *     t = tanh(u)
 *     a = act_scale * t;   a = a + act_shift             (NULL: 1 and 0 -- the two operations are still carried out)
 *     w = fma(-t, t, 1)
 *     e = w + 1e-6;   c = log(e)
 *     g_i = (-0.5 * eps_i) * eps_i;   g_i = g_i - l_i;   g_i = g_i - 0.5 log(2 pi)
 *     G = ((g_0 + g_1) + ...) + g_{k-1};   C = ((c_0 + c_1) + ...) + c_{k-1};   logp = G - C
 * The Gaussian term uses eps directly where torch forms (u - m) / s: the same value.  Its reparameterised gradient is the exact
 * cancellation: 0 with respect to m, -1 with respect to l.  alpha = exp(*log_alpha) is formed by every kernel from the device
 * value, so a step of log_alpha is seen by the next launch without the host. */
#ifndef ATACOM_SOFT_HIP_H
#define ATACOM_SOFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "atacom_evaluate_hip.h" /* atacom_evaluate_view; atacom_mlp through atacom_hip.h */

#ifdef __cplusplus
extern "C" {
#endif

#define ATACOM_SOFT_F32 0
#define ATACOM_SOFT_F64 1

#define ATACOM_SOFT_OK 0
#define ATACOM_SOFT_E_INVALID (-1)     /* bad argument */
#define ATACOM_SOFT_E_HIP (-2)         /* a HIP runtime call failed */
#define ATACOM_SOFT_E_UNSUPPORTED (-3) /* no kernel for the dtype or the network, or a grid the launch cannot express */

#define ATACOM_SOFT_MAX_IN 32 /* D + k, the critic's first-layer inputs */
#define ATACOM_SOFT_MAX_ACT 8
#define ATACOM_SOFT_HIDDEN 64
#define ATACOM_SOFT_MAX_BLOCKS 65535
#define ATACOM_SOFT_MAX_ROWS 2147483647 /* n_outer * n_inner of one call, and n_idx */
#define ATACOM_SOFT_STATS 4

/* The critic of the reference's SAC agent (SACCriticNetwork): a plain 2 x 64 network on x1 = [xn | a], the action RAW as its
 * forward concatenates it, xn = (x - obs_shift) * obs_scale:  q = W3 act(W2 act(W1 x1 + b1) + b2) + b3.  Every matrix is
 * row-major like a torch.nn.Linear weight. */
typedef struct atacom_soft_critic {
    int32_t n_obs;      /* D >= 1 */
    int32_t n_act;      /* k, 1 .. 8;  D + k <= 32 */
    int32_t activation; /* 0 = ReLU, 1 = tanh */
    int32_t reserved;   /* 0 */
    const void *W1, *b1; /* [64, D + k], [64] */
    const void *W2, *b2; /* [64, 64], [64] */
    const void *W3, *b3; /* [1, 64], [1] */
    const void *obs_shift, *obs_scale; /* [D], may be NULL (identity) */
} atacom_soft_critic;

/* Rows are addressed as in atacom_evaluate_hip.h: row (o, i) of a view starts at ptr[o * stride_outer + i * stride_inner],
 * strides in ELEMENTS, the elements of a row contiguous; the flat number of that row is o * n_inner + i.  The M rows of a call
 * are the rows idx[r], r < n_idx, or every row once in order without idx; repeats are allowed and THE KERNEL DOES NOT GUARD AN
 * INDEX OUT OF RANGE.  eps, target and the per-row outputs hold one row per row r of the CALL (not per row of the views): row r
 * starts at ptr[r * stride], stride in elements and at least the row's width.
 * No output may overlap an input, the workspace or another output (byte extents are compared). */
typedef struct atacom_soft_target_args {
    uint32_t struct_size; /* = sizeof(atacom_soft_target_args) */
    int32_t device;       /* HIP device index of every pointer of the call */
    int32_t dtype;        /* ATACOM_SOFT_F32 / ATACOM_SOFT_F64: the networks, the rows and the outputs */
    int32_t n_blocks;     /* workgroups; 0 = the library chooses */
    int32_t n_critics;    /* 2: the reference's SAC has two critics */
    int32_t reserved;     /* 0 */
    int64_t n_outer, n_inner; /* both >= 1; n_outer * n_inner rows in the views, at most ATACOM_SOFT_MAX_ROWS */
    atacom_mlp policy;
    atacom_soft_critic critics[2]; /* the TARGET critics; same n_obs and n_act */
    atacom_evaluate_view next_obs;  /* rows of D */
    atacom_evaluate_view reward;    /* rows of 1 */
    atacom_evaluate_view absorbing; /* rows of 1: 0.0 / 1.0 in the dtype, read as > 0.5 */
    const void* eps;       /* M rows of k standard normals drawn by the caller */
    int64_t eps_stride;
    const void *act_scale, *act_shift; /* [k], NULL = 1 and 0: MushroomRL's _delta_a and _central_a */
    const void* log_alpha; /* one value in the dtype */
    double gamma;          /* rounded once to the dtype; finite */
    const int64_t* idx;    /* n_idx flat row numbers in [0, n_outer * n_inner); NULL = every row once, in order */
    int64_t n_idx;         /* >= 1 with idx, ignored without */
    void* y;               /* OUT M rows of 1 */
    int64_t y_stride;
    void* action_out;      /* OUT M rows of k: a'; NULL = not wanted */
    int64_t action_out_stride;
    void* logp_out;        /* OUT M rows of 1: logp'; NULL = not wanted */
    int64_t logp_out_stride;
    void* stream;
} atacom_soft_target_args;

/* The gradient of critic j, `grad[j]`, is one buffer of 64 (D + k) + 64 + 4096 + 64 + 64 + 1 values in the order dW1, db1, dW2,
 * db2, dW3 [1, 64], db3 -- the layout of the gradient of a value network of n_in = D + k inputs and one output; `stats[j]`
 * holds ATACOM_SOFT_STATS values, the loss first and zeros after it. */
typedef struct atacom_soft_critic_args {
    uint32_t struct_size;
    int32_t device;
    int32_t dtype;
    int32_t n_blocks;     /* workgroups per critic; 0 = the library chooses */
    int32_t n_critics;    /* 1 or 2 (a pair is bit-equal to two calls with one) */
    int32_t reserved;
    int64_t n_outer, n_inner;
    atacom_soft_critic critics[2];
    atacom_evaluate_view obs;    /* rows of D */
    atacom_evaluate_view action; /* rows of k */
    const void* target;          /* M rows of 1: row r for row r of the call */
    int64_t target_stride;
    const int64_t* idx;
    int64_t n_idx;
    void* grad[2];
    void* stats[2];
    void* workspace;             /* atacom_soft_workspace_size() bytes, aligned to 16; its content is of no meaning afterwards */
    size_t workspace_bytes;
    void* stream;
} atacom_soft_critic_args;

typedef struct atacom_soft_actor_args {
    uint32_t struct_size;
    int32_t device;
    int32_t dtype;
    int32_t n_blocks;     /* workgroups per network of the policy; 0 = the library chooses */
    int64_t n_outer, n_inner;
    atacom_mlp policy;
    atacom_soft_critic critics[2]; /* the ONLINE critics, only read */
    atacom_evaluate_view obs;      /* rows of D */
    const void* eps;
    int64_t eps_stride;
    const void *act_scale, *act_shift;
    const void* log_alpha;
    double target_entropy; /* rounded once to the dtype */
    const int64_t* idx;
    int64_t n_idx;
    void* grad_mu;        /* OUT 64 D + 64 + 4096 + 64 + 64 k + k values: dW1, db1, dW2, db2, dW3, db3 of the mu network */
    void* grad_sigma;     /* OUT the same for the sigma network */
    void* stats;          /* OUT ATACOM_SOFT_STATS values, see atacom_soft_actor_gradient */
    void* action_out;     /* OUT M rows of k: a; NULL = not wanted (the gradients hold the same bits either way) */
    int64_t action_out_stride;
    void* logp_out;       /* OUT M rows of 1 */
    int64_t logp_out_stride;
    void* q_out;          /* OUT M rows of 2: q_1, q_2 */
    int64_t q_out_stride;
    void* dqda_out;       /* OUT M rows of k: dq/da of the selected critic */
    int64_t dqda_out_stride;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
} atacom_soft_actor_args;

/* torch.optim.Adam's default step (no weight decay, no amsgrad) on the ONE value log_alpha, the arithmetic of
 * include/atacom_optim_hip.h restated for one element.  `state` is ATACOM_SOFT_ALPHA_STATE bytes of device memory, aligned to
 * 8: the head of atacom_optim_hip.h -- int64 step; double beta1_pow; double beta2_pow; 8 reserved bytes -- and after it m and v
 * in the dtype.  A fresh optimiser has step = 0, beta1_pow = beta2_pow = 1 and everything else zero.  With g = *grad; lines
 * marked (double) are double arithmetic, every other operation is an individually rounded one of the dtype (no contraction),
 * sqrt and the divisions are IEEE:
 *     t = step + 1;  b1p = beta1_pow * beta1;  b2p = beta2_pow * beta2                      (double)
 *     step_size = lr / (1 - b1p);  bc2s = sqrt(1 - b2p)                                     (double, each rounded once to the dtype)
 *     omb1 = 1 - beta1;  omb2 = 1 - beta2                                                   (double, each rounded once to the dtype)
 *     beta2 and eps are rounded once to the dtype
 *     m = m + (g - m) * omb1
 *     v = beta2 * v + (omb2 * g) * g
 *     x = x - step_size * (m / (sqrt(v) / bc2s + eps))
 * and then the head becomes  step = t, beta1_pow = b1p, beta2_pow = b2p.  One launch of one thread; the host reads nothing. */
#define ATACOM_SOFT_ALPHA_STATE 48
typedef struct atacom_soft_alpha_args {
    uint32_t struct_size;
    int32_t device;
    int32_t dtype;
    int32_t reserved;
    void* log_alpha;     /* IN/OUT one value */
    const void* grad;    /* one value: element 2 of the actor call's stats */
    void* state;         /* IN/OUT ATACOM_SOFT_ALPHA_STATE bytes */
    double lr, beta1, beta2, eps;
    void* stream;
} atacom_soft_alpha_args;

const char* atacom_soft_version(void);
const char* atacom_soft_last_error(void);

/* Bytes of workspace of a critic call (n_nets = its critics, n_in = D + k, n_out = 1) or an actor call (n_nets = 2: mu and
 * sigma, n_in = D, n_out = k): n_nets times the effective number of workgroups times (the values of one gradient +
 * ATACOM_SOFT_STATS) in the dtype, rounded up to a multiple of 256.  `rows` = M.  0 for arguments that no call accepts. */
size_t atacom_soft_workspace_size(int32_t dtype, int32_t n_nets, int32_t n_in, int32_t n_out, int64_t rows, int32_t n_blocks);

/* MushroomRL's SAC._next_q and the target of SAC.fit in one launch.  Per row of the call, with (a', logp') the row arithmetic
 * above on next_obs and x1 = [xn_j | a'] with critic j's own normalisation:
 *     q = q_2 < q_1 ? q_2 : q_1
 *     z = alpha * logp';   z = q - z
 *     y = reward + gamma * ((1 - absorbing) * z)          (1 - absorbing is 0 or 1)
 * One launch whose workgroups walk the phases mu, sigma, critic 1, critic 2 over a tile of 64 rows per wavefront (float32), one
 * network resident in LDS at a time; a row's a', logp' and q_1 stay in the registers of the lane that owns it. */
int atacom_soft_target(const atacom_soft_target_args* args);

/* For each critic j, the gradient of  L_j = mean_r (Q_j([xn | action]) - target[r])^2  and stats[j][0] = L_j.  Per row:
 *     d = q - target[r];   dy = 2 d;   loss term d * d
 *     delta2 = (W3^T dy) * act'(h2),   delta1 = (W2^T delta2) * act'(h1)     act' from the activation's value:
 *                                                                            h > 0 (ReLU), fma(-h, h, 1) (tanh)
 *     dW3 += dy h2^T, db3 += dy, dW2 += delta2 h1^T, db2 += delta2, dW1 += delta1 x1^T, db1 += delta1
 * and the sums over the M rows are divided by M once, at the end.  Float32 runs on the matrix cores
 * (v_mfma_f32_16x16x4_f32, a wavefront takes 64 rows as four blocks of 16), the weight-gradient accumulators stay in registers
 * for a wavefront's whole walk, wavefronts 1 - 3 hand theirs to wavefront 0 through LDS, each workgroup writes one partial and
 * a second kernel adds the partials in a fixed order.  Float64 runs on the vector unit: one record per row in LDS, explicit
 * fused multiply-adds.  The two critics are independent workgroups of one launch (the grid's second dimension). */
int atacom_soft_critic_gradient(const atacom_soft_critic_args* args);

/* The gradient of  L = mean_r (alpha * logp - min_j Q_j([xn | a]))  with respect to the six tensors of the mu network and the six
 * of the sigma network; the critics are only read.  Per row, after the row arithmetic above, each line individually rounded:
 *     q = q_2 < q_1 ? q_2 : q_1                        (equal values: critic 1.  The reference's torch.min splits the gradient
 *                                                       0.5 / 0.5 between the critics at an exact tie; the device does not, by
 *                                                       design: tests/test_edge_cases_oracle.py shows the difference)
 *     delta2 = W3^T * act'(h2),  delta1 = (W2^T delta2) * act'(h1)  of that critic, from dq = 1
 *     dq/da = the a-columns of W1^T delta1
 *     r = (2 t) * w;   r = r / e                        (= d(-c)/du: c = log(w + 1e-6), dw/du = -2 t w)
 *     du = alpha * r - dq/da * (act_scale * w)
 *     dm = du
 *     dl = (du * p - alpha) * [log_std_min < l_raw < log_std_max]
 *                                                      (strict on both sides.  The reference's torch.clamp passes the gradient
 *                                                       where l_raw equals a bound exactly; the device gives dl = 0 there, by
 *                                                       design: tests/test_edge_cases_oracle.py shows the difference)
 * then the backward pass of Mu from dm and of Sig from dl as in atacom_soft_critic_gradient, the sums divided by M at the end.
 * stats[0] = L = mean_r (alpha logp - q), stats[1] = mean_r logp, stats[2] = mean_r -(logp + target_entropy) (the gradient of
 * MushroomRL's alpha loss with respect to log_alpha), stats[3] = the share of rows with an element of l clamped.
 * The grid's second dimension is the network whose gradient a workgroup accumulates (0 = mu, 1 = sigma): both halves walk the
 * forward phases mu, sigma, critic 1, critic 2 of their rows, then restage their own network and run it forward again and
 * backward; the statistics and the per-row outputs are written by the first half. */
int atacom_soft_actor_gradient(const atacom_soft_actor_args* args);

int atacom_soft_alpha_step(const atacom_soft_alpha_args* args);

#ifdef __cplusplus
}
#endif
#endif
