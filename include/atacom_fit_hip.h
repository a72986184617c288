/* libatacom_fit.so -- the gradient of an on-policy update, on the device and in one launch per network (plus a small one that
 * adds the workgroups' partial sums): the mean-squared-error loss of a critic, or PPO's clipped surrogate of an actor with a
 * state-independent Gaussian, differentiated by hand through the project's architecture (Linear(n_in, 64) - act -
 * Linear(64, 64) - act - Linear(64, n_out), atacom_hip.h: atacom_mlp) over the rows of a finished collection, optionally
 * gathered through a list of row numbers (a minibatch).  Plain C11.  The eighth library of the project; like
 * libatacom_evaluate.so it has no handle, keeps no state, belongs to no environment and reads records where they lie.
 *
 * Conventions of atacom_hip.h: every pointer of the network or held by a view is DEVICE memory owned by the caller; all work is
 * enqueued on `stream` (a hipStream_t passed as void*, NULL = the null stream) of device `device`; return codes are 0 or
 * negative (ATACOM_FIT_E_*), atacom_fit_last_error() gives the message of the calling thread's last failure.  Argument
 * validation happens before any device call.  Nothing synchronises and nothing is allocated -- the caller brings the workspace
 * -- so a call can be captured in a HIP graph. */
#ifndef ATACOM_FIT_HIP_H
#define ATACOM_FIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "atacom_evaluate_hip.h" /* atacom_evaluate_view; atacom_mlp through atacom_hip.h */

#ifdef __cplusplus
extern "C" {
#endif

#define ATACOM_FIT_F32 0
#define ATACOM_FIT_F64 1

#define ATACOM_FIT_OK 0
#define ATACOM_FIT_E_INVALID (-1)     /* bad argument */
#define ATACOM_FIT_E_HIP (-2)         /* a HIP runtime call failed */
#define ATACOM_FIT_E_UNSUPPORTED (-3) /* no kernel for the dtype or the network, or a grid the launch cannot express */

#define ATACOM_FIT_VALUE 0    /* L = mean (y - target)^2 of a one-output network */
#define ATACOM_FIT_PPO_CLIP 1 /* L = -mean min(rho A, clamp(rho, 1 - clip, 1 + clip) A) */

#define ATACOM_FIT_MAX_IN 32
#define ATACOM_FIT_MAX_OUT 8
#define ATACOM_FIT_HIDDEN 64
#define ATACOM_FIT_MAX_BLOCKS 65535
#define ATACOM_FIT_MAX_ROWS 2147483647 /* n_outer * n_inner of one call, and n_idx */
#define ATACOM_FIT_STATS 4

/* Rows are addressed as in atacom_evaluate_hip.h: row (o, i) of a view starts at ptr[o * stride_outer + i * stride_inner],
 * strides in ELEMENTS, the elements of a row contiguous; the flat number of that row is o * n_inner + i. */
typedef struct atacom_fit_args {
    uint32_t struct_size; /* = sizeof(atacom_fit_args) */
    int32_t device;       /* HIP device index of every pointer of the call */
    int32_t dtype;        /* ATACOM_FIT_F32 / ATACOM_FIT_F64: the network, the rows, the outputs and the workspace */
    int32_t n_blocks;     /* workgroups of the gradient launch = partial sums; 0 = the library chooses (below) */
    int32_t head;         /* ATACOM_FIT_VALUE / ATACOM_FIT_PPO_CLIP */
    int32_t reserved;     /* 0 */
    int64_t n_outer, n_inner; /* both >= 1; n_outer * n_inner rows, at most ATACOM_FIT_MAX_ROWS */
    atacom_mlp net;       /* hidden = 64, 1 <= n_in <= 32, 1 <= n_out <= 8 (VALUE: n_out = 1); struct_size its own or
                             ATACOM_MLP_SIZE_V1.  Of the exploration fields only std is read (PPO_CLIP, required there); a
                             sigma network, squash, mean_mode and explore are refused */
    atacom_evaluate_view x;        /* rows of n_in: the network's input */
    atacom_evaluate_view action;   /* rows of n_out: the recorded actions; PPO_CLIP only */
    atacom_evaluate_view weight;   /* rows of 1: VALUE the regression target t, PPO_CLIP the advantage A */
    atacom_evaluate_view logp_old; /* rows of 1: the log-probability at collection time; PPO_CLIP only */
    const int64_t* idx;   /* n_idx flat row numbers in [0, n_outer * n_inner), repeats allowed; NULL = every row once, in order.
                             THE KERNEL DOES NOT GUARD AN INDEX OUT OF RANGE: that they are in range is the caller's contract */
    int64_t n_idx;        /* >= 1 with idx, ignored without.  M = n_idx, or n_outer * n_inner without idx */
    double clip;          /* > 0; PPO_CLIP only */
    void* grad;           /* OUT P contiguous values: dW1 [64, n_in], db1 [64], dW2 [64, 64], db2 [64], dW3 [n_out, 64],
                             db3 [n_out], every matrix row-major like its weight, P = 64 n_in + 64 + 4096 + 64 + 64 n_out +
                             n_out; PPO_CLIP: n_out more, d L / d log std */
    void* stats;          /* OUT 4 values: L, the share of rows whose ratio term is inactive, mean(logp_old - logp), 0;
                             VALUE: L, 0, 0, 0 */
    void* workspace;      /* atacom_fit_workspace_size(args) bytes, written and read by the call; aligned to the dtype */
    size_t workspace_bytes;
    void* stream;
} atacom_fit_args;

const char* atacom_fit_version(void);
const char* atacom_fit_last_error(void);

/* The bytes of workspace a call with these dtype, n_blocks, net.n_in, net.n_out, n_outer, n_inner, idx and n_idx needs:
 * n_blocks_effective * (P + n_out + ATACOM_FIT_STATS) * sizeof(dtype), rounded up to a multiple of 256; 0 for arguments that
 * atacom_fit_gradient would refuse for these fields (atacom_fit_last_error() says why).  It touches no device.
 * n_blocks_effective is n_blocks when that is not 0, and otherwise  min(ceil(M / R), 512)  with R = 256 rows for float32 (four
 * wavefronts of 64 rows) and 16 for float64: a rule of the sizes alone, so that a workspace sized once fits every call of those
 * sizes on every device. */
size_t atacom_fit_workspace_size(const atacom_fit_args* args);

/* With r running over the M rows of the call (row idx[r], or r), xn = (x - obs_shift) * obs_scale and
 *     a1 = W1 xn + b1,  h1 = act(a1),  a2 = W2 h1 + b2,  h2 = act(a2),  y = W3 h2 + b3
 * VALUE:     L = (1 / M) sum_r (y_r - t_r)^2,                       dy_r = 2 (y_r - t_r)
 * PPO_CLIP:  z = (action - y) / std,  logp = fma(-1/2, sum_k z_k^2, c)  exactly as atacom_evaluate_hip.h forms it,
 *            rho = exp(logp - logp_old),  lo = 1 - clip and hi = 1 + clip formed in double and rounded once to the dtype;
 *            a row is INACTIVE iff (A > 0 and rho > hi) or (A < 0 and rho < lo);
 *            L = -(1 / M) sum_r min(rho A, min(max(rho, lo), hi) A);
 *            g_r = -rho_r A_r for an active row and 0 for an inactive one,
 *            dy_rk = g_r z_rk / std_k,   d L / d log std_k = (1 / M) sum_r g_r (z_rk^2 - 1)
 * backward:  dW3 = sum_r dy_r h2_r^T, db3 = sum_r dy_r, da2 = (W3^T dy) * act'(a2), dW2 = sum_r da2 h1^T, db2 = sum_r da2,
 *            da1 = (W2^T da2) * act'(a1), dW1 = sum_r da1 xn^T, db1 = sum_r da1;  relu' = [a > 0], tanh' = 1 - h^2.
 * The row terms are summed unscaled; every sum is divided by M once, at the end (an IEEE division).  obs_shift, obs_scale and
 * std are constants: no gradient with respect to them is formed other than d L / d log std.  This is the gradient autograd
 * gives for  -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean()  and  (v - ret).pow(2).mean()  away from
 * the kinks of relu and of the clamp.  stats[2] averages logp_old - logp, the usual estimate of the KL divergence.
 *
 * Two launches.  k_fit_gradient: a workgroup stages the weights in LDS once and walks the row tiles b, b + n_blocks, ...; in
 * float32 a wavefront takes 64 rows at a time as four blocks of 16, and the forward pass, the two data-gradient products and the
 * three weight-gradient products run on the matrix cores (v_mfma_f32_16x16x4_f32) with the weight-gradient accumulators in
 * registers across the whole walk; in float64 a workgroup takes 16 rows at a time on the vector unit and every thread owns a
 * fixed set of gradient entries, which it accumulates by fused multiply-adds in row order.  Activations live in registers and
 * LDS: nothing per row is written to memory.  The workgroup's wavefronts add their sums in wave order and the workgroup writes
 * ONE partial of P + n_out + 4 values to workspace[b].  k_fit_reduce adds the partials in a fixed order (eight interleaved sums, over
 * b = s, s + 8, ... each, then added in the order of s), divides by M and writes grad and stats.  There are no atomics: repeating a call with the same n_blocks_effective gives the same bits; calls
 * with different n_blocks may differ in rounding.
 *
 * grad, stats and workspace must not overlap x, action, weight, logp_old, idx or each other (their byte extents are
 * compared); rows outside the views, rows that idx does not name and the padding between rows are neither read nor written. */
int atacom_fit_gradient(const atacom_fit_args* args);

#ifdef __cplusplus
}
#endif
#endif
