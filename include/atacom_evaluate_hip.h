/* libatacom_evaluate.so -- the network evaluation of an on-policy iteration, on the device and in one launch: a critic or an
 * actor of the project's architecture (Linear(n_in, 64) - act - Linear(64, 64) - act - Linear(64, n_out), atacom_hip.h:
 * atacom_mlp) over every row of a finished collection, optionally with the log-probability of the recorded actions under the
 * diagonal Gaussian around the network's mean.  Plain C11.  The seventh library of the project; like libatacom_returns.so it
 * has no handle, keeps no state, belongs to no environment and reads the records of any of them where they lie.
 *
 * Conventions of atacom_hip.h: every pointer of the network or held by a view is DEVICE memory owned by the caller; all work is
 * enqueued on `stream` (a hipStream_t passed as void*, NULL = the null stream) of device `device`; return codes are 0 or
 * negative (ATACOM_EVALUATE_E_*), atacom_evaluate_last_error() gives the message of the calling thread's last failure.
 * Argument validation happens before any device call.  Nothing synchronises and nothing is allocated: a call can be captured
 * in a HIP graph. */
#ifndef ATACOM_EVALUATE_HIP_H
#define ATACOM_EVALUATE_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "atacom_hip.h" /* atacom_mlp, ATACOM_MLP_SIZE_V1 */

#ifdef __cplusplus
extern "C" {
#endif

#define ATACOM_EVALUATE_F32 0
#define ATACOM_EVALUATE_F64 1

#define ATACOM_EVALUATE_OK 0
#define ATACOM_EVALUATE_E_INVALID (-1)     /* bad argument */
#define ATACOM_EVALUATE_E_HIP (-2)         /* a HIP runtime call failed */
#define ATACOM_EVALUATE_E_UNSUPPORTED (-3) /* no kernel for the dtype or the network, or a grid the launch cannot express */

#define ATACOM_EVALUATE_MAX_IN 32
#define ATACOM_EVALUATE_MAX_OUT 8
#define ATACOM_EVALUATE_HIDDEN 64
#define ATACOM_EVALUATE_MAX_BLOCKS 65535
#define ATACOM_EVALUATE_MAX_ROWS 2147483647 /* n_outer * n_inner of one call */

/* The rows of one array, addressed where they lie: row (o, i), o < n_outer, i < n_inner (both sizes are the call's), starts at
 * ptr[o * stride_outer + i * stride_inner], strides in ELEMENTS; the elements of a row are contiguous.  This names a contiguous
 * [R, n] array (n_outer = 1, stride_inner = n), the obs columns of [T, B, F] records in place (ptr = records + offset of obs,
 * stride_outer = batch_stride * F, stride_inner = F) and a column of one number per row alike.  A stride of a dimension of
 * size 1 is not read.  Strides of an output are at least the row's width; an input may also repeat rows (stride 0). */
typedef struct atacom_evaluate_view {
    void* ptr;
    int64_t stride_outer, stride_inner;
} atacom_evaluate_view;

typedef struct atacom_evaluate_args {
    uint32_t struct_size; /* = sizeof(atacom_evaluate_args) */
    int32_t device;       /* HIP device index of every pointer of the call */
    int32_t dtype;        /* ATACOM_EVALUATE_F32 / ATACOM_EVALUATE_F64: the network, the rows and the outputs */
    int32_t n_blocks;     /* workgroups of the launch, each looping over row tiles; 0 = the library chooses */
    int64_t n_outer, n_inner; /* both >= 1; n_outer * n_inner rows, at most ATACOM_EVALUATE_MAX_ROWS */
    atacom_mlp net;       /* hidden = 64, 1 <= n_in <= 32, 1 <= n_out <= 8; struct_size its own or ATACOM_MLP_SIZE_V1.  Of the
                             exploration fields only std is read (by logp); a sigma network, squash, mean_mode and explore are
                             refused */
    atacom_evaluate_view x;      /* rows of n_in: the network's input */
    atacom_evaluate_view action; /* rows of n_out: the recorded actions; ptr NULL unless logp is asked for */
    atacom_evaluate_view y;      /* OUT rows of n_out: the network's output; ptr NULL = not wanted */
    atacom_evaluate_view logp;   /* OUT rows of 1: the log-probability; ptr NULL = not wanted; needs action and net.std */
    void* stream;
} atacom_evaluate_args;

const char* atacom_evaluate_version(void);
const char* atacom_evaluate_last_error(void);

/* For every row r:
 *     y[r]    = W3 act(W2 act(W1 ((x[r] - obs_shift) * obs_scale) + b1) + b2) + b3
 *     logp[r] = sum_k (-z_k^2 / 2 - log std_k) - n_out log(2 pi) / 2,   z = (action[r] - y[r]) / std
 * the latter being torch.distributions.MultivariateNormal(y, diag(std^2)).log_prob(action), the policy of MushroomRL's
 * GaussianTorchPolicy.  At least one of y and logp is requested; with both, one pass writes both, and each holds the bits the
 * call with it alone writes.
 *
 * Float32 runs the three layers on the matrix cores (v_mfma_f32_16x16x4_f32, one wavefront = 64 rows), float64 on the vector
 * unit with four lanes per row.  The weights are staged in LDS once per workgroup, which then walks the row tiles
 * b, b + n_blocks, ...  The result of a row does not depend on n_blocks, on the strides or on the row's position.
 * logp is formed as  fma(-1/2, sum_k z_k^2, c)  with the sum accumulated by fused multiply-adds in the order of k from 0, the
 * division IEEE, and c = -(sum_k log std_k) - n_out log(2 pi) / 2 computed in double and rounded once to the dtype.
 *
 * The outputs must not overlap x, action or each other (their byte extents are compared); rows outside the views and the
 * padding between rows are neither read nor written. */
int atacom_evaluate_mlp(const atacom_evaluate_args* args);

#ifdef __cplusplus
}
#endif
#endif
