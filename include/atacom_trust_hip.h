/* libatacom_trust.so -- the product of a policy's Fisher matrix with a vector, on the device and in one launch (plus a small one
 * that adds the workgroups' partial sums): the stage of a trust-region policy update (TRPO) that a conjugate-gradient solve
 * repeats over the whole collection.  The policy is the project's: the mean network Linear(n_in, 64) - act - Linear(64, 64) - act -
 * Linear(64, n_out) (atacom_hip.h: atacom_mlp) with a state-independent std = exp(log_std).  Plain C11.  The tenth library of the
 * project; like libatacom_fit.so it has no handle, keeps no state, belongs to no environment and reads records where they lie.
 *
 * Conventions of atacom_hip.h: every pointer of the network or held by a view is DEVICE memory owned by the caller; all work is
 * enqueued on `stream` (a hipStream_t passed as void*, NULL = the null stream) of device `device`; return codes are 0 or
 * negative (ATACOM_TRUST_E_*), atacom_trust_last_error() gives the message of the calling thread's last failure.  Argument
 * validation happens before any device call.  Nothing synchronises and nothing is allocated -- the caller brings the workspace
 * -- so a call can be captured in a HIP graph. */
#ifndef ATACOM_TRUST_HIP_H
#define ATACOM_TRUST_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "atacom_evaluate_hip.h" /* atacom_evaluate_view; atacom_mlp through atacom_hip.h */

#ifdef __cplusplus
extern "C" {
#endif

#define ATACOM_TRUST_F32 0
#define ATACOM_TRUST_F64 1

#define ATACOM_TRUST_OK 0
#define ATACOM_TRUST_E_INVALID (-1)     /* bad argument */
#define ATACOM_TRUST_E_HIP (-2)         /* a HIP runtime call failed */
#define ATACOM_TRUST_E_UNSUPPORTED (-3) /* no kernel for the dtype or the network, or a grid the launch cannot express */

#define ATACOM_TRUST_MAX_IN 32
#define ATACOM_TRUST_MAX_OUT 8
#define ATACOM_TRUST_HIDDEN 64
#define ATACOM_TRUST_MAX_BLOCKS 65535
#define ATACOM_TRUST_MAX_ROWS 2147483647 /* n_outer * n_inner of one call, and n_idx */

/* Rows are addressed as in atacom_evaluate_hip.h: row (o, i) of a view starts at ptr[o * stride_outer + i * stride_inner],
 * strides in ELEMENTS, the elements of a row contiguous; the flat number of that row is o * n_inner + i. */
typedef struct atacom_trust_args {
    uint32_t struct_size; /* = sizeof(atacom_trust_args) */
    int32_t device;       /* HIP device index of every pointer of the call */
    int32_t dtype;        /* ATACOM_TRUST_F32 / ATACOM_TRUST_F64: the network, the rows, v, out and the workspace */
    int32_t n_blocks;     /* workgroups of the product launch = partial sums; 0 = the library chooses (below) */
    int64_t n_outer, n_inner; /* both >= 1; n_outer * n_inner rows, at most ATACOM_TRUST_MAX_ROWS */
    atacom_mlp net;       /* hidden = 64, 1 <= n_in <= 32, 1 <= n_out <= 8; struct_size its own or ATACOM_MLP_SIZE_V1.  std is
                             required; a sigma network, squash, mean_mode and explore are refused */
    atacom_evaluate_view x; /* rows of n_in: the network's input */
    const int64_t* idx;   /* n_idx flat row numbers in [0, n_outer * n_inner), repeats allowed; NULL = every row once, in order.
                             THE KERNEL DOES NOT GUARD AN INDEX OUT OF RANGE: that they are in range is the caller's contract */
    int64_t n_idx;        /* >= 1 with idx, ignored without.  M = n_idx, or n_outer * n_inner without idx */
    const void* v;        /* P + n_out contiguous values, the direction: V1 [64, n_in], vb1 [64], V2 [64, 64], vb2 [64],
                             V3 [n_out, 64], vb3 [n_out], v_ls [n_out]; every matrix row-major like its weight,
                             P = 64 n_in + 64 + 4096 + 64 + 64 n_out + n_out */
    double damping;       /* >= 0 and finite; rounded once to the dtype */
    void* out;            /* OUT P + n_out values in the order of v: F v + damping v */
    void* workspace;      /* atacom_trust_workspace_size(args) bytes, written and read by the call; aligned to the dtype */
    size_t workspace_bytes;
    void* stream;
} atacom_trust_args;

const char* atacom_trust_version(void);
const char* atacom_trust_last_error(void);

/* The bytes of workspace a call with these dtype, n_blocks, net.n_in, net.n_out, n_outer, n_inner, idx and n_idx needs:
 * n_blocks_effective * P * sizeof(dtype), rounded up to a multiple of 256; 0 for arguments that atacom_trust_fvp would refuse for
 * these fields (atacom_trust_last_error() says why).  It touches no device.  n_blocks_effective is n_blocks when that is not 0,
 * and otherwise  min(ceil(M / R), 512)  with R = 256 rows for float32 (four wavefronts of 64 rows) and 16 for float64: the rule
 * of atacom_fit_workspace_size, of the sizes alone. */
size_t atacom_trust_workspace_size(const atacom_trust_args* args);

/* F is the Hessian at theta' = theta of  mean_r KL(N(mu_theta(x_r), std^2) || N(mu_theta'(x_r), std'^2))  with respect to
 * theta' = (W1, b1, W2, b2, W3, b3, log_std).  The KL's first derivative in mu vanishes there, so F has no second-order network
 * terms and no cross terms between the network and log_std:  F_net = mean_r J_r^T diag(1 / std^2) J_r  with J_r the Jacobian of
 * mu at row r, and F_ls = 2 I.  With r running over the M rows of the call (row idx[r], or r), xn = (x - obs_shift) * obs_scale:
 *     forward:   a1 = W1 xn + b1, h1 = act(a1);  a2 = W2 h1 + b2, h2 = act(a2)
 *     tangent:   t1 = (V1 xn + vb1) * act'(a1)
 *                t2 = (W2 t1 + V2 h1 + vb2) * act'(a2)
 *                ty =  W3 t2 + V3 h2 + vb3                                   (= J_r v)
 *     head:      dy_k = ty_k / (std_k * std_k)            the square rounded, then an IEEE division
 *     backward:  dW3 = sum_r dy_r h2_r^T, db3 = sum_r dy_r, da2 = (W3^T dy) * act'(a2), dW2 = sum_r da2 h1^T, db2 = sum_r da2,
 *                da1 = (W2^T da2) * act'(a1), dW1 = sum_r da1 xn^T, db1 = sum_r da1;  relu' = [a > 0], tanh' = 1 - h^2
 * exactly as atacom_fit_hip.h writes the backward pass.  The row terms are summed unscaled and every sum is divided by M once
 * (an IEEE division).  Then, for every element i of the network part and k of the log-std part, with d = damping rounded to the
 * dtype and every operation rounded on its own (no fused multiply-add):
 *     out_i  = (sum_i / M) + (d * v_i)
 *     out_ls = (2 * v_ls) + (d * v_ls)
 * Away from the kinks of relu this is what two torch.autograd.grad calls through kl_divergence(old, new).mean() give, plus
 * damping * v.
 *
 * Two launches.  k_trust_fvp: a workgroup stages the weights AND the network part of v in LDS once (two blocks of the layout of
 * atacom_policy.h, 31008 bytes each) and walks the row tiles b, b + n_blocks, ...; in float32 a wavefront takes 64 rows at a time
 * as four blocks of 16 and every product of the forward, tangent and backward pass runs on the matrix cores
 * (v_mfma_f32_16x16x4_f32) with the weight-gradient accumulators in registers across the whole walk; the tangent products have
 * the shape of the forward ones, so t1 and t2 come out in the register layout of h1 and h2.  LDS of a float32 workgroup: 2 x
 * 31008 + 32 + 4 x 8192 (two [16][64] transposition buffers a wavefront) = 94816 bytes.  In float64 a workgroup takes 16 rows at
 * a time on the vector unit, one LDS record of 393 + 4 ceil(n_in / 4) doubles a row, and every thread owns a fixed set of entries,
 * which it accumulates by fused multiply-adds in row order.  The workgroup writes ONE partial of P values to workspace[b].
 * k_trust_reduce adds the partials in a fixed order (eight interleaved sums, over b = s, s + 8, ... each, then added in the order
 * of s), divides by M and applies the two lines above.  There are no atomics: repeating a call with the same
 * n_blocks_effective gives the same bits; calls with different n_blocks may differ in rounding.
 *
 * out and workspace must not overlap x, v, idx or each other (their byte extents are compared); rows outside the view, rows
 * that idx does not name and the padding between rows are neither read nor written. */
int atacom_trust_fvp(const atacom_trust_args* args);

#ifdef __cplusplus
}
#endif
#endif
