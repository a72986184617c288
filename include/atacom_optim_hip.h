/* libatacom_optim.so -- the optimiser step of an on-policy update, on the device and in one launch: torch's default Adam (no
 * amsgrad, no weight decay, not maximising) applied to one to four parameter groups, each one network of the project's
 * architecture (Linear(n_in, 64) - act - Linear(64, 64) - act - Linear(64, n_out)) and optionally the log std of its Gaussian,
 * with the step count and the running powers of the betas in DEVICE memory, so that the step after the gradients of
 * libatacom_fit.so can be captured in a HIP graph with them.  Plain C11.  The ninth library of the project; it has no handle
 * and belongs to no environment.
 *
 * Conventions of atacom_fit_hip.h: every pointer of a group is DEVICE memory owned by the caller; all work is enqueued on
 * `stream` (a hipStream_t passed as void*, NULL = the null stream) of device `device`; return codes are 0 or negative
 * (ATACOM_OPTIM_E_*), atacom_optim_last_error() gives the message of the calling thread's last failure.  Argument validation
 * happens before any device call.  Nothing synchronises and nothing is allocated -- the caller brings the state -- so a call
 * can be captured in a HIP graph. */
#ifndef ATACOM_OPTIM_HIP_H
#define ATACOM_OPTIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ATACOM_OPTIM_F32 0
#define ATACOM_OPTIM_F64 1

#define ATACOM_OPTIM_OK 0
#define ATACOM_OPTIM_E_INVALID (-1)     /* bad argument */
#define ATACOM_OPTIM_E_HIP (-2)         /* a HIP runtime call failed */
#define ATACOM_OPTIM_E_UNSUPPORTED (-3) /* no kernel for the dtype or the network */

#define ATACOM_OPTIM_MAX_GROUPS 4
#define ATACOM_OPTIM_MAX_IN 32
#define ATACOM_OPTIM_MAX_OUT 8
#define ATACOM_OPTIM_HIDDEN 64
#define ATACOM_OPTIM_HEAD 32 /* bytes of a state's head */

/* One parameter group: a network, optionally its log std.  N = 64 n_in + 64 + 4096 + 64 + 64 n_out + n_out values, and n_out
 * more with log_std. */
typedef struct atacom_optim_group {
    int32_t n_in;  /* 1 .. 32 */
    int32_t n_out; /* 1 .. 8 */
    void* W1;      /* [64, n_in] row-major, updated in place -- as are the five that follow */
    void* b1;      /* [64] */
    void* W2;      /* [64, 64] */
    void* b2;      /* [64] */
    void* W3;      /* [n_out, 64] */
    void* b3;      /* [n_out] */
    void* log_std; /* [n_out], updated in place; NULL = the group has none */
    void* std;     /* OUT [n_out] = exp(log_std) after the update; NULL = not wanted; only with log_std */
    const void* grad; /* N contiguous values in the order of atacom_fit_gradient's grad: dW1, db1, dW2, db2, dW3, db3, then
                         d log std when the group has log_std.  Read, never written */
    void* state;   /* atacom_optim_state_size() bytes, 8-byte aligned (below) */
    double lr;         /* >= 0, finite */
    double grad_scale; /* finite: the gradient is multiplied by it first (0.5 for the value loss of  policy + 0.5 value) */
} atacom_optim_group;

typedef struct atacom_optim_args {
    uint32_t struct_size; /* = sizeof(atacom_optim_args) */
    int32_t device;       /* HIP device index of every pointer of the call */
    int32_t dtype;        /* ATACOM_OPTIM_F32 / ATACOM_OPTIM_F64: parameters, gradients, moments and std */
    int32_t n_groups;     /* 1 .. ATACOM_OPTIM_MAX_GROUPS; groups[n_groups ..] are not read */
    double beta1, beta2;  /* in [0, 1) */
    double eps;           /* > 0, finite */
    void* stream;
    atacom_optim_group groups[ATACOM_OPTIM_MAX_GROUPS];
} atacom_optim_args;

const char* atacom_optim_version(void);
const char* atacom_optim_last_error(void);

/* The state of a group: a head of ATACOM_OPTIM_HEAD = 32 bytes
 *     int64 step;  double beta1_pow;  double beta2_pow;  8 reserved bytes
 * followed by the first moments m[N] and the second moments v[N] in the dtype, both in the order of grad.  This returns
 * 32 + 2 N sizeof(dtype), or 0 for a dtype, n_in or n_out that a step would refuse (atacom_optim_last_error() says why).  It
 * touches no device. */
size_t atacom_optim_state_size(int32_t dtype, int32_t n_in, int32_t n_out, int32_t has_log_std);

/* Enqueue the work that makes the state of every group of `args` a fresh one: step = 0, beta1_pow = beta2_pow = 1, the
 * reserved bytes and all moments zero.  It takes the argument struct of the steps that follow and validates all of it as
 * atacom_optim_adam_step does, except that grad may be NULL; it reads and writes nothing but the states. */
int atacom_optim_adam_init(const atacom_optim_args* args);

/* One Adam step of every group, ONE launch.  Per group, with the head read from its state; lines marked (double) are double
 * arithmetic whatever the dtype, every other operation is one individually rounded operation of the dtype (the library is
 * compiled without contraction: there are no fused multiply-adds), sqrt and the divisions are IEEE:
 *
 *     t = step + 1;  b1p = beta1_pow * beta1;  b2p = beta2_pow * beta2                      (double)
 *     step_size = lr / (1 - b1p);  bc2s = sqrt(1 - b2p)                                     (double, each rounded once to the dtype)
 *     omb1 = 1 - beta1;  omb2 = 1 - beta2                                                   (double, each rounded once to the dtype)
 *     beta2, eps and grad_scale are rounded once to the dtype
 *   and for every value of the group
 *     g = grad_scale * grad
 *     m = m + (g - m) * omb1
 *     v = beta2 * v + (omb2 * g) * g
 *     p = p - step_size * (m / (sqrt(v) / bc2s + eps))
 *   and for a group with std, after the update
 *     std = exp(log_std)
 *   and then the head becomes  step = t, beta1_pow = b1p, beta2_pow = b2p.
 *
 * The powers are running products, not pow(): a float64 loop `b1p *= beta1` reproduces them bit for bit, and the step count
 * never visits the host.  This is torch.optim.Adam's single-tensor arithmetic (lerp, addcmul, addcdiv) with beta ** t replaced
 * by the product; in float64 the two agree to a few units of 1e-16 of each value's scale.
 *
 * The launch is k_adam<T>: n_groups workgroups of 1024 threads, one per group.  Thread 0 forms the scalars above and hands
 * them to the others through LDS; the threads walk the group's six or seven segments with a stride of the workgroup; after a
 * barrier thread 0 writes the head.  No workgroup reads another's head: there are no atomics and no ordering between
 * workgroups, and a launch of several groups gives the bits of one launch per group.  A group is at most 6800 values, so the
 * call is bound by the latency of one launch and not by bandwidth.
 *
 * Refused before any device call: the byte extents of the parameters, log_std, std, grad and state of all groups of a call
 * must be pairwise disjoint (two groups that name the same parameter are refused).  grad is only read; nothing outside
 * the named extents is read or written. */
int atacom_optim_adam_step(const atacom_optim_args* args);

#ifdef __cplusplus
}
#endif
#endif
