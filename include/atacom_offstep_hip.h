/* libatacom_offstep.so -- the optimiser step of an off-policy update (DDPG, TD3, SAC) on the device and in one launch: torch's
 * default Adam (no amsgrad, no weight decay, not maximising) applied to one to four parameter groups, each one network of the
 * project's architecture (Linear(n_in, 64) - act - Linear(64, 64) - act - Linear(64, n_out)) or one two-branch critic (the same
 * with W2a [64, n_act], the action's second entry), and in the SAME launch the soft update of the group's target network from
 * the values just written.  The step count and the running powers of the betas live in DEVICE memory, so a whole fit -- TD
 * target, gradients, step, targets -- can be captured in a HIP graph.  Plain C11.  The fourteenth library of the project; it has
 * no handle and belongs to no environment.
 *
 * Conventions of atacom_optim_hip.h: every pointer of a group is DEVICE memory owned by the caller; all work is enqueued on
 * `stream` (a hipStream_t passed as void*, NULL = the null stream) of device `device`; return codes are 0 or negative
 * (ATACOM_OFFSTEP_E_*), atacom_offstep_last_error() gives the message of the calling thread's last failure.  Argument
 * validation happens before any device call.  Nothing synchronises and nothing is allocated -- the caller brings the state --
 * so a call can be captured in a HIP graph. */
#ifndef ATACOM_OFFSTEP_HIP_H
#define ATACOM_OFFSTEP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ATACOM_OFFSTEP_F32 0
#define ATACOM_OFFSTEP_F64 1

#define ATACOM_OFFSTEP_OK 0
#define ATACOM_OFFSTEP_E_INVALID (-1) /* bad argument */
#define ATACOM_OFFSTEP_E_HIP (-2)     /* a HIP runtime call failed */

#define ATACOM_OFFSTEP_MAX_GROUPS 4
#define ATACOM_OFFSTEP_MAX_IN 32
#define ATACOM_OFFSTEP_MAX_OUT 8
#define ATACOM_OFFSTEP_MAX_ACT 8
#define ATACOM_OFFSTEP_HIDDEN 64
#define ATACOM_OFFSTEP_TENSORS 7
#define ATACOM_OFFSTEP_HEAD 32 /* bytes of a state's head */

/* One parameter group: a network and, optionally, the target network that follows it.
 * N = 64 n_in + 64 + 4096 + 64 + 64 n_out + n_out + 64 n_act values. */
typedef struct atacom_offstep_group {
    int32_t n_in;  /* 1 .. 32: the inputs of the first layer (a TD3 critic: observation + action elements) */
    int32_t n_out; /* 1 .. 8 */
    int32_t n_act; /* 0 .. 8: the columns of W2a; 0 = a plain network without W2a */
    int32_t reserved;
    void* W1;  /* [64, n_in] row-major, updated in place -- as are the six that follow */
    void* b1;  /* [64] */
    void* W2;  /* [64, 64] */
    void* b2;  /* [64] */
    void* W3;  /* [n_out, 64] */
    void* b3;  /* [n_out] */
    void* W2a; /* [64, n_act]; not read when n_act = 0 */
    void* target[ATACOM_OFFSTEP_TENSORS]; /* the target network's tensors in the same order and shapes, updated in place: all
                                             NULL (the group has no target) or all set (target[6] is not read when n_act = 0) */
    const void* grad; /* N contiguous values: dW1, db1, dW2, db2, dW3, db3, dW2a -- the order of atacom_offgrad_critic_gradient's
                         grad and, for n_act = 0, of atacom_fit_gradient's.  Read, never written.  NULL = the group is not
                         stepped in this call: only its target follows */
    void* state;      /* atacom_offstep_state_size() bytes, 8-byte aligned (below) */
    double lr;         /* >= 0, finite */
    double grad_scale; /* finite: the gradient is multiplied by it first */
} atacom_offstep_group;

typedef struct atacom_offstep_args {
    uint32_t struct_size; /* = sizeof(atacom_offstep_args) */
    int32_t device;       /* HIP device index of every pointer of the call */
    int32_t dtype;        /* ATACOM_OFFSTEP_F32 / ATACOM_OFFSTEP_F64: parameters, targets, gradients and moments */
    int32_t n_groups;     /* 1 .. ATACOM_OFFSTEP_MAX_GROUPS; groups[n_groups ..] are not read */
    double beta1, beta2;  /* in [0, 1) */
    double eps;           /* > 0, finite */
    double tau;           /* in [0, 1]: the share of the online value in a target's update */
    void* stream;
    atacom_offstep_group groups[ATACOM_OFFSTEP_MAX_GROUPS];
} atacom_offstep_args;

const char* atacom_offstep_version(void);
const char* atacom_offstep_last_error(void);

/* The state of a group has the layout of atacom_optim_hip.h: a head of ATACOM_OFFSTEP_HEAD = 32 bytes
 *     int64 step;  double beta1_pow;  double beta2_pow;  8 reserved bytes
 * followed by the first moments m[N] and the second moments v[N] in the dtype, both in the order of grad.  This returns
 * 32 + 2 N sizeof(dtype), or 0 for a dtype, n_in, n_out or n_act that a step would refuse (atacom_offstep_last_error() says
 * why).  It touches no device. */
size_t atacom_offstep_state_size(int32_t dtype, int32_t n_in, int32_t n_out, int32_t n_act);

/* Enqueue the work that makes the state of every group of `args` a fresh one: step = 0, beta1_pow = beta2_pow = 1, the
 * reserved bytes and all moments zero.  It takes the argument struct of the steps that follow and validates all of it as
 * atacom_offstep_adam_step does; it reads and writes nothing but the states. */
int atacom_offstep_adam_init(const atacom_offstep_args* args);

/* One step of every group, ONE launch.  Lines marked (double) are double arithmetic whatever the dtype, every other operation
 * is one individually rounded operation of the dtype (the library is compiled without contraction: there are no fused
 * multiply-adds), sqrt and the divisions are IEEE.  Per group:
 *
 * 1. With grad: the step of atacom_optim_hip.h, with the head read from the group's state,
 *     t = step + 1;  b1p = beta1_pow * beta1;  b2p = beta2_pow * beta2                      (double)
 *     step_size = lr / (1 - b1p);  bc2s = sqrt(1 - b2p)                                     (double, each rounded once to the dtype)
 *     omb1 = 1 - beta1;  omb2 = 1 - beta2                                                   (double, each rounded once to the dtype)
 *     beta2, eps and grad_scale are rounded once to the dtype
 *   and for every value of the group
 *     g = grad_scale * grad
 *     m = m + (g - m) * omb1
 *     v = beta2 * v + (omb2 * g) * g
 *     p = p - step_size * (m / (sqrt(v) / bc2s + eps))
 *   and then the head becomes  step = t, beta1_pow = b1p, beta2_pow = b2p.
 * 2. Without grad (NULL) the group is not stepped: p, m, v and the head keep their bits; m, v and the head are not touched.
 * 3. With a target, every value of it then follows the p just written -- the unchanged p of a group that was not stepped --
 *    by atacom_offpolicy_soft_update's arithmetic, with a = (T) tau and b = (T)(1.0 - tau), the subtraction in double:
 *     target = fl(fl(a * p) + fl(b * target))
 *    p is the value the thread holds in a register; it is not read back from memory.
 *
 * There is no log std and no std in this library -- the networks of DDPG, TD3 and SAC have none -- and no exp in its kernel.
 * For a plain group with grad the bits of p, m, v and the head are those of atacom_optim_adam_step; the bits of the target are
 * those of atacom_offpolicy_soft_update called after it.
 *
 * The launch is k_adam_track<T>: n_groups workgroups of 1024 threads, one per group.  Thread 0 forms the scalars above and
 * hands them to the others through LDS; the threads walk the group's segments with a stride of the workgroup, loading grad, m,
 * v, p and target together; after a barrier thread 0 writes the head.  No workgroup reads what another writes: there are no
 * atomics and no ordering between workgroups, and a launch of several groups gives the bits of one launch per group.  A group
 * is at most 7304 values, so the call is bound by the latency of one launch and not by bandwidth.
 *
 * Refused before any device call (ATACOM_OFFSTEP_E_INVALID, with a message): a wrong struct_size; a dtype, n_groups, n_in,
 * n_out or n_act out of range; lr negative or not finite; grad_scale not finite; tau outside [0, 1]; a beta outside [0, 1);
 * eps <= 0 or not finite; a target that is partly set; a state that is not aligned to 8 bytes or a tensor that is not aligned
 * to the dtype; and any overlap of byte extents: parameters, targets and states with anything of the call, grad with anything
 * that is written (two groups may read one gradient).  Nothing outside the named extents is read or written. */
int atacom_offstep_adam_step(const atacom_offstep_args* args);

#ifdef __cplusplus
}
#endif
#endif
