// Row N4: rigid-body dynamics of the iiwa + striker chain (nine movable joints of the reference's urdf/iiwa_1.urdf),
// one evaluation per lane, everything in registers.
//
// What it replaces in the reference (iiwa "7H", torque control):
//   * acc_to_ctrl_action            atacom/environments/iiwa_air_hockey/iiwa_hit_atacom.py:58-63
//                                   PyBullet calculateInverseDynamics(q, dq, ddq padded with zeros)[:6]
//   * the physics sub-step          PyBullet stepSimulation under those torques, URDF joint damping
//                                   (urdf/iiwa_1.urdf:77,115,152,189,226,263,300), joint 7 and the universal joint held by
//                                   position servos (env_base.py:62-70, env_single.py:137-185)
// Bullet is a third-party dependency that is neither vendored nor installed, so this is the model of this build
// (DESIGN.md section 4a), identical in oracle/dynamics.py, whose inverse dynamics and mass matrix are pinned to the
// reference's URDF file (golden set G11).  The constants come from atacom_iiwa_inertia.h (generated from that URDF).
//
// What the kernels evaluate per physics sub-step (rigid_body_substep, atacom_kernels.h): the bias h = C(q, dq) dq + g(q) by
// recursive Newton-Euler, the mass-matrix rows of the controlled joints with their coupling to the servo joints, and the
// world axes behind the servo set-points -- all in link coordinates (atacom_dynamics_link.h) -- then, below, the servo
// set-points and the Cholesky solve of the controlled joints' 6 x 6 block.  oracle/dynamics.py states the same equations
// in world coordinates.
#pragma once
#include "atacom_envs.h"
#include "atacom_iiwa_inertia.h"
#include "atacom_dynamics_link.h"

namespace atacom {

// x = A^-1 b for the symmetric positive definite A given by its lower triangle (overwritten by its Cholesky factor)
// (A may carry NR - NB further rows below the block: they are not touched)
template <typename T, int NB, int NR = NB>
__device__ __forceinline__ void chol_solve(T (&A)[NR][NB], T (&b)[NB]) {
    T inv[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        T d = A[j][j];
#pragma unroll
        for (int k2 = 0; k2 < j; ++k2) d = num<T>::fma(-A[j][k2], A[j][k2], d);
        const T l = num<T>::sqrt(d);
        inv[j] = num<T>::rcp(l);
        A[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < NB; ++i) {
            T v = A[i][j];
#pragma unroll
            for (int k2 = 0; k2 < j; ++k2) v = num<T>::fma(-A[i][k2], A[j][k2], v);
            A[i][j] = v * inv[j];
        }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {                          // L y = b
        T v = b[i];
#pragma unroll
        for (int k2 = 0; k2 < i; ++k2) v = num<T>::fma(-A[i][k2], b[k2], v);
        b[i] = v * inv[i];
    }
#pragma unroll
    for (int i = NB - 1; i >= 0; --i) {                     // L^T x = y
        T v = b[i];
#pragma unroll
        for (int k2 = i + 1; k2 < NB; ++k2) v = num<T>::fma(-A[k2][i], b[k2], v);
        b[i] = v * inv[i];
    }
}

// ---- servo set-points (env_single.py:137-185) from the arm's forward kinematics
// joint 7: the angle that keeps the striker's y axis horizontal, evaluated with joint 7 at zero (env_single.py:139-142)
template <typename T>
__device__ __forceinline__ T joint7_target(const T (&Y)[3], const T (&Z)[3], T q7_cur) {
    // Y, Z: the y and z axes of link_7 with joint 7 AT ZERO.  They come from the chain the dynamics have just evaluated:
    // joint 7's origin frame maps link_6's (x, y, z) to (-x, z, y) (urdf:295, kind 1 in lk::servo_axes), so at q7 = 0 link_7's
    // y axis is link_6's z axis = the axis of joint 6 (z6) and its z axis is joint 7's own axis (z7) -- no second
    // pass through the seven joint rotations (it had cost seven sincos and ~400 instructions per physics sub-step).
    const T down[3] = {T(0), T(0), T(-1)};
    T yd[3];
    lk::crossv(down, Z, yd);                                                      // :144
    const T nrm = num<T>::sqrt(num<T>::fma(yd[0], yd[0], num<T>::fma(yd[1], yd[1], yd[2] * yd[2])));
    const bool big = nrm > T(1e-2);
    const T inrm = big ? num<T>::rcp(nrm) : T(1);
#pragma unroll
    for (int d = 0; d < 3; ++d) yd[d] = big ? yd[d] * inrm : Z[d];                // :146-150
    T dot = num<T>::fma(Y[0], yd[0], num<T>::fma(Y[1], yd[1], Y[2] * yd[2]));
    dot = num<T>::min(num<T>::max(dot, T(-1)), T(1));
    T target = num<T>::acos(dot);                                                 // :152
    T ax[3];
    lk::crossv(Y, yd, ax);
    const T an = num<T>::sqrt(num<T>::fma(ax[0], ax[0], num<T>::fma(ax[1], ax[1], ax[2] * ax[2])));
    const bool abig = an > T(1e-2);
    const T ian = abig ? num<T>::rcp(an) : T(1);
    const T sgn = abig ? (ax[0] * Z[0] + ax[1] * Z[1] + ax[2] * Z[2]) * ian : Z[2];   // axis . z, axis = (0,0,1) fallback
    target *= sgn;                                                                // :161
    const T pi = T(3.14159265358979323846);
    if constexpr (std::is_same<T, double>::value) {
        // :163-166 as selects in the float64 kernels (at the register ceiling): a branch here is one more region at whose
        // join hipcc 7.2 can place the register allocator's copies under the narrowed exec mask (num<double>::acos,
        // atacom_linalg.h: with acos branch-free the copies of `target` moved to this join in the quad T-step kernel).  The
        // float32 kernels keep the text they were measured with.
        const T off = target - q7_cur;
        const T shift = (off > pi / 2) ? -pi : ((off < -pi / 2) ? pi : T(0));
        return target + shift;
    }
    if (target - q7_cur > pi / 2) target -= pi;                                   // :163-166
    else if (target - q7_cur < -pi / 2) target += pi;
    return target;
}

// universal joint: tilt of link_7's z axis against the table normal, signed by its y axis (env_single.py:169-185)
template <typename T>
__device__ __forceinline__ T universal_target(const T (&z7)[3], const T (&y7)[3]) {
    const T dot = num<T>::min(num<T>::max(-z7[2], T(-1)), T(1));
    const T q1 = num<T>::acos(dot);
    const T down[3] = {T(0), T(0), T(-1)};
    T ax[3];
    lk::crossv(z7, down, ax);
    const T an = num<T>::sqrt(num<T>::fma(ax[0], ax[0], num<T>::fma(ax[1], ax[1], ax[2] * ax[2])));
    const bool abig = an > T(1e-2);
    const T ian = abig ? num<T>::rcp(an) : T(1);
    const T sgn = abig ? (ax[0] * y7[0] + ax[1] * y7[1] + ax[2] * y7[2]) * ian : y7[2];
    return q1 * sgn;
}

}  // namespace atacom
