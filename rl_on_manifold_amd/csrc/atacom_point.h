// Kernels of the collision-avoidance task (the reference's PointReachAtacom), templated on the scalar type and the
// number of obstacles N in {2, 4}.  They live in their own library, libatacom_point.so (include/atacom_point_hip.h):
// the task shares no state layout, sub-stepping, puck, dynamics or chart mode with the air-hockey handle.
//
//   atacom/environments/collision_avoidance/collision_avoidance_base.py    PointGoalReach      (cited as base:LINE)
//   atacom/environments/collision_avoidance/collision_avoidance_atacom.py  PointReachAtacom    (cited as atacom:LINE)
//
// Specification: tests/point_reach_oracle.py (PointReachBatched), which restates the two files with their quirks.
//
// Mapping: ONE ENVIRONMENT PER LANE.  The whole step lives in registers: J_c = [J_q | diag(s)] is N x (N + 2), one
// bidiag_solve_null<T, N, N + 2> gives the pseudo-inverse solve and the 2-column null basis, rref_apply the chart
// (atacom_linalg.h -- the solver is shared with the main library, not copied).  The float32 kernels use no scratch
// memory and no LDS (the statistics reduction apart).
//
// Memory.  The persistent state is kept in groups of four fields, [group][env][4] (the layout of atacom_kernels.h:
// every access of a wave is one contiguous 1 KB segment of dwordx4).  The T-step kernel writes two rows of
// 4 (1 + N) values per environment and step; a lane owns a row, which is 48 or 80 contiguous, 16-byte aligned bytes, and
// writes it with 16-byte stores: the rows of a wave are adjacent, so the wave's 3 or 5 store instructions of one row
// set together cover one contiguous span (3 or 5 KB) completely and the L2 merges them into whole lines.  They must stay
// PLAIN stores for that: the same stores marked non-temporal ran 3.8 x slower at 1 M environments
// (profiles/point_reach.md).  Workgroups of 256: 64 and 128 were 1-5 % slower there.
#pragma once
#include <stdint.h>
#include "../../include/atacom_point_hip.h"
#include "atacom_kernels.h"          // device_uniform (the counter-based generator), num<T>, the solver via atacom_linalg.h

namespace atacom_point {

using atacom::num;

template <typename T>
struct PParams {
    int batch, horizon, auto_reset, random_walk;
    unsigned int seed;
    T dt;
};

// host: the launch parameters of every kernel that takes a handle's configuration, in either library of the task
template <typename T>
static PParams<T> params(const atacom_point_config& c) {
    PParams<T> P;
    P.batch = c.batch; P.horizon = c.horizon; P.auto_reset = c.auto_reset; P.random_walk = c.random_walk;
    P.seed = (unsigned int)c.seed;
    P.dt = (T)c.dt;
    return P;
}

// ------------------------------------------------------------------ persistent state
template <int N>
struct Layout {
    static constexpr int OBS = 4 * (1 + N);                 // [q, dq, (p_i, dp_i) per obstacle]
    static constexpr int S = OBS, CTR = S + N, TIME = CTR + 2 * N, SSUM = TIME + 1, SCMAX = SSUM + 1, COUNT = SCMAX + 1;
    static constexpr int GROUPS = (COUNT + 3) / 4;
    static constexpr int VALUES_PER_ENV = 4 * GROUPS;
    static constexpr int I_T = 0, I_EP = 1, I_HAVE = 2, I_CNT = 3;      // one int4 per environment
    // user-facing row of get_state / set_state: [state, s, centres, time, t, episode, have_centres]
    static constexpr int STATE_DIM = 7 * N + 8;
};

template <typename T>
__device__ __forceinline__ T& pl(T* f, int field, int B, int b) {
    return f[((size_t)(field >> 2) * B + b) * 4 + (field & 3)];
}
template <typename T>
__device__ __forceinline__ const T& pl(const T* f, int field, int B, int b) {
    return f[((size_t)(field >> 2) * B + b) * 4 + (field & 3)];
}

template <typename T, int N>
struct PState {
    // grouped as the memory is (fields that travel in one 16-byte access sit together: a struct in another order had the
    // vectoriser form accesses that straddle members, and the register promotion then gave up on the whole struct)
    T r[4];            // robot: q(2), dq(2)
    T o[N][4];         // obstacle i: p(2), dp(2)
    T s[N], ctr[N][2], time;
    int t, ep, have;
};

template <typename T, int N>
__device__ __forceinline__ void load_state(const T* __restrict__ f, const int* __restrict__ ip, int B, int b,
                                           PState<T, N>& st) {
    using L = Layout<N>;
#pragma unroll
    for (int c = 0; c < 2; ++c) { st.r[c] = pl(f, c, B, b); st.r[2 + c] = pl(f, 2 + c, B, b); }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            st.o[i][c] = pl(f, 4 * (i + 1) + c, B, b);
            st.o[i][2 + c] = pl(f, 4 * (i + 1) + 2 + c, B, b);
            st.ctr[i][c] = pl(f, L::CTR + 2 * i + c, B, b);
        }
#pragma unroll
    for (int i = 0; i < N; ++i) st.s[i] = pl(f, L::S + i, B, b);
    st.time = pl(f, L::TIME, B, b);
    st.t = ip[(size_t)b * 4 + L::I_T];
    st.ep = ip[(size_t)b * 4 + L::I_EP];
    st.have = ip[(size_t)b * 4 + L::I_HAVE];
}

// everything but the statistics (SSUM, SCMAX, I_CNT), which the callers own
template <typename T, int N>
__device__ __forceinline__ void store_state(T* __restrict__ f, int* __restrict__ ip, int B, int b,
                                            const PState<T, N>& st) {
    using L = Layout<N>;
#pragma unroll
    for (int c = 0; c < 2; ++c) { pl(f, c, B, b) = st.r[c]; pl(f, 2 + c, B, b) = st.r[2 + c]; }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            pl(f, 4 * (i + 1) + c, B, b) = st.o[i][c];
            pl(f, 4 * (i + 1) + 2 + c, B, b) = st.o[i][2 + c];
            pl(f, L::CTR + 2 * i + c, B, b) = st.ctr[i][c];
        }
#pragma unroll
    for (int i = 0; i < N; ++i) pl(f, L::S + i, B, b) = st.s[i];
    pl(f, L::TIME, B, b) = st.time;
    ip[(size_t)b * 4 + L::I_T] = st.t;
    ip[(size_t)b * 4 + L::I_EP] = st.ep;
    ip[(size_t)b * 4 + L::I_HAVE] = st.have;
}

// one observation row: 1 + N stores of four values (16 bytes in float32), the row base is aligned to them
template <typename T, int N>
__device__ __forceinline__ void write_row(const PState<T, N>& st, T* __restrict__ o) {
    typedef T V4 __attribute__((ext_vector_type(4)));
    V4* const o4 = reinterpret_cast<V4*>(o);
    o4[0] = V4{st.r[0], st.r[1], st.r[2], st.r[3]};
#pragma unroll
    for (int i = 0; i < N; ++i) o4[1 + i] = V4{st.o[i][0], st.o[i][1], st.o[i][2], st.o[i][3]};
}

// ------------------------------------------------------------------ reset, base:25-39 + atacom:19-28
// draw(i, c): the value np.random.uniform(2, 8) returned for coordinate c of obstacle i
template <typename T, int N, typename DF>
__device__ __forceinline__ void point_reset(PState<T, N>& st, DF&& draw) {
    st.time = T(0);
    st.t = 0;
    st.r[0] = st.r[1] = T(1);
    st.r[2] = st.r[3] = T(0);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const T px = draw(i, 0), py = draw(i, 1);
        st.o[i][0] = px; st.o[i][1] = py;
        st.o[i][2] = st.o[i][3] = T(0);
        // base:35 appends a centre at every reset and base:71-72 index the list from its start: the centres of the
        // FIRST reset serve for the life of the object
        st.ctr[i][0] = st.have ? st.ctr[i][0] : px - T(2);
        st.ctr[i][1] = st.have ? st.ctr[i][1] : py;
        const T dx = st.r[0] - px, dy = st.r[1] - py;
        const T c = T(0.36) - num<T>::fma(dx, dx, dy * dy);
        st.s[i] = num<T>::sqrt(num<T>::max(T(-2) * c, T(0)));                           // atacom:26
    }
    st.have = 1;
    st.ep += 1;
}

template <typename T, int N>
__device__ __forceinline__ void point_reset_generated(const PParams<T>& P, int b, PState<T, N>& st) {
    const int ep = st.ep;
    point_reset<T, N>(st, [&](int i, int c) {
        return num<T>::fma(T(6), atacom::device_uniform<T>(P.seed, b, ep, 2 * i + c), T(2));
    });
}

// ------------------------------------------------------------------ one env step, atacom:30-52 + base:41-79
// draw(i, c): the value np.random.uniform(-1, 1) returned for coordinate c of obstacle i (random walk only).
// cmax: the row the reference appends to its constraint log BEFORE the step (atacom:41).
template <typename T, int N, typename DF>
__device__ __forceinline__ void point_step(const PParams<T>& P, PState<T, N>& st, const T (&alpha)[2], DF&& draw,
                                           T& reward, T& cmax) {
    constexpr int NN = N + 2;
    const T dt = P.dt;
    T d[N][2], rhs[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        d[i][0] = st.r[0] - st.o[i][0];
        d[i][1] = st.r[1] - st.o[i][1];
        const T d2 = num<T>::fma(d[i][0], d[i][0], d[i][1] * d[i][1]);
        const T c0 = T(0.36) - d2;                                                      // atacom:74-78
        cmax = (i == 0) ? c0 : num<T>::max(cmax, c0);
        // J_p dp + J_q dq = 2 d . (dp - dq), atacom:80-86
        const T dc = T(2) * num<T>::fma(d[i][0], st.o[i][2] - st.r[2], d[i][1] * (st.o[i][3] - st.r[3]));
        // get_bp + get_bq are built from POSITIONS (atacom:109-113): 2 d . p - 2 d . q = -2 |d|^2, times K = 0.5
        const T psi = dc - d2;                                                          // atacom:124-131
        const T c = c0 + num<T>::fma(T(0.5) * st.s[i], st.s[i], T(0.5) * dc);           // atacom:42
        rhs[i] = num<T>::fma(T(100), c, psi);
    }
    auto aget = [&](auto rc, auto cc) -> T {
        constexpr int r = decltype(rc)::value, c = decltype(cc)::value;
        if constexpr (c < 2) return T(-2) * d[r][c];                                    // J_q, atacom:88-90
        else if constexpr (c - 2 == r) return st.s[r];                                  // diag(s), atacom:121
        else return T(0);
    };
    auto yget = [&](auto rc) -> T { return -rhs[decltype(rc)::value]; };
    T x[NN], nb[NN][2];
    atacom::bidiag_solve_null<T, N, NN>(aget, yget, x, nb);                             // atacom:37 (pinv_null)
    // rref(N_c, row_vectors=False, tol=None): tol = max(m, n) eps |V|_inf, V = N_c^T (null_space_coordinate.py:49-50)
    T n0 = T(0), n1 = T(0);
#pragma unroll
    for (int j = 0; j < NN; ++j) { n0 += num<T>::abs(nb[j][0]); n1 += num<T>::abs(nb[j][1]); }
    const T tol = T(NN) * atacom::eps_of<T>::value * num<T>::max(n0, n1);
    T na[NN];
    atacom::rref_apply<T, NN, 2>(nb, alpha, tol, na);                                   // atacom:44,47
#pragma unroll
    for (int i = 0; i < N; ++i) st.s[i] = num<T>::fma(x[2 + i] + na[2 + i], dt, st.s[i]);   // atacom:48: the UNCLIPPED rate
    // base:45-54: clip to +-1, scale by 10, q with the old velocity, then the velocity, then the wall flip
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const T a = num<T>::clamp(x[c] + na[c], T(-1), T(1)) * T(10);
        st.r[c] = num<T>::fma(st.r[2 + c], dt, st.r[c]);
        const T v = num<T>::fma(a, dt, st.r[2 + c]);
        st.r[2 + c] = (st.r[c] <= T(0) || st.r[c] >= T(10)) ? -v : v;
    }
    if (P.random_walk) {                                                                // base:59-69 (launch-uniform)
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const T pn = num<T>::clamp(num<T>::fma(st.o[i][2 + c], dt, st.o[i][c]), T(2), T(10));
                const T u = draw(i, c);
                const T v = (pn <= T(2) || pn >= T(10)) ? -st.o[i][2 + c] : st.o[i][2 + c];
                st.o[i][c] = pn;
                st.o[i][2 + c] = num<T>::clamp(num<T>::fma(u * T(10), dt, v), T(-1), T(1));
            }
    } else {                                                                            // base:70-76; _time before it advances
        T sn, cs;
        num<T>::sincos(st.time * T(2) * T(3.141592653589793), &sn, &cs);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            st.o[i][0] = num<T>::fma(T(2), cs, st.ctr[i][0]);
            st.o[i][1] = num<T>::fma(T(2), sn, st.ctr[i][1]);
            st.o[i][2] = T(-4) * T(3.141592653589793) * sn;
            st.o[i][3] = T(4) * T(3.141592653589793) * cs;
        }
    }
    st.time += dt;                                                                      // base:78
    st.t += 1;
    const T gx = T(9) - st.r[0], gy = T(9) - st.r[1];
    reward = -num<T>::sqrt(num<T>::fma(gx, gx, gy * gy)) * T(0.08838834764831845);     // base:79: / (8 sqrt 2)
}

// ------------------------------------------------------------------ kernels
constexpr int BLOCK = 256;

// mask (nullable): environments whose byte is 0 keep their state.  draws (nullable): [B, N, 2] values of U(2, 8);
// without them the generator draws (seed, env, episode, 2 i + c).  obs (nullable): [B, 4 (1 + N)] current observation.
template <typename T, int N>
__global__ void __launch_bounds__(BLOCK) k_point_reset(const PParams<T> P, T* __restrict__ f, int* __restrict__ ip,
                                                       const uint8_t* __restrict__ mask, const T* __restrict__ draws,
                                                       T* __restrict__ obs) {
    using L = Layout<N>;
    const int B = P.batch;
    const int b = blockIdx.x * BLOCK + threadIdx.x;
    if (b >= B) return;
    PState<T, N> st;
    load_state<T, N>(f, ip, B, b, st);
    if (!mask || mask[b] != 0) {
        if (draws) point_reset<T, N>(st, [&](int i, int c) { return draws[((size_t)b * N + i) * 2 + c]; });
        else point_reset_generated<T, N>(P, b, st);
        store_state<T, N>(f, ip, B, b, st);
    }
    if (obs) write_row<T, N>(st, obs + (size_t)b * L::OBS);
}

template <typename T, int N>
__global__ void __launch_bounds__(BLOCK) k_point_step(const PParams<T> P, T* __restrict__ f, int* __restrict__ ip,
                                                      const T* __restrict__ action, const T* __restrict__ draws,
                                                      T* __restrict__ obs, T* __restrict__ reward,
                                                      uint8_t* __restrict__ absorbing, uint8_t* __restrict__ last) {
    using L = Layout<N>;
    const int B = P.batch;
    const int b = blockIdx.x * BLOCK + threadIdx.x;
    if (b >= B) return;
    PState<T, N> st;
    load_state<T, N>(f, ip, B, b, st);
    const T ssum0 = pl(f, L::SSUM, B, b), scmax0 = pl(f, L::SCMAX, B, b);
    const int cnt0 = ip[(size_t)b * 4 + L::I_CNT];
    const T alpha[2] = {action[(size_t)b * 2], action[(size_t)b * 2 + 1]};
    T r, cmax;
    const int t0 = st.t, ep = st.ep - 1;
    if (draws) point_step<T, N>(P, st, alpha, [&](int i, int c) { return draws[((size_t)b * N + i) * 2 + c]; }, r, cmax);
    else point_step<T, N>(P, st, alpha, [&](int i, int c) {
            return num<T>::fma(T(2), atacom::device_uniform<T>(P.seed, b, ep, 2 * N + 2 * (N * t0 + i) + c), T(-1));
        }, r, cmax);
    write_row<T, N>(st, obs + (size_t)b * L::OBS);
    const bool lst = st.t >= P.horizon;
    reward[b] = r;
    absorbing[b] = 0;                                                                   // base:80: never absorbing
    if (last) last[b] = lst ? 1 : 0;
    pl(f, L::SSUM, B, b) = ssum0 + cmax;
    pl(f, L::SCMAX, B, b) = num<T>::max(scmax0, cmax);
    ip[(size_t)b * 4 + L::I_CNT] = cnt0 + 1;
    if (P.auto_reset && lst) point_reset_generated<T, N>(P, b, st);
    store_state<T, N>(f, ip, B, b, st);
}

// n_steps steps per launch: the state is read once and written once.  actions [T, B, 2]; draws (nullable) [T, B, N, 2];
// obs / next_obs [T, B, 4 (1 + N)] (next_obs nullable); reward / absorbing / last [T, B].  An environment that reaches
// its horizon is reset in the kernel (generator draws keyed by its episode counter) when auto_reset is set.
template <typename T, int N>
__global__ void __launch_bounds__(BLOCK) k_point_rollout(const PParams<T> P, int n_steps, T* __restrict__ f,
                                                         int* __restrict__ ip, const T* __restrict__ actions,
                                                         const T* __restrict__ draws, T* __restrict__ obs,
                                                         T* __restrict__ next_obs, T* __restrict__ reward,
                                                         uint8_t* __restrict__ absorbing, uint8_t* __restrict__ last) {
    using L = Layout<N>;
    const int B = P.batch;
    const int b = blockIdx.x * BLOCK + threadIdx.x;
    if (b >= B) return;
    PState<T, N> st;
    load_state<T, N>(f, ip, B, b, st);
    T ssum = T(0), scmax = pl(f, L::SCMAX, B, b);
    // the actions of step t + 1 are fetched while step t computes (atacom_kernels.h: k_rollout)
    T act_next[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) act_next[k] = (n_steps > 0) ? actions[(size_t)b * 2 + k] : T(0);
#pragma unroll 1
    for (int t = 0; t < n_steps; ++t) {
        const size_t row = (size_t)t * B + b;
        const T alpha[2] = {act_next[0], act_next[1]};
        {
            const size_t nrow = (size_t)((t + 1 < n_steps) ? t + 1 : t) * B + b;        // last step: a harmless re-read
            act_next[0] = actions[nrow * 2];
            act_next[1] = actions[nrow * 2 + 1];
        }
        write_row<T, N>(st, obs + row * L::OBS);
        T r, cmax;
        const int t0 = st.t, ep = st.ep - 1;
        if (draws) point_step<T, N>(P, st, alpha, [&](int i, int c) { return draws[(row * N + i) * 2 + c]; }, r, cmax);
        else point_step<T, N>(P, st, alpha, [&](int i, int c) {
                return num<T>::fma(T(2), atacom::device_uniform<T>(P.seed, b, ep, 2 * N + 2 * (N * t0 + i) + c), T(-1));
            }, r, cmax);
        if (next_obs) write_row<T, N>(st, next_obs + row * L::OBS);
        const bool lst = st.t >= P.horizon;
        reward[row] = r;
        absorbing[row] = 0;
        last[row] = lst ? 1 : 0;
        ssum += cmax;
        scmax = num<T>::max(scmax, cmax);
        if (P.auto_reset && lst) point_reset_generated<T, N>(P, b, st);
    }
    pl(f, L::SSUM, B, b) += ssum;
    pl(f, L::SCMAX, B, b) = scmax;
    ip[(size_t)b * 4 + L::I_CNT] += n_steps;
    store_state<T, N>(f, ip, B, b, st);
}

// constraint statistics (atacom:133-139): per-block partials {sum, count, max} in double; clear != 0 empties the log
template <typename T, int N>
__global__ void __launch_bounds__(256) k_point_stats(int B, T* __restrict__ f, int* __restrict__ ip,
                                                     double* __restrict__ partial, int clear) {
    using L = Layout<N>;
    __shared__ double sh[3][256];
    double s = 0.0, c = 0.0, m = -INFINITY;
    for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {
        s += (double)pl(f, L::SSUM, B, b);
        c += (double)ip[(size_t)b * 4 + L::I_CNT];
        m = fmax(m, (double)pl(f, L::SCMAX, B, b));
        if (clear) {
            pl(f, L::SSUM, B, b) = T(0);
            pl(f, L::SCMAX, B, b) = -INFINITY;
            ip[(size_t)b * 4 + L::I_CNT] = 0;
        }
    }
    sh[0][threadIdx.x] = s; sh[1][threadIdx.x] = c; sh[2][threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + w];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + w];
            sh[2][threadIdx.x] = fmax(sh[2][threadIdx.x], sh[2][threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[blockIdx.x * 3 + 0] = sh[0][0];
        partial[blockIdx.x * 3 + 1] = sh[1][0];
        partial[blockIdx.x * 3 + 2] = sh[2][0];
    }
}

// state <-> the user-facing rows [B, 7 N + 8] = [state, s, centres, time, t, episode, have_centres]; set != 0 writes the
// handle (the statistics are not part of the row and stay)
template <typename T, int N>
__global__ void k_point_state_io(int B, T* __restrict__ f, int* __restrict__ ip, T* __restrict__ buf, int set) {
    using L = Layout<N>;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    T* const row = buf + (size_t)b * L::STATE_DIM;
    if (set) {
#pragma unroll
        for (int i = 0; i < L::TIME + 1; ++i) pl(f, i, B, b) = row[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) ip[(size_t)b * 4 + i] = (int)num<T>::max(row[L::TIME + 1 + i] + T(0.5), T(0));
    } else {
#pragma unroll
        for (int i = 0; i < L::TIME + 1; ++i) row[i] = pl(f, i, B, b);
#pragma unroll
        for (int i = 0; i < 3; ++i) row[L::TIME + 1 + i] = (T)ip[(size_t)b * 4 + i];
    }
}

}  // namespace atacom_point
