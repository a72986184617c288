// Kernels of libatacom_returns.so (include/atacom_returns_hip.h states the arithmetic).
//
// Scan kernels (k_returns_gae, k_returns_episodes, k_returns_lane_stats): one lane per (block w, environment b), adjacent lanes own
// adjacent environments, W on grid.y.  The recurrences are two dependent operations per step and no load depends on them, so a
// lane keeps the loads of the next kDepth steps in flight while it computes the kDepth steps it holds.  Registers only: no LDS,
// no scratch, no barrier.  The contraction is fixed: the fused multiply-adds the header writes down are explicit, and everything
// else stays a single IEEE operation -- contraction is off for the whole unit (build.py) and again by pragma in every kernel.
//
// Reduction stage (k_returns_reduce_partial, k_returns_reduce_final): the per-lane triples of doubles [3][L] are summed by a
// tree of fixed shape -- strided per-thread sums in index order, then a halving tree in LDS -- first into at most 256 partials,
// then into one.  No atomics: the same bits on every run.
#include "atacom_returns.h"

namespace atacom_returns {

template <typename T>
struct View {
    T* p;
    int64_t st, sb, sw;
};

template <typename T>
View<T> view_of(const atacom_returns_view& v) {
    return {static_cast<T*>(v.ptr), v.stride_t, v.stride_b, v.stride_w};
}

// the view moved to the lane's (b, w): what is left is the walk over t
template <typename T>
__device__ __forceinline__ T* lane_base(const View<T>& v, int b, int w) {
    return v.p + (int64_t)b * v.sb + (int64_t)w * v.sw;
}

template <typename E>
__device__ __forceinline__ bool is_set(uint8_t f) {
    return f != 0;
}
template <typename E>
__device__ __forceinline__ bool is_set(E f) {
    return f > (E)0.5;          // the flag columns of packed records, as rollout.unpack_fields reads them
}

__device__ __forceinline__ float fused(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fused(double a, double b, double c) { return __builtin_fma(a, b, c); }

__device__ __forceinline__ bool lane_is_real(const int32_t* sizes, int b, int w) { return sizes == nullptr || b < sizes[w]; }

template <typename E, typename F>
struct GaeParams {
    View<const E> r, v, vn;
    View<const F> ab, last;
    View<E> ret, adv;
    int T, B;
    E gamma, gl;
};

template <typename E, typename F, bool HAS_V>
__global__ __launch_bounds__(kScanBlock) void k_returns_gae(const GaeParams<E, F> p) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * kScanBlock + threadIdx.x, w = blockIdx.y;
    if (b >= p.B) return;
    const E* r = lane_base(p.r, b, w);
    const E* v = HAS_V ? lane_base(p.v, b, w) : nullptr;
    const E* vn = HAS_V ? lane_base(p.vn, b, w) : nullptr;
    const F* ab = lane_base(p.ab, b, w);
    const F* last = lane_base(p.last, b, w);
    E* ret = lane_base(p.ret, b, w);
    E* adv = lane_base(p.adv, b, w);

    struct Step {
        E r, v, vn;
        F ab, last;
    };
    Step cur[kDepth], nxt[kDepth];
    // steps t_hi, t_hi - 1, ...; an index below 0 repeats step 0 (in bounds, never used)
    auto load = [&](Step(&s)[kDepth], int t_hi) {
#pragma unroll
        for (int i = 0; i < kDepth; ++i) {
            const int64_t t = t_hi - i > 0 ? t_hi - i : 0;
            s[i].r = r[t * p.r.st];
            s[i].last = last[t * p.last.st];
            if (HAS_V) {
                s[i].ab = ab[t * p.ab.st];
                s[i].v = v[t * p.v.st];
                s[i].vn = vn[t * p.vn.st];
            }
        }
    };
    E carry = (E)0;
    load(cur, p.T - 1);
    for (int t_hi = p.T - 1; t_hi >= 0; t_hi -= kDepth) {
        const bool more = t_hi - kDepth >= 0;       // wave-uniform
        if (more) load(nxt, t_hi - kDepth);
#pragma unroll
        for (int i = 0; i < kDepth; ++i) {
            const int64_t t = t_hi - i;
            if (t >= 0) {
                const Step& s = cur[i];
                const E vv = HAS_V ? s.v : (E)0;
                const E vnext = HAS_V ? (is_set<E>(s.ab) ? (E)0 : s.vn) : (E)0;
                const E d = fused(p.gamma, vnext, s.r) - vv;
                const E a = fused(p.gl, is_set<E>(s.last) ? (E)0 : carry, d);
                carry = a;
                adv[t * p.adv.st] = a;
                ret[t * p.ret.st] = a + vv;
            }
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < kDepth; ++i) cur[i] = nxt[i];
        }
    }
}

template <typename E, typename F>
struct EpisodeParams {
    View<const E> r;
    View<const F> last;
    const int32_t* sizes;
    double* lanes;          // [3][L]: sum of j, number of episodes, sum of j * j of every lane
    int T, B;
    int64_t L;
    E gamma;
};

template <typename E, typename F>
__global__ __launch_bounds__(kScanBlock) void k_returns_episodes(const EpisodeParams<E, F> p) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * kScanBlock + threadIdx.x, w = blockIdx.y;
    if (b >= p.B) return;
    const int64_t lane = (int64_t)w * p.B + b;
    double sum = 0.0, count = 0.0, squares = 0.0;
    if (lane_is_real(p.sizes, b, w)) {
        const E* r = lane_base(p.r, b, w);
        const F* last = lane_base(p.last, b, w);
        struct Step {
            E r;
            F last;
        };
        Step cur[kDepth], nxt[kDepth];
        // steps t_lo, t_lo + 1, ...; an index past T - 1 repeats step T - 1 (in bounds, never used)
        auto load = [&](Step(&s)[kDepth], int t_lo) {
#pragma unroll
            for (int i = 0; i < kDepth; ++i) {
                const int64_t t = t_lo + i < p.T ? t_lo + i : p.T - 1;
                s[i].r = r[t * p.r.st];
                s[i].last = last[t * p.last.st];
            }
        };
        E j = (E)0, g = (E)1;
        load(cur, 0);
        for (int t_lo = 0; t_lo < p.T; t_lo += kDepth) {
            const bool more = t_lo + kDepth < p.T;
            if (more) load(nxt, t_lo + kDepth);
#pragma unroll
            for (int i = 0; i < kDepth; ++i) {
                const int t = t_lo + i;
                if (t < p.T) {
                    j = fused(g, cur[i].r, j);
                    g = g * p.gamma;
                    if (is_set<E>(cur[i].last) || t == p.T - 1) {
                        const double jd = (double)j;
                        sum = sum + jd;
                        squares = squares + jd * jd;
                        count = count + 1.0;
                        j = (E)0;
                        g = (E)1;
                    }
                }
            }
            if (more) {
#pragma unroll
                for (int i = 0; i < kDepth; ++i) cur[i] = nxt[i];
            }
        }
    }
    p.lanes[lane] = sum;
    p.lanes[p.L + lane] = count;
    p.lanes[2 * p.L + lane] = squares;
}

// per-lane [sum of adv, T, sum of adv * adv] over time, t descending like the scan; zeros for a padding lane
template <typename E>
__global__ __launch_bounds__(kScanBlock) void k_returns_lane_stats(const View<const E> adv, const int32_t* sizes, double* lanes,
                                                                   int T, int B, int64_t L) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * kScanBlock + threadIdx.x, w = blockIdx.y;
    if (b >= B) return;
    const int64_t lane = (int64_t)w * B + b;
    double sum = 0.0, squares = 0.0;
    const bool real = lane_is_real(sizes, b, w);
    if (real) {
        const E* a = lane_base(adv, b, w);
        for (int t_hi = T - 1; t_hi >= 0; t_hi -= kDepth) {
            E x[kDepth];
#pragma unroll
            for (int i = 0; i < kDepth; ++i) x[i] = a[(int64_t)(t_hi - i > 0 ? t_hi - i : 0) * adv.st];
#pragma unroll
            for (int i = 0; i < kDepth; ++i)
                if (t_hi - i >= 0) {
                    const double xd = (double)x[i];
                    sum = sum + xd;
                    squares = squares + xd * xd;
                }
        }
    }
    lanes[lane] = sum;
    lanes[L + lane] = real ? (double)T : 0.0;
    lanes[2 * L + lane] = squares;
}

// a halving tree over the block's kReduceBlock triples; the result is in thread 0
__device__ __forceinline__ void block_tree(double (&acc)[3], double (*lds)[kReduceBlock]) {
    const int tid = threadIdx.x;
    for (int k = 0; k < 3; ++k) lds[k][tid] = acc[k];
    __syncthreads();
    for (int s = kReduceBlock / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int k = 0; k < 3; ++k) lds[k][tid] = lds[k][tid] + lds[k][tid + s];
        __syncthreads();
    }
    for (int k = 0; k < 3; ++k) acc[k] = lds[k][0];
}

// block q sums the triples of lanes [q * chunk, (q + 1) * chunk) of in [3][n] into out [3][gridDim.x]
__global__ __launch_bounds__(kReduceBlock) void k_returns_reduce_partial(const double* in, int64_t n, int64_t chunk, double* out) {
#pragma clang fp contract(off)
    __shared__ double lds[3][kReduceBlock];
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t i = lo + threadIdx.x; i < hi; i += kReduceBlock)
        for (int k = 0; k < 3; ++k) acc[k] = acc[k] + in[k * n + i];
    block_tree(acc, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) out[(int64_t)k * gridDim.x + blockIdx.x] = acc[k];
}

// one block: the n <= kReduceBlock partials [3][n] -> out[3].  STATS: [sum, count, squares] -> [count, mean, population std]
template <bool STATS>
__global__ __launch_bounds__(kReduceBlock) void k_returns_reduce_final(const double* in, int n, double* out) {
#pragma clang fp contract(off)
    __shared__ double lds[3][kReduceBlock];
    double acc[3] = {0.0, 0.0, 0.0};
    if ((int)threadIdx.x < n)
        for (int k = 0; k < 3; ++k) acc[k] = in[k * n + threadIdx.x];
    block_tree(acc, lds);
    if (threadIdx.x == 0) {
        if (STATS) {
            // no real row at all (every block size 0): mean 0, std 0 -- nothing is normalised then, and nothing is NaN
            const double mean = acc[1] > 0.0 ? acc[0] / acc[1] : 0.0;
            const double var = acc[1] > 0.0 ? acc[2] / acc[1] - mean * mean : 0.0;
            out[0] = acc[1];
            out[1] = mean;
            out[2] = sqrt(var > 0.0 ? var : 0.0);
        } else {
            out[0] = acc[0];
            out[1] = acc[1];
            out[2] = acc[2];
        }
    }
}

// adv <- (adv - mean) / (std + 1e-8) on the real rows, in double from the statistics as they are returned, rounded once to E;
// grid (b blocks, T, W)
template <typename E>
__global__ __launch_bounds__(kReduceBlock) void k_returns_normalize(const View<E> adv, const int32_t* sizes, const double* stats,
                                                                    int B) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * kReduceBlock + threadIdx.x, t = blockIdx.y, w = blockIdx.z;
    if (b >= B || !lane_is_real(sizes, b, w)) return;
    const double mean = stats[1], scale = stats[2] + 1e-8;
    E* a = lane_base(adv, b, w) + (int64_t)t * adv.st;
    *a = (E)(((double)*a - mean) / scale);
}

static dim3 scan_grid(const atacom_returns_shape& sh) { return dim3((sh.batch + kScanBlock - 1) / kScanBlock, sh.n_blocks, 1); }

// the two reduction stages over lanes [3][L] at the head of ws; the partials follow them
template <bool STATS>
void reduce_launch(double* ws, int64_t L, double* out, hipStream_t s) {
    const int P = reduce_blocks(L);
    const int64_t chunk = (L + P - 1) / P;
    double* partials = ws + 3 * L;
    hipLaunchKernelGGL(k_returns_reduce_partial, dim3(P), dim3(kReduceBlock), 0, s, ws, L, chunk, partials);
    hipLaunchKernelGGL(k_returns_reduce_final<STATS>, dim3(1), dim3(kReduceBlock), 0, s, partials, P, out);
}

template <typename E, typename F>
void gae_launch_typed(const atacom_returns_gae_args& a, hipStream_t s) {
    GaeParams<E, F> p;
    p.r = view_of<const E>(a.reward);
    p.v = view_of<const E>(a.v);
    p.vn = view_of<const E>(a.v_next);
    p.ab = view_of<const F>(a.absorbing);
    p.last = view_of<const F>(a.last);
    p.ret = view_of<E>(a.ret);
    p.adv = view_of<E>(a.adv);
    p.T = a.shape.n_steps;
    p.B = a.shape.batch;
    p.gamma = (E)a.gamma;
    p.gl = (E)a.gamma * (E)a.lam;        // formed once, here, in the call's dtype
    if (a.v.ptr)
        hipLaunchKernelGGL((k_returns_gae<E, F, true>), scan_grid(a.shape), dim3(kScanBlock), 0, s, p);
    else
        hipLaunchKernelGGL((k_returns_gae<E, F, false>), scan_grid(a.shape), dim3(kScanBlock), 0, s, p);
}

template <typename E, typename F>
void episodes_launch_typed(const atacom_returns_episodes_args& a, hipStream_t s) {
    EpisodeParams<E, F> p;
    p.r = view_of<const E>(a.reward);
    p.last = view_of<const F>(a.last);
    p.sizes = a.shape.d_sizes;
    p.lanes = a.d_workspace;
    p.T = a.shape.n_steps;
    p.B = a.shape.batch;
    p.L = (int64_t)a.shape.n_blocks * a.shape.batch;
    p.gamma = (E)a.gamma;
    hipLaunchKernelGGL((k_returns_episodes<E, F>), scan_grid(a.shape), dim3(kScanBlock), 0, s, p);
    reduce_launch<false>(a.d_workspace, p.L, a.d_result, s);
}

template <typename E>
void normalize_launch_typed(const atacom_returns_shape& sh, const atacom_returns_view& adv, double* ws, double* stats, hipStream_t s) {
    const int64_t L = (int64_t)sh.n_blocks * sh.batch;
    hipLaunchKernelGGL(k_returns_lane_stats<E>, scan_grid(sh), dim3(kScanBlock), 0, s, view_of<const E>(adv), sh.d_sizes, ws,
                       sh.n_steps, sh.batch, L);
    reduce_launch<true>(ws, L, stats, s);
    hipLaunchKernelGGL(k_returns_normalize<E>, dim3((sh.batch + kReduceBlock - 1) / kReduceBlock, sh.n_steps, sh.n_blocks),
                       dim3(kReduceBlock), 0, s, view_of<E>(adv), sh.d_sizes, stats, sh.batch);
}

int gae_launch(const atacom_returns_gae_args& a, hipStream_t s) {
    const bool f64 = a.shape.dtype == ATACOM_RETURNS_F64, bytes = a.shape.flag_dtype == ATACOM_RETURNS_FLAG_U8;
    if (f64)
        bytes ? gae_launch_typed<double, uint8_t>(a, s) : gae_launch_typed<double, double>(a, s);
    else
        bytes ? gae_launch_typed<float, uint8_t>(a, s) : gae_launch_typed<float, float>(a, s);
    return 0;
}

int normalize_launch(const atacom_returns_shape& sh, const atacom_returns_view& adv, double* ws, double* stats, hipStream_t s) {
    if (sh.dtype == ATACOM_RETURNS_F64)
        normalize_launch_typed<double>(sh, adv, ws, stats, s);
    else
        normalize_launch_typed<float>(sh, adv, ws, stats, s);
    return 0;
}

int episodes_launch(const atacom_returns_episodes_args& a, hipStream_t s) {
    const bool f64 = a.shape.dtype == ATACOM_RETURNS_F64, bytes = a.shape.flag_dtype == ATACOM_RETURNS_FLAG_U8;
    if (f64)
        bytes ? episodes_launch_typed<double, uint8_t>(a, s) : episodes_launch_typed<double, double>(a, s);
    else
        bytes ? episodes_launch_typed<float, uint8_t>(a, s) : episodes_launch_typed<float, float>(a, s);
    return 0;
}

}  // namespace atacom_returns
