// Kernels of libatacom_offstep.so (include/atacom_offstep_hip.h states the arithmetic): k_adam_track<T>, one Adam step of up to
// four parameter groups and the soft update of their target networks in one launch, and k_adam_track_init, which makes their
// states fresh.  One workgroup per group.  A group is at most 7304 values -- eight values a thread -- so what the launch costs
// is its latency, not bandwidth, and nothing here is tuned for bandwidth: the kernel is a single pass with no loop-carried
// dependence, its five loads per value are independent and issued together, and the only serial part is thread 0's handful of
// double operations, whose results reach the other threads through LDS (one address: a broadcast read).  The target follows
// the parameter from the register that holds it, which is what a separate soft-update launch would have had to read back.
// Whether a group is stepped and whether it has a target are uniform over its workgroup: the branches below do not diverge.
// Compiled with -ffp-contract=off (build.UNIT_FLAGS): every operation below is the individually rounded one it is written as.
#include "atacom_offstep.h"

namespace atacom_offstep {

struct Head {
    long long step;
    double beta1_pow, beta2_pow;
    long long reserved;
};
static_assert(sizeof(Head) == ATACOM_OFFSTEP_HEAD, "the head of a state is 32 bytes");

struct Group {
    void* p[kSegments];        // W1, b1, W2, b2, W3, b3, W2a
    void* t[kSegments];        // the target's, all null without one
    const void* grad;          // null: the group is not stepped
    void* state;
    double lr, grad_scale;
    int n[kSegments];          // values of each segment
    int N;
};

struct Launch {
    Group g[ATACOM_OFFSTEP_MAX_GROUPS];
    double beta1, beta2, eps, tau;
};

__device__ inline float sqrt_t(float x) { return sqrtf(x); }
__device__ inline double sqrt_t(double x) { return sqrt(x); }

template <typename T>
__global__ __launch_bounds__(kBlock) void k_adam_track(const Launch L) {
    const Group& G = L.g[blockIdx.x];
    const bool stepped = G.grad != nullptr, tracked = G.t[0] != nullptr;
    if (!stepped && !tracked) return;                    // (the whole workgroup: no barrier is left waiting)
    Head* head = (Head*)G.state;
    __shared__ T sc[8];
    Head next = {0, 0.0, 0.0, 0};
    if (stepped && threadIdx.x == 0) {
        const Head h = *head;
        next.step = h.step + 1;
        next.beta1_pow = h.beta1_pow * L.beta1;
        next.beta2_pow = h.beta2_pow * L.beta2;
        sc[0] = (T)(G.lr / (1.0 - next.beta1_pow));      // step_size
        sc[1] = (T)sqrt(1.0 - next.beta2_pow);           // bc2s
        sc[2] = (T)(1.0 - L.beta1);
        sc[3] = (T)L.beta2;
        sc[4] = (T)(1.0 - L.beta2);
        sc[5] = (T)L.eps;
        sc[6] = (T)G.grad_scale;
    }
    __syncthreads();
    T step_size = 0, bc2s = 0, omb1 = 0, beta2 = 0, omb2 = 0, eps = 0, scale = 0;
    if (stepped) step_size = sc[0], bc2s = sc[1], omb1 = sc[2], beta2 = sc[3], omb2 = sc[4], eps = sc[5], scale = sc[6];
    const T a = (T)L.tau, b = (T)(1.0 - L.tau);          // as k_soft_update of libatacom_offpolicy.so forms them
    const T* grad = (const T*)G.grad;
    T* m = (T*)((char*)G.state + ATACOM_OFFSTEP_HEAD);
    T* v = m + G.N;
    int off = 0;
#pragma unroll
    for (int s = 0; s < kSegments; ++s) {
        T* par = (T*)G.p[s];
        T* tgt = (T*)G.t[s];
        const int n = G.n[s];
        for (int i = threadIdx.x; i < n; i += kBlock) {
            T gi = 0, mi = 0, vi = 0, ti = 0;
            T pn = par[i];
            if (stepped) gi = grad[off + i], mi = m[off + i], vi = v[off + i];
            if (tracked) ti = tgt[i];
            if (stepped) {
                const T g = scale * gi;
                const T mn = mi + (g - mi) * omb1;
                const T vn = beta2 * vi + (omb2 * g) * g;
                pn = pn - step_size * (mn / (sqrt_t(vn) / bc2s + eps));
                m[off + i] = mn;
                v[off + i] = vn;
                par[i] = pn;
            }
            if (tracked) {
                const T x = a * pn;
                const T z = b * ti;
                tgt[i] = x + z;
            }
        }
        off += n;
    }
    if (!stepped) return;
    __syncthreads();                                     // (thread 0 read the head before the first barrier)
    if (threadIdx.x == 0) *head = next;
}

// A fresh state: zero words from the end of the head on, and the head itself.
__global__ __launch_bounds__(kBlock) void k_adam_track_init(const Launch L, const int esize) {
    const Group& G = L.g[blockIdx.x];
    unsigned* w = (unsigned*)G.state;
    const int words = (ATACOM_OFFSTEP_HEAD + 2 * G.N * esize) / 4;
    for (int i = ATACOM_OFFSTEP_HEAD / 4 + threadIdx.x; i < words; i += kBlock) w[i] = 0u;
    if (threadIdx.x == 0) *(Head*)G.state = Head{0, 1.0, 1.0, 0};
}

static Launch pack(const atacom_offstep_args& a) {
    Launch L = {};
    L.beta1 = a.beta1, L.beta2 = a.beta2, L.eps = a.eps, L.tau = a.tau;
    for (int k = 0; k < a.n_groups; ++k) {
        const atacom_offstep_group& s = a.groups[k];
        Group& g = L.g[k];
        void* const p[kSegments] = {s.W1, s.b1, s.W2, s.b2, s.W3, s.b3, s.W2a};
        g.N = segments(s.n_in, s.n_out, s.n_act, g.n);
        for (int i = 0; i < kSegments; ++i) {
            const bool used = g.n[i] > 0;                // a plain network has no W2a: its pointers are never formed
            g.p[i] = used ? p[i] : nullptr;
            g.t[i] = used && s.target[0] ? s.target[i] : nullptr;
        }
        g.grad = s.grad, g.state = s.state, g.lr = s.lr, g.grad_scale = s.grad_scale;
    }
    return L;
}

void init_launch(const atacom_offstep_args& a, hipStream_t s) {
    hipLaunchKernelGGL(k_adam_track_init, dim3(a.n_groups), dim3(kBlock), 0, s, pack(a), a.dtype == ATACOM_OFFSTEP_F64 ? 8 : 4);
}

void step_launch(const atacom_offstep_args& a, hipStream_t s) {
    if (a.dtype == ATACOM_OFFSTEP_F64)
        hipLaunchKernelGGL(k_adam_track<double>, dim3(a.n_groups), dim3(kBlock), 0, s, pack(a));
    else
        hipLaunchKernelGGL(k_adam_track<float>, dim3(a.n_groups), dim3(kBlock), 0, s, pack(a));
}

}  // namespace atacom_offstep
