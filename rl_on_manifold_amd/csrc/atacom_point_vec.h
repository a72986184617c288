// Kernels of libatacom_point_vec.so (include/atacom_point_vec_hip.h): the collision-avoidance task's masked step and the copy
// behind its checkpoint.  The environment itself -- point_step, point_reset_generated, the state layout and its accessors --
// is atacom_point.h, called and not copied: a masked-in lane runs the instructions' source of k_point_step.
#pragma once
#include <stdint.h>
#include "../../include/atacom_point_vec_hip.h"
#include "atacom_point.h"
#include "atacom_point_vec_ops.h"

namespace atacom_point {

// k_point_step for the environments whose mask byte is not zero (mask == nullptr: all of them).  One environment per lane,
// everything in registers.  A masked-out lane leaves by the first branch: it has written its observation row and three
// output scalars and nothing of the handle.  Its action and draw rows are not read.  The whole state is loaded BEFORE the mask
// byte is looked at, next to it: a masked-in lane then waits for memory once, as in k_point_step, and not twice.  What a
// masked-out lane saves is the write-back; loading only its observation groups would save a wave nothing unless the mask is
// the same across 64-byte segments, since neighbouring lanes share them (profiles/point_vec.md).
template <typename T, int N>
__global__ void __launch_bounds__(BLOCK) k_point_step_masked(const PParams<T> P, T* __restrict__ f, int* __restrict__ ip,
                                                             const uint8_t* __restrict__ mask, const T* __restrict__ action,
                                                             const T* __restrict__ draws, T* __restrict__ obs,
                                                             T* __restrict__ reward, uint8_t* __restrict__ absorbing,
                                                             uint8_t* __restrict__ last) {
    using L = Layout<N>;
    const int B = P.batch;
    const int b = blockIdx.x * BLOCK + threadIdx.x;
    if (b >= B) return;
    PState<T, N> st;
    load_state<T, N>(f, ip, B, b, st);
    if (mask && mask[b] == 0) {
        write_row<T, N>(st, obs + (size_t)b * L::OBS);
        reward[b] = T(0);
        absorbing[b] = 0;
        if (last) last[b] = 0;
        return;
    }
    // from here on: the body of k_point_step
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
    absorbing[b] = 0;
    if (last) last[b] = lst ? 1 : 0;
    pl(f, L::SSUM, B, b) = ssum0 + cmax;
    pl(f, L::SCMAX, B, b) = num<T>::max(scmax0, cmax);
    ip[(size_t)b * 4 + L::I_CNT] = cnt0 + 1;
    if (P.auto_reset && lst) point_reset_generated<T, N>(P, b, st);
    store_state<T, N>(f, ip, B, b, st);
}

// ------------------------------------------------------------------ checkpoint
// SnapHeader, what an image starts with: atacom_point_vec_ops.h (the host reads it back)
constexpr int kSnapHeaderItems = (int)(sizeof(SnapHeader) / 16);

typedef uint32_t Item __attribute__((ext_vector_type(4)));       // 16 bytes: the copy does not know the handle's scalar type

// image = [header | nf items of the float buffer | ni items of the int buffer].  SAVE: the handle's buffers -> the image,
// the header written from the launch arguments by the first lane of the grid (vector stores); else the image -> the buffers
// (the header has been read and checked by the host).  Grid-stride: the launcher caps the grid.
template <bool SAVE>
__global__ void __launch_bounds__(BLOCK) k_point_snapshot_copy(const SnapHeader hdr, Item* __restrict__ fbuf, size_t nf,
                                                               Item* __restrict__ ibuf, size_t ni, Item* __restrict__ image) {
    Item* const body = image + kSnapHeaderItems;
    const size_t stride = (size_t)gridDim.x * BLOCK;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < nf + ni; i += stride) {
        Item* const p = (i < nf) ? fbuf + i : ibuf + (i - nf);
        if (SAVE) body[i] = *p;
        else *p = body[i];
    }
    if (SAVE && blockIdx.x == 0 && threadIdx.x == 0) {
        image[0] = Item{hdr.magic, hdr.format, (uint32_t)hdr.dtype, (uint32_t)hdr.n_objects};
        image[1] = Item{(uint32_t)hdr.batch, (uint32_t)hdr.seed, 0u, 0u};
        image[2] = Item{0u, 0u, 0u, 0u};
        image[3] = Item{0u, 0u, 0u, 0u};
    }
}

}  // namespace atacom_point
