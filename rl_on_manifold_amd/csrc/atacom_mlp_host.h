// Host side of the network description atacom_mlp (include/atacom_hip.h), shared by every library that takes one: the
// ABI-size rule of its struct_size and the conversion to the kernels' argument block MlpArgs<T> (atacom_policy.h).
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/atacom_hip.h"

namespace atacom {

template <typename T>
struct MlpArgs;      // atacom_policy.h: complete wherever mlp_args is instantiated (the C-ABI files need the copy only)

// Copies *in to *net when its struct_size is this build's or the first release's (ATACOM_MLP_SIZE_V1): the latter gets the
// appended fields zeroed (mean_mode = explore = 0, what it ran before they existed) and its memory past that size is never
// read.  Returns false, *net untouched, for any other size.
static inline bool mlp_abi_copy(const atacom_mlp* in, atacom_mlp* net) {
    if (in->struct_size != (int32_t)sizeof(atacom_mlp) && in->struct_size != ATACOM_MLP_SIZE_V1) return false;
    std::memset(net, 0, sizeof(atacom_mlp));
    std::memcpy(net, in, (size_t)in->struct_size);
    return true;
}

template <typename T>
static MlpArgs<T> mlp_args(const atacom_mlp& net) {
    MlpArgs<T> a{};
    a.W1 = (const T*)net.W1; a.b1 = (const T*)net.b1; a.W2 = (const T*)net.W2; a.b2 = (const T*)net.b2;
    a.W3 = (const T*)net.W3; a.b3 = (const T*)net.b3; a.obs_shift = (const T*)net.obs_shift;
    a.obs_scale = (const T*)net.obs_scale; a.std = (const T*)net.std;
    a.sW1 = (const T*)net.sW1; a.sb1 = (const T*)net.sb1; a.sW2 = (const T*)net.sW2; a.sb2 = (const T*)net.sb2;
    a.sW3 = (const T*)net.sW3; a.sb3 = (const T*)net.sb3;
    a.log_std_min = (T)net.log_std_min; a.log_std_max = (T)net.log_std_max; a.squash = net.squash;
    a.n_in = net.n_in; a.n_out = net.n_out; a.activation = net.activation;
    a.mean_mode = net.mean_mode; a.explore = net.explore;
    a.act_scale = (const T*)net.act_scale; a.act_low = (const T*)net.act_low; a.act_high = (const T*)net.act_high;
    a.ou_x0 = (const T*)net.ou_x0; a.ou_state = (T*)net.ou_state;
    // x <- x - (theta dt) x + (sqrt(dt) std) eps: the two products of constants formed once, in double
    a.ou_theta_dt = (T)(net.ou_theta * net.ou_dt); a.ou_sqrt_dt = (T)(net.explore == 2 ? std::sqrt(net.ou_dt) : 0.0);
    return a;
}

}  // namespace atacom
