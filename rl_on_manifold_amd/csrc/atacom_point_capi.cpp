// C-ABI host side of libatacom_point.so (see include/atacom_point_hip.h).  Owns the per-handle device state and
// dispatches to the launch table of its (scalar type, obstacle count); contains no numerics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "atacom_point_handle.h"
#include "atacom_point_ops.h"
#define ATACOM_CAPI_E_HIP ATACOM_POINT_E_HIP
#include "atacom_capi_common.h"      // g_err, fail, HIP_TRY, DeviceGuard, ON_DEVICE

namespace {

constexpr int kStatBlocks = 256;

}  // namespace

// struct atacom_point_handle: atacom_point_handle.h (libatacom_point_policy.so borrows the handles created here)

namespace {
// observation rows are written four elements at a time
bool row_aligned(const atacom_point_handle* h, const void* p) {
    return ((uintptr_t)p & (4 * h->ops->elem - 1)) == 0;
}
}  // namespace

extern "C" {

const char* atacom_point_last_error(void) { return g_err.c_str(); }
const char* atacom_point_version(void) { return "atacom_point 1.0 (gfx950)"; }

int atacom_point_default_config(atacom_point_config* cfg) {
    if (!cfg) return fail(ATACOM_POINT_E_INVALID, "atacom_point_default_config: null argument");
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t)sizeof(*cfg);
    cfg->batch = 1;
    cfg->dtype = ATACOM_POINT_F32;
    cfg->n_objects = 4;
    cfg->random_walk = 0;
    cfg->horizon = 1000;
    cfg->auto_reset = 1;
    cfg->seed = 0;
    cfg->dt = 0.01;
    cfg->gamma = 0.99;
    return ATACOM_POINT_OK;
}

int atacom_point_create(const atacom_point_config* cfg, int device, atacom_point_handle** out) {
    if (!cfg || !out) return fail(ATACOM_POINT_E_INVALID, "atacom_point_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(atacom_point_config))
        return fail(ATACOM_POINT_E_INVALID, "atacom_point_create: struct_size does not match this library's atacom_point_config");
    if (cfg->batch <= 0 || cfg->horizon <= 0 || !(cfg->dt > 0.0))
        return fail(ATACOM_POINT_E_INVALID, "atacom_point_create: batch, horizon and dt must be positive");
    if (cfg->dtype != ATACOM_POINT_F32 && cfg->dtype != ATACOM_POINT_F64)
        return fail(ATACOM_POINT_E_INVALID, "atacom_point_create: dtype must be ATACOM_POINT_F32 or ATACOM_POINT_F64");
    const atacom_point::PointOps* ops = atacom_point::point_ops(cfg->dtype, cfg->n_objects);
    if (!ops)
        return fail(ATACOM_POINT_E_UNSUPPORTED, "atacom_point_create: n_objects = " + std::to_string(cfg->n_objects) +
                                                    " is not compiled in (kernels exist for 2 and 4 obstacles)");
    atacom_point_handle* h = new atacom_point_handle();
    h->magic = atacom_point::kHandleMagic;
    h->cfg = *cfg;
    h->ops = ops;
    h->device = device;
    h->f = nullptr; h->ip = nullptr; h->partial_dev = nullptr; h->partial_host = nullptr;
    DeviceGuard guard(device);
    const size_t fb = ops->elem * ops->values_per_env * (size_t)cfg->batch, ib = sizeof(int) * 4 * (size_t)cfg->batch;
    hipError_t e = guard.err;
    if (e == hipSuccess) e = hipMalloc(&h->f, fb);
    if (e == hipSuccess) e = hipMalloc((void**)&h->ip, ib);
    if (e == hipSuccess) e = hipMalloc((void**)&h->partial_dev, sizeof(double) * 3 * kStatBlocks);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->partial_host, sizeof(double) * 3 * kStatBlocks);
    if (e == hipSuccess) e = hipMemset(h->f, 0, fb);
    if (e == hipSuccess) e = hipMemset(h->ip, 0, ib);
    if (e == hipSuccess) {                       // an empty log: sum 0, max -inf, count 0
        ops->stats(h->cfg, h->f, h->ip, h->partial_dev, std::min(kStatBlocks, (cfg->batch + 255) / 256), 1, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        const std::string msg = std::string("atacom_point_create: ") + hipGetErrorString(e);
        atacom_point_destroy(h);
        return fail(ATACOM_POINT_E_HIP, msg);
    }
    *out = h;
    return ATACOM_POINT_OK;
}

int atacom_point_destroy(atacom_point_handle* h) {
    if (!h) return ATACOM_POINT_OK;
    DeviceGuard guard(h->device);
    if (h->f) (void)hipFree(h->f);
    if (h->ip) (void)hipFree(h->ip);
    if (h->partial_dev) (void)hipFree(h->partial_dev);
    if (h->partial_host) (void)hipHostFree(h->partial_host);
    h->magic = 0;
    delete h;
    return ATACOM_POINT_OK;
}

int atacom_point_reset(atacom_point_handle* h, const uint8_t* d_mask, const void* d_draws, void* d_obs, void* stream) {
    if (!h) return fail(ATACOM_POINT_E_INVALID, "atacom_point_reset: null handle");
    if (d_obs && !row_aligned(h, d_obs)) return fail(ATACOM_POINT_E_INVALID, "atacom_point_reset: d_obs must be aligned to four elements");
    ON_DEVICE(h);
    h->ops->reset(h->cfg, h->f, h->ip, d_mask, d_draws, d_obs, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_POINT_OK;
}

int atacom_point_step(atacom_point_handle* h, const void* d_action, const void* d_draws, void* d_obs, void* d_reward,
                      uint8_t* d_absorbing, uint8_t* d_last, void* stream) {
    if (!h || !d_action || !d_obs || !d_reward || !d_absorbing)
        return fail(ATACOM_POINT_E_INVALID, "atacom_point_step: null argument");
    if (!row_aligned(h, d_obs)) return fail(ATACOM_POINT_E_INVALID, "atacom_point_step: d_obs must be aligned to four elements");
    ON_DEVICE(h);
    h->ops->step(h->cfg, h->f, h->ip, d_action, d_draws, d_obs, d_reward, d_absorbing, d_last, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_POINT_OK;
}

int atacom_point_rollout(atacom_point_handle* h, int32_t n_steps, const void* d_actions, const void* d_draws, void* d_obs,
                         void* d_next_obs, void* d_reward, uint8_t* d_absorbing, uint8_t* d_last, void* stream) {
    if (!h || !d_actions || !d_obs || !d_reward || !d_absorbing || !d_last)
        return fail(ATACOM_POINT_E_INVALID, "atacom_point_rollout: null argument");
    if (n_steps <= 0) return fail(ATACOM_POINT_E_INVALID, "atacom_point_rollout: n_steps must be positive");
    if (!row_aligned(h, d_obs) || (d_next_obs && !row_aligned(h, d_next_obs)))
        return fail(ATACOM_POINT_E_INVALID, "atacom_point_rollout: d_obs / d_next_obs must be aligned to four elements");
    ON_DEVICE(h);
    h->ops->rollout(h->cfg, n_steps, h->f, h->ip, d_actions, d_draws, d_obs, d_next_obs, d_reward, d_absorbing, d_last,
                    (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_POINT_OK;
}

int atacom_point_get_stats(atacom_point_handle* h, double out[3], int32_t clear, void* stream) {
    if (!h || !out) return fail(ATACOM_POINT_E_INVALID, "atacom_point_get_stats: null argument");
    ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const int nb = std::min(kStatBlocks, (h->cfg.batch + 255) / 256);
    h->ops->stats(h->cfg, h->f, h->ip, h->partial_dev, nb, clear ? 1 : 0, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->partial_host, h->partial_dev, sizeof(double) * 3 * nb, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    double sum = 0.0, cnt = 0.0, cmax = -INFINITY;
    for (int i = 0; i < nb; ++i) {
        sum += h->partial_host[3 * i + 0];
        cnt += h->partial_host[3 * i + 1];
        cmax = std::fmax(cmax, h->partial_host[3 * i + 2]);
    }
    out[0] = cnt > 0 ? sum / cnt : NAN;    // np.mean of an empty log is nan as well
    out[1] = cmax;
    out[2] = 0.0;                          // collision_avoidance_atacom.py:40-41: the second log column is the constant 0
    return ATACOM_POINT_OK;
}

int atacom_point_get_state(atacom_point_handle* h, void* d_state, void* stream) {
    if (!h || !d_state) return fail(ATACOM_POINT_E_INVALID, "atacom_point_get_state: null argument");
    ON_DEVICE(h);
    h->ops->state_io(h->cfg, h->f, h->ip, d_state, 0, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_POINT_OK;
}

int atacom_point_set_state(atacom_point_handle* h, const void* d_state, void* stream) {
    if (!h || !d_state) return fail(ATACOM_POINT_E_INVALID, "atacom_point_set_state: null argument");
    ON_DEVICE(h);
    h->ops->state_io(h->cfg, h->f, h->ip, const_cast<void*>(d_state), 1, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_POINT_OK;
}

int atacom_point_set_seed(atacom_point_handle* h, int32_t seed) {
    if (!h) return fail(ATACOM_POINT_E_INVALID, "atacom_point_set_seed: null handle");
    h->cfg.seed = seed;
    return ATACOM_POINT_OK;
}

}  // extern "C"
