// C-ABI host side of libatacom_point_vec.so (see include/atacom_point_vec_hip.h).  Borrows the handles of libatacom_point.so
// (atacom_point_handle.h); validates, then dispatches to the launchers; contains no numerics.
#include <hip/hip_runtime.h>

#include <string>

#include "atacom_point_handle.h"
#include "atacom_point_vec_ops.h"
#define ATACOM_CAPI_E_HIP ATACOM_POINT_E_HIP
#include "atacom_capi_common.h"      // g_err, fail, HIP_TRY, DeviceGuard, ON_DEVICE

namespace {

using atacom_point::SnapHeader;

std::string dec(long long v) { return std::to_string(v); }

// the first thing every entry point does with a handle: nothing of it is used before the layout number has been seen
int check_handle(const atacom_point_handle* h, const std::string& w) {
    if (!h) return fail(ATACOM_POINT_E_INVALID, w + ": null handle");
    if (h->magic != atacom_point::kHandleMagic)
        return fail(ATACOM_POINT_E_INVALID, w + ": not a live handle of the libatacom_point.so this library was built with "
                                                "(layout number mismatch, or the handle was destroyed)");
    return ATACOM_POINT_OK;
}

size_t elem_bytes(const atacom_point_handle* h) { return h->cfg.dtype == ATACOM_POINT_F64 ? 8 : 4; }

// sizes of the handle's two device buffers, as atacom_point_create allocated them; 0 for a shape this library does not know
size_t float_bytes(const atacom_point_handle* h) {
    return elem_bytes(h) * (size_t)atacom_point::point_vec_values_per_env(h->cfg.n_objects) * (size_t)h->cfg.batch;
}
size_t int_bytes(const atacom_point_handle* h) { return sizeof(int) * 4 * (size_t)h->cfg.batch; }

int check_shape(const atacom_point_handle* h, const std::string& w) {
    if ((h->cfg.dtype != ATACOM_POINT_F32 && h->cfg.dtype != ATACOM_POINT_F64) || float_bytes(h) == 0)
        return fail(ATACOM_POINT_E_UNSUPPORTED, w + ": no kernel for dtype " + dec(h->cfg.dtype) + ", n_objects = " + dec(h->cfg.n_objects));
    return ATACOM_POINT_OK;
}

// reads the header of an image (synchronises the stream) and compares every field with the handle; writes nothing
int read_header(const atacom_point_handle* h, const void* d_image, const std::string& w, hipStream_t s, SnapHeader* got) {
    HIP_TRY(hipMemcpyAsync(got, d_image, sizeof(*got), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (got->magic != atacom_point::kSnapMagic) return fail(ATACOM_POINT_E_INVALID, w + ": not a checkpoint image of this library (bad magic)");
    auto differs = [&](const char* field, long long image, long long handle) {
        return fail(ATACOM_POINT_E_INVALID, w + ": image " + field + " = " + dec(image) + ", handle " + dec(handle));
    };
    if (got->format != atacom_point::kSnapFormat)
        return fail(ATACOM_POINT_E_INVALID, w + ": image format = " + dec(got->format) + ", this library reads format " +
                                                dec(atacom_point::kSnapFormat));
    if (got->dtype != h->cfg.dtype) return differs("dtype", got->dtype, h->cfg.dtype);
    if (got->n_objects != h->cfg.n_objects) return differs("n_objects", got->n_objects, h->cfg.n_objects);
    if (got->batch != h->cfg.batch) return differs("batch", got->batch, h->cfg.batch);
    return ATACOM_POINT_OK;
}

}  // namespace

extern "C" {

const char* atacom_point_vec_last_error(void) { return g_err.c_str(); }
const char* atacom_point_vec_version(void) { return "atacom_point_vec 1.0 (gfx950)"; }

int atacom_point_vec_step_masked(atacom_point_handle* h, const uint8_t* d_mask, const void* d_action, const void* d_draws,
                                 void* d_obs, void* d_reward, uint8_t* d_absorbing, uint8_t* d_last, void* stream) {
    const std::string w = "atacom_point_vec_step_masked";
    if (int rc = check_handle(h, w)) return rc;
    if (!d_action || !d_obs || !d_reward || !d_absorbing) return fail(ATACOM_POINT_E_INVALID, w + ": null argument");
    if ((uintptr_t)d_obs & (4 * elem_bytes(h) - 1)) return fail(ATACOM_POINT_E_INVALID, w + ": d_obs must be aligned to four elements");
    ON_DEVICE(h);
    if (atacom_point::point_vec_step_launch(h->cfg, h->f, h->ip, d_mask, d_action, d_draws, d_obs, d_reward, d_absorbing, d_last,
                                            (hipStream_t)stream))
        return fail(ATACOM_POINT_E_UNSUPPORTED, w + ": no kernel for dtype " + dec(h->cfg.dtype) + ", n_objects = " + dec(h->cfg.n_objects));
    HIP_TRY(hipGetLastError());
    return ATACOM_POINT_OK;
}

int64_t atacom_point_vec_snapshot_bytes(const atacom_point_handle* h) {
    const std::string w = "atacom_point_vec_snapshot_bytes";
    if (int rc = check_handle(h, w)) return rc;
    if (int rc = check_shape(h, w)) return rc;
    return (int64_t)(sizeof(SnapHeader) + float_bytes(h) + int_bytes(h));
}

int atacom_point_vec_snapshot_save(atacom_point_handle* h, void* d_image, void* stream) {
    const std::string w = "atacom_point_vec_snapshot_save";
    if (int rc = check_handle(h, w)) return rc;
    if (!d_image) return fail(ATACOM_POINT_E_INVALID, w + ": null argument");
    if ((uintptr_t)d_image & 15) return fail(ATACOM_POINT_E_INVALID, w + ": d_image must be aligned to 16 bytes");
    if (int rc = check_shape(h, w)) return rc;
    ON_DEVICE(h);
    atacom_point::point_vec_snapshot_launch(h->cfg, true, h->f, float_bytes(h), h->ip, int_bytes(h), d_image, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return ATACOM_POINT_OK;
}

int atacom_point_vec_snapshot_inspect(atacom_point_handle* h, const void* d_image, int32_t* seed, void* stream) {
    const std::string w = "atacom_point_vec_snapshot_inspect";
    if (int rc = check_handle(h, w)) return rc;
    if (!d_image) return fail(ATACOM_POINT_E_INVALID, w + ": null argument");
    ON_DEVICE(h);
    SnapHeader got;
    if (int rc = read_header(h, d_image, w, (hipStream_t)stream, &got)) return rc;
    if (seed) *seed = got.seed;
    return ATACOM_POINT_OK;
}

int atacom_point_vec_snapshot_restore(atacom_point_handle* h, const void* d_image, void* stream) {
    const std::string w = "atacom_point_vec_snapshot_restore";
    if (int rc = check_handle(h, w)) return rc;
    if (!d_image) return fail(ATACOM_POINT_E_INVALID, w + ": null argument");
    if ((uintptr_t)d_image & 15) return fail(ATACOM_POINT_E_INVALID, w + ": d_image must be aligned to 16 bytes");
    if (int rc = check_shape(h, w)) return rc;
    ON_DEVICE(h);
    SnapHeader got;
    if (int rc = read_header(h, d_image, w, (hipStream_t)stream, &got)) return rc;
    atacom_point::point_vec_snapshot_launch(h->cfg, false, h->f, float_bytes(h), h->ip, int_bytes(h), const_cast<void*>(d_image),
                                            (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    h->cfg.seed = got.seed;              // what atacom_point_set_seed does
    return ATACOM_POINT_OK;
}

}  // extern "C"
