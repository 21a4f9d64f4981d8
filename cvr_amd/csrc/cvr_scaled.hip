// cvr_scaled.hip -- the C ABI of the scaled product (include/cvr_amd.h: cvr_spmv_scaled_device, cvr_spmv_scaled): y = alpha A x + beta y.
// The scaling is done where the kernels store a row's final value (cvr_kernels.h: ScaleEpi) -- the SpMV kernel of a single image and its fix-up of
// rows cut over chunks, or the combine pass of column panels --, so it costs the read of old y and no pass of its own.
// CVR_DEBUG=scaled_two_pass at cvr_create / cvr_load_image gives the handle the two-pass form instead: the plain product into a buffer of the handle,
// then an elementwise kernel (a bitwise cross-check of the fused write-outs and a timing baseline).
#include "cvr_internal.h"

using namespace cvrh;

namespace {

// the two-pass form's buffer for the plain product: y_ext's size, allocated at the first call that needs it
hipError_t two_pass_buffer(cvr_handle *h, void **out)
{
    if (!h->d_scaled_tmp) {
        const hipError_t e = hipMalloc(&h->d_scaled_tmp, h->vsz * (size_t)h->info.yext_elems);
        if (e != hipSuccess) { h->d_scaled_tmp = nullptr; return e; }
    }
    *out = h->d_scaled_tmp;
    return hipSuccess;
}

// after the argument checks
int scaled_device(cvr_handle *h, double alpha, const void *x, double beta, void *y, hipStream_t st)
{
    if (!h->converted) return fail(CVR_ERR_STATE, "cvr_spmv_scaled before cvr_preprocess");
    HIP_TRY(hipSetDevice(h->device));          // the NULL stream means the current device's
    const bool f32 = h->vsz == 4;
    // alpha and beta rounded to the handle's type: what every kernel computes with, and what decides the form
    const double a = f32 ? (double)(float)alpha : alpha, b = f32 ? (double)(float)beta : beta;
    const cvr::ScaleEpi sc{a, b, (uint32_t)h->info.nrows, b == 0 ? 1u : 2u};
    if (a == 0) {          // neither the matrix nor x is read: y = beta y, or +0
        HIP_TRY(cvr::launch_axpby(nullptr, y, h->info.nrows, f32, cvr::ScaleEpi{0, b, sc.nrows, b == 0 ? 0u : 2u}, st));
        return CVR_OK;
    }
    if (a == 1 && b == 0) {          // the plain product
        HIP_TRY(run_spmv(h, x, y, st));
        return CVR_OK;
    }
    if (h->scaled_two_pass) {
        void *t = nullptr;
        HIP_TRY(two_pass_buffer(h, &t));
        HIP_TRY(handle_enter(h, st));          // (the buffer is the handle's: a call on another stream waits for this one's elementwise pass)
        HIP_TRY(run_spmv(h, x, t, st));
        HIP_TRY(cvr::launch_axpby(t, y, h->info.nrows, f32, sc, st));
        HIP_TRY(handle_leave(h, st));
        return CVR_OK;
    }
    HIP_TRY(run_spmv(h, x, y, st, &sc));
    return CVR_OK;
}

}  // namespace

namespace cvrh {
int spmv_scaled_enqueue(cvr_handle *h, double alpha, const void *x, double beta, void *y, hipStream_t st) { return scaled_device(h, alpha, x, beta, y, st); }
}  // namespace cvrh

extern "C" {

int cvr_spmv_scaled_device(cvr_handle *h, double alpha, const void *x_dev, double beta, void *y_dev, void *stream)
{
    if (!h || !y_dev || (!x_dev && alpha != 0)) return fail(CVR_ERR_INVALID, "null argument");
    return scaled_device(h, alpha, x_dev, beta, y_dev, (hipStream_t)stream);
}

int cvr_spmv_scaled(cvr_handle *h, double alpha, const void *x_host, double beta, void *y_host)
{
    if (!h || !y_host || (!x_host && alpha != 0)) return fail(CVR_ERR_INVALID, "null argument");
    if (!h->converted) return fail(CVR_ERR_STATE, "cvr_spmv_scaled before cvr_preprocess");
    Range range("cvr_spmv_scaled (h2d x and y, one launch, d2h y)");
    HIP_TRY(hipSetDevice(h->device));
    if (x_host && h->info.ncols) HIP_TRY(hipMemcpyAsync(h->d_x, x_host, h->vsz * (size_t)h->info.ncols, hipMemcpyHostToDevice, h->stream));
    if (beta != 0 && h->info.nrows) HIP_TRY(hipMemcpyAsync(h->d_y, y_host, h->vsz * (size_t)h->info.nrows, hipMemcpyHostToDevice, h->stream));
    const int rc = scaled_device(h, alpha, x_host ? h->d_x : nullptr, beta, h->d_y, h->stream);
    if (rc) return rc;
    if (h->info.nrows) HIP_TRY(hipMemcpyAsync(y_host, h->d_y, h->vsz * (size_t)h->info.nrows, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return CVR_OK;
}

}  // extern "C"
