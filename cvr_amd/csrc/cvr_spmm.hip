// cvr_spmm.hip -- the C ABI of several vectors at once (include/cvr_amd.h: cvr_spmm_device, cvr_spmm, cvr_spmm_supported): Y = A X over
// an image of the plain layout, the one cvr_create builds for cvr_options.nvec >= 2 (the k-wide kernel: cvr_spmv.hip, spmm_kernel).
#include "cvr_internal.h"

using namespace cvrh;

namespace {

// the handle's one image, if it is of the plain layout (column panels are several images: never)
const cvr::DeviceImage *plain_image(const cvr_handle *h)
{
    if (!h || !h->converted || h->parts.size() != 1 || !cvr::spmm_plain(h->parts[0].img)) return nullptr;
    return &h->parts[0].img;
}

int check_args(const cvr_handle *h, const void *X, int64_t ldx, const void *Y, int64_t ldy, int32_t nvec)
{
    if (!h || !X || !Y) return fail(CVR_ERR_INVALID, "null argument");
    if (nvec < 1) return fail(CVR_ERR_INVALID, "nvec = %d: at least one vector", nvec);
    if (ldx < nvec || ldy < nvec) return fail(CVR_ERR_INVALID, "ldx = %lld, ldy = %lld: each must be >= nvec = %d", (long long)ldx, (long long)ldy, nvec);
    return CVR_OK;
}

// after check_args: the device work of cvr_spmm_device
int spmm_device(cvr_handle *h, const void *X, int64_t ldx, void *Y, int64_t ldy, int32_t nvec, hipStream_t st)
{
    if (!h->converted) return fail(CVR_ERR_STATE, "cvr_spmm before cvr_preprocess");
    HIP_TRY(hipSetDevice(h->device));          // the NULL stream means the current device's
    if (nvec == 1 && ldx == 1 && ldy == 1) {          // one vector of stride 1: cvr_spmv_device, whatever the layout
        HIP_TRY(run_spmv(h, X, Y, st));
        return CVR_OK;
    }
    const cvr::DeviceImage *img = plain_image(h);
    if (!img) return fail(CVR_ERR_STATE, "cvr_spmm_device: this handle's image is not the plain layout; create it with cvr_options.nvec >= 2 for several vectors");
    if ((uint64_t)(h->info.ncols + 1) * (uint64_t)ldx * h->vsz > 0xffffffffull)
        return fail(CVR_ERR_INVALID, "X of %lld rows of %lld values exceeds the 4 GiB a buffer descriptor addresses", (long long)(h->info.ncols + 1), (long long)ldx);
    if (h->d_map) HIP_TRY(handle_enter(h, st));          // (a mutable handle's image: ordered with its updates)
    HIP_TRY(cvr::launch_spmm(*img, X, ldx, Y, ldy, nvec, st));
    if (h->d_map) HIP_TRY(handle_leave(h, st));
    return CVR_OK;
}

}  // namespace

extern "C" {

int cvr_spmm_supported(const cvr_handle *h) { return plain_image(h) ? 1 : 0; }

int cvr_spmm_device(cvr_handle *h, const void *X_dev, int64_t ldx, void *Y_dev, int64_t ldy, int32_t nvec, void *stream)
{
    const int rc = check_args(h, X_dev, ldx, Y_dev, ldy, nvec);
    if (rc) return rc;
    return spmm_device(h, X_dev, ldx, Y_dev, ldy, nvec, (hipStream_t)stream);
}

int cvr_spmm(cvr_handle *h, const void *X_host, void *Y_host, int32_t nvec, int iters, cvr_timing *tm)
{
    int rc = check_args(h, X_host, nvec, Y_host, nvec, nvec);
    if (rc) return rc;
    if (!h->converted) return fail(CVR_ERR_STATE, "cvr_spmm before cvr_preprocess");
    if (iters < 1) iters = 1;
    Range range("cvr_spmm (h2d X, timed launches, d2h Y)");
    HIP_TRY(hipSetDevice(h->device));
    const size_t need = (size_t)iters + 1;
    while (h->events.size() < need) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        h->events.push_back(e);
    }
    // X_ext = [X | a zero row], Y_ext = [Y | dump | carry slots], nvec values per row, in one allocation for this call
    const size_t xb = h->vsz * (size_t)nvec * (size_t)(h->info.ncols + 1), yb = h->vsz * (size_t)nvec * (size_t)h->info.yext_elems;
    struct Mem { void *p = nullptr; ~Mem() { if (p) (void)hipFree(p); } } mem;
    HIP_TRY(hipMalloc(&mem.p, xb + yb + 256));
    uint8_t *X = static_cast<uint8_t *>(mem.p), *Y = X + ((xb + 255) & ~(size_t)255);
    double t0 = now_s();
    if (h->info.ncols) HIP_TRY(hipMemcpyAsync(X, X_host, xb - h->vsz * (size_t)nvec, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(X + xb - h->vsz * (size_t)nvec, 0, h->vsz * (size_t)nvec, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const double h2d = now_s() - t0;
    rc = spmm_device(h, X, nvec, Y, nvec, nvec, h->stream);          // warm-up, untimed
    if (rc) return rc;
    HIP_TRY(hipEventRecord(h->events[0], h->stream));
    for (int i = 0; i < iters; i++) {
        rc = spmm_device(h, X, nvec, Y, nvec, nvec, h->stream);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(h->events[(size_t)i + 1], h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    t0 = now_s();
    if (h->info.nrows) HIP_TRY(hipMemcpyAsync(Y_host, Y, h->vsz * (size_t)nvec * (size_t)h->info.nrows, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const double d2h = now_s() - t0;
    if (tm) {
        memset(tm, 0, sizeof(*tm));
        tm->iters = iters; tm->h2d_s = h2d; tm->d2h_s = d2h;
        double              sum = 0;
        std::vector<double> ts((size_t)iters);
        for (int i = 0; i < iters; i++) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, h->events[(size_t)i], h->events[(size_t)i + 1]));
            ts[(size_t)i] = ms * 1e-3;
            sum += ts[(size_t)i];
        }
        float tot = 0;
        HIP_TRY(hipEventElapsedTime(&tot, h->events[0], h->events[(size_t)iters]));
        std::sort(ts.begin(), ts.end());
        tm->mean_s = sum / iters; tm->min_s = ts.front(); tm->max_s = ts.back(); tm->median_s = ts[ts.size() / 2]; tm->total_s = tot * 1e-3;
        tm->step_mean_s = tm->mean_s; tm->step_min_s = tm->min_s; tm->step_median_s = tm->median_s; tm->step_max_s = tm->max_s; tm->gather_mean_s = 0;
    }
    return CVR_OK;
}

}  // extern "C"
