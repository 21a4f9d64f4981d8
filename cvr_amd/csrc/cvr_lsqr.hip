// cvr_lsqr.hip -- LSQR (Paige & Saunders) on the device for min ||b - A x||_2 with A of any shape and rank, Tikhonov damping included
// (include/cvr_amd.h: cvr_lsqr_device, cvr_lsqr): cvr_cg.hip's plan with the Golub-Kahan bidiagonalisation.  Two handles, A (m x n) and A^T (n x m,
// usually cvr_options.transpose = 1 on the same CSR); per step one SpMV on each through run_spmv (cvr_spmv_device's path) and three vector launches:
//   q = A v
//   lsqr_u_kernel      over m: u^ = q - (alpha / beta) u^ and the partial sums of u^ . u^
//   p = A^T u^
//   lsqr_v_kernel      over n: beta' = ||u^|| from those partials; v^ = p / beta' - beta' v in v's place and the partial sums of v^ . v^
//   lsqr_x_kernel      over n: alpha' = ||v^||, the two rotations, the breakdown test, x += (phi / rho) w, the norm estimates and the stop tests;
//                      not stopped: v = v^ / alpha', w = v - (theta / rho) w
// u is kept unnormalised (u^ = beta u): normalising it would need ||u^|| before the pass that divides by it -- a fourth launch over m --, while
// A^T u^ = beta A^T u lets the division ride on lsqr_v_kernel's pass over n, which has the sum by then.  12 vector passes per step (q u u | p v v |
// x w v x v w, less four at the stop), 3 over m and 9 over n, all in 16-byte packets; the sums, the grid and the packet helpers are cvr_krylov.h's, so a call gives the same
// bits every time.  u^ is at once the output of A's scaled product (the start: u^ = b - A x0) and the input of A^T's product: its buffer has the
// larger of the two sizes and its element m is zeroed behind the scaled product, whose scratch tail begins there.
// The scalars that outlive a kernel sit in a state cell (LsqrCell) that workgroup 0 writes, double-buffered by step parity where a workgroup reads
// what another one of the same launch writes; the kernel that finds a stop records it there and every later kernel of the batch returns without
// writing -- the result does not depend on how many steps the host enqueues between two read-backs.
// The host side is cvr_krylov.h's driver but for its square-matrix helpers: the sizes here come from two handles.
// (The reference has no solver: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_lsqr_kernels.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

// the library's buffers of one call: v (A's x_ext: an SpMV input, x0 at the start), u^ (A's y_ext and A^T's x_ext), q (A's y_ext), p (A^T's y_ext),
// w (n values), three sets of partial sums (u^ . u^ | v^ . v^ | -; at the start b . b | u^ . u^ | v^ . v^), the cell
template <typename T>
struct Workspace {
    T        *v, *u, *q, *p, *w;
    double   *part;
    LsqrCell *cell;
};

size_t elems_bytes(const cvr_handle *h, std::initializer_list<int64_t> elems) { return h->vsz * (size_t)std::max<int64_t>(std::max(elems), 1); }

int check_damp(double damp)
{
    if (!(damp >= 0) || !std::isfinite(damp)) return fail(CVR_ERR_INVALID, "cvr_lsqr: damp = %g: must be finite and not negative", damp);
    return CVR_OK;
}

// what comes before any device work and before a handle is looked at
int check_args(const cvr_handle *a, const cvr_handle *at, const void *b, const void *x, double damp, const cvr_cg_options *opt, const cvr_cg_result *res)
{
    if (const int rc = check_solver_args(a, b, x, opt, res)) return rc;
    if (!at) return fail(CVR_ERR_INVALID, "cvr_lsqr: null handle of the transpose");
    if (opt->minv_dev) return fail(CVR_ERR_INVALID, "cvr_lsqr takes no preconditioner: opt->minv_dev must be NULL");
    return check_damp(damp);
}

int check_handles(const cvr_handle *a, const cvr_handle *at)
{
    if (!a->converted || !at->converted) return fail(CVR_ERR_STATE, "cvr_lsqr before cvr_preprocess");
    if (at->info.nrows != a->info.ncols || at->info.ncols != a->info.nrows)
        return fail(CVR_ERR_INVALID, "cvr_lsqr: A is %lld x %lld, the handle of its transpose %lld x %lld", (long long)a->info.nrows, (long long)a->info.ncols,
                    (long long)at->info.nrows, (long long)at->info.ncols);
    if (a->vsz != at->vsz) return fail(CVR_ERR_INVALID, "cvr_lsqr: the two handles hold different value types");
    if (a->device != at->device) return fail(CVR_ERR_INVALID, "cvr_lsqr: the two handles are on devices %d and %d", a->device, at->device);
    return CVR_OK;
}

template <typename T>
int lsqr_solve(cvr_handle *a, cvr_handle *at, const T *b, T *x, double damp, const cvr_cg_options *opt, cvr_cg_result *res, cvr_lsqr_info *info, hipStream_t st)
{
    const long long m = a->info.nrows, n = a->info.ncols;
    const bool      al = (((uintptr_t)b | (uintptr_t)x) & 15u) == 0;

    Arena        ar;
    const size_t ov = ar.add(elems_bytes(a, {a->info.x_elems, n + 1})), ou = ar.add(elems_bytes(a, {a->info.yext_elems, at->info.x_elems, m + 1}));
    const size_t oq = ar.add(elems_bytes(a, {a->info.yext_elems, m})), op = ar.add(elems_bytes(a, {at->info.yext_elems, n})), ow = ar.add(elems_bytes(a, {n}));
    const size_t opart = ar.add(sizeof(double) * 3 * kBlocks), ocell = ar.add(sizeof(LsqrCell));
    HIP_TRY(ar.alloc());
    const Workspace<T> w{ar.at<T>(ov), ar.at<T>(ou), ar.at<T>(oq), ar.at<T>(op), ar.at<T>(ow), ar.at<double>(opart), ar.at<LsqrCell>(ocell)};
    if (const int rc = ar.begin(st)) return rc;

    // v = x0 for the moment, u^ = b; u^ = b - A x0, whose scratch tail begins at u^[m]: the pad slot of A^T's input; the start's sums; p = A^T u^; v, w
    if (const int rc = zero_pad_slot(w.v, sizeof(T) * (size_t)n, sizeof(T), st)) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(w.v, x, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, st));
    if (m) HIP_TRY(hipMemcpyAsync(w.u, b, sizeof(T) * (size_t)m, hipMemcpyDeviceToDevice, st));
    if (const int rc = spmv_scaled_enqueue(a, -1.0, w.v, 1.0, w.u, st)) return rc;
    if (const int rc = zero_pad_slot(w.u, sizeof(T) * (size_t)m, sizeof(T), st)) return rc;
    with_flags([&](auto AL) { launch(lsqr_init_kernel<T, AL>, st, b, w.u, m, w.part); }, al);
    HIP_TRY(hipGetLastError());
    HIP_TRY(run_spmv(at, w.u, w.p, st));
    int spmvs = 2;
    launch(lsqr_v0_kernel<T>, st, w.p, w.v, n, w.part, w.part + 2 * kBlocks, w.cell, opt->rtol);          // (reads sets 0 and 1: its own sums go to a third)
    launch(lsqr_start_kernel<T>, st, w.v, w.w, n, w.part + 2 * kBlocks, w.cell);
    HIP_TRY(hipGetLastError());

    LsqrCell  cell{};
    const int rc = run_batches(
        opt,
        [&](int k) -> int {
            HIP_TRY(run_spmv(a, w.v, w.q, st));
            launch(lsqr_u_kernel<T>, st, w.q, w.u, m, w.part, w.cell, k);
            HIP_TRY(hipGetLastError());
            HIP_TRY(run_spmv(at, w.u, w.p, st));
            launch(lsqr_v_kernel<T>, st, w.p, w.v, n, w.part, w.part + kBlocks, w.cell);
            with_flags([&](auto AL) { launch(lsqr_x_kernel<T, AL>, st, x, w.v, w.w, n, w.part, w.cell, k, damp, opt->rtol); }, al);
            HIP_TRY(hipGetLastError());
            spmvs += 2;
            return CVR_OK;
        },
        [&](int, bool *stopped) -> int {
            if (const int rc = read_cell(&cell, w.cell, sizeof(cell), st)) return rc;
            *stopped = cell.stop != 0;
            return CVR_OK;
        });
    if (rc) return rc;
    if (const int rc = finish_solve(ar, st, x, sizeof(T) * (size_t)n, cell, spmvs, res)) return rc;
    if (info) {
        memset(info, 0, sizeof(*info));
        info->arnorm = cell.arnorm;
        info->anorm = cell.anorm;
        info->stop_test = cell.stop_test;
    }
    return CVR_OK;
}

// behind the argument checks
int lsqr_device(cvr_handle *a, cvr_handle *at, const void *b, void *x, double damp, const cvr_cg_options *opt, cvr_cg_result *res, cvr_lsqr_info *info, hipStream_t st)
{
    if (const int rc = check_handles(a, at)) return rc;
    Range range("cvr_lsqr_device");
    HIP_TRY(hipSetDevice(a->device));
    return with_value_type(a, [&](auto t) { return lsqr_solve(a, at, static_cast<const decltype(t) *>(b), static_cast<decltype(t) *>(x), damp, opt, res, info, st); });
}

}  // namespace

extern "C" {

int cvr_lsqr_device(cvr_handle *a, cvr_handle *at, const void *b_dev, void *x_dev, double damp, const cvr_cg_options *opt, cvr_cg_result *res, cvr_lsqr_info *info,
                    void *stream)
{
    if (const int rc = check_args(a, at, b_dev, x_dev, damp, opt, res)) return rc;
    return lsqr_device(a, at, b_dev, x_dev, damp, opt, res, info, (hipStream_t)stream);
}

// b (m values) and x (n values) ride on A's own vectors: d_y holds at least nrows values, d_x ncols + 1
int cvr_lsqr(cvr_handle *a, cvr_handle *at, const void *b_host, void *x_host, double damp, const cvr_cg_options *opt, cvr_cg_result *res, cvr_lsqr_info *info)
{
    if (const int rc = check_args(a, at, b_host, x_host, damp, opt, res)) return rc;
    if (const int rc = check_handles(a, at)) return rc;
    HIP_TRY(hipSetDevice(a->device));
    const size_t bb = a->vsz * (size_t)a->info.nrows, xb = a->vsz * (size_t)a->info.ncols;
    if (xb) HIP_TRY(hipMemcpyAsync(a->d_x, x_host, xb, hipMemcpyHostToDevice, a->stream));
    if (bb) HIP_TRY(hipMemcpyAsync(a->d_y, b_host, bb, hipMemcpyHostToDevice, a->stream));
    if (const int rc = lsqr_device(a, at, a->d_y, a->d_x, damp, opt, res, info, a->stream)) return rc;
    if (xb) HIP_TRY(hipMemcpyAsync(x_host, a->d_x, xb, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    return CVR_OK;
}

}  // extern "C"
