// cvr_bicgstab.hip -- BiCGSTAB on the device for nonsymmetric A (include/cvr_amd.h: cvr_bicgstab_device, cvr_bicgstab): cvr_cg.hip's plan with the
// other recurrence.  Right-preconditioned, shadow residual r^ = r0; per step two SpMVs through run_spmv (cvr_spmv_device's path) and five vector launches:
//   v = A p^
//   bicg_rv_kernel         the partial sums of r^ . v
//   bicg_s_kernel          alpha = rho / (r^ . v) from those partials (summed in every workgroup, the same order everywhere); s = r - alpha v,
//                          s^ = minv .* s and the partial sums of s . s
//   t = A s^
//   bicg_half_kernel       ||s|| <= rtol ||b||: x += alpha p^, the stop recorded (the half step); else the partial sums of t . s and t . t
//   bicg_update_kernel     omega = (t . s) / (t . t); x += alpha p^ + omega s^, r = s - omega t and the partial sums of r . r and r^ . r
//   bicg_direction_kernel  the stop test; beta = (rho' / rho)(alpha / omega); p = r + beta (p - omega v), p^ = minv .* p
// 18 vector passes per step (r^ v | r v s | t s | x p s t r^ x r | r p v p), 23 with a preconditioner, all in 16-byte packets; the sums, the grid and
// the packet helpers are cvr_krylov.h's, so a call gives the same bits every time.  The scalars that outlive a kernel sit in a state cell (BiCell) that
// workgroup 0 writes: the kernel that finds a stop records it there and every later kernel of the batch returns without writing -- the result does not
// depend on how many steps the host enqueues between two read-backs.
// The host side is cvr_krylov.h's driver: this file adds the cell, the kernels, the step and the read-back.
// (The reference has no solver: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_bicg_kernels.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

// the library's buffers of one call: p and s (x_ext each: SpMV inputs without a preconditioner), p^ and s^ (x_ext each, with one),
// v, t and r (y_ext each: r takes the scaled product), r^, two sets of partial sums that the kernels use in turn, the cell
template <typename T>
struct Workspace {
    T      *p, *s, *phat, *shat, *v, *t, *r, *rhat;
    double *part_a, *part_b;
    BiCell *cell;
};

// step k up to the second SpMV: r^ . v, then alpha and s (the SpMV v = A p^ is enqueued in front).  (A kernel whose only caller's array is minv
// has no <T, false, false> form: AL || !PRE.)
template <typename T>
hipError_t launch_first_half(const Workspace<T> &w, const T *minv, long long n, bool al, int k, hipStream_t st)
{
    launch(bicg_rv_kernel<T>, st, w.rhat, w.v, n, w.part_a, w.cell);
    with_flags([&](auto PRE, auto AL) { launch(bicg_s_kernel<T, PRE, AL || !PRE>, st, w.r, w.v, minv, w.s, w.shat, n, w.part_a, w.part_b, w.cell, k); }, minv != nullptr, al);
    return hipGetLastError();
}

// the rest of step k (the SpMV t = A s^ is enqueued in front): the half-step test, the update, the stop test and the new direction
template <typename T>
hipError_t launch_second_half(const Workspace<T> &w, T *x, const T *minv, long long n, bool al, int k, double rtol, hipStream_t st)
{
    const T *ph = minv ? w.phat : w.p, *sh = minv ? w.shat : w.s;
    with_flags([&](auto AL) { launch(bicg_half_kernel<T, AL>, st, x, ph, w.s, w.t, n, w.part_b, w.part_a, w.cell, k, rtol); }, al);
    with_flags([&](auto PRE, auto AL) { launch(bicg_update_kernel<T, PRE, AL>, st, x, w.r, ph, sh, w.s, w.t, w.rhat, n, w.part_a, w.part_b, w.cell, k); }, minv != nullptr, al);
    with_flags([&](auto PRE, auto AL) { launch(bicg_direction_kernel<T, PRE, AL || !PRE>, st, w.p, w.phat, w.r, w.v, minv, n, w.part_b, w.cell, k, rtol); }, minv != nullptr, al);
    return hipGetLastError();
}

int check_handle(const cvr_handle *h) { return check_square_preprocessed(h, "cvr_bicgstab", "BiCGSTAB needs"); }

// cvr_krylov.h's driver with BiCGSTAB's start, step and cell
template <typename T>
int bicgstab_solve(cvr_handle *h, const T *b, T *x, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    const long long n = h->info.nrows;
    const size_t    vb = sizeof(T) * (size_t)n;
    const T        *minv = static_cast<const T *>(opt->minv_dev);
    const bool      al = (((uintptr_t)b | (uintptr_t)x | (uintptr_t)minv) & 15u) == 0;

    Arena        a;
    const size_t nx = x_ext_bytes(h), ny = y_ext_bytes(h), nh = minv ? nx : 0, npart = sizeof(double) * 2 * kBlocks;
    const size_t op = a.add(nx), os = a.add(nx), ophat = a.add(nh), oshat = a.add(nh), ov = a.add(ny), ot = a.add(ny), orr = a.add(ny), orhat = a.add(vec_bytes(h));
    const size_t oa = a.add(npart), ob = a.add(npart), ocell = a.add(sizeof(BiCell));
    HIP_TRY(a.alloc());
    const Workspace<T> w{a.at<T>(op), a.at<T>(os), minv ? a.at<T>(ophat) : nullptr, minv ? a.at<T>(oshat) : nullptr, a.at<T>(ov), a.at<T>(ot), a.at<T>(orr), a.at<T>(orhat),
                         a.at<double>(oa), a.at<double>(ob), a.at<BiCell>(ocell)};
    if (const int rc = a.begin(st)) return rc;

    // the pad slots of the SpMV inputs; p = x0 for the moment, r = b; r = b - A x0; then r^, p, p^ and the start's sums
    for (T *q : {w.p, w.s, w.phat, w.shat})
        if (q)
            if (const int rc = zero_pad_slot(q, vb, sizeof(T), st)) return rc;
    if (const int rc = start_residual(h, w.p, w.r, x, b, n, st)) return rc;
    int spmvs = 1;
    with_flags([&](auto PRE, auto AL) { launch(bicg_init_kernel<T, PRE, AL>, st, b, minv, w.r, w.rhat, w.p, w.phat, n, w.part_b); }, minv != nullptr, al);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bicg_check_kernel, dim3(1), dim3(kThreads), 0, st, w.part_b, opt->rtol, w.cell);
    HIP_TRY(hipGetLastError());

    const T  *ph = minv ? w.phat : w.p, *sh = minv ? w.shat : w.s;
    BiCell    cell{};
    const int rc = run_batches(
        opt,
        [&](int k) -> int {
            HIP_TRY(run_spmv(h, ph, w.v, st));
            HIP_TRY(launch_first_half(w, minv, n, al, k, st));
            HIP_TRY(run_spmv(h, sh, w.t, st));
            HIP_TRY(launch_second_half(w, x, minv, n, al, k, opt->rtol, st));
            spmvs += 2;
            return CVR_OK;
        },
        [&](int, bool *stopped) -> int {
            if (const int rc = read_cell(&cell, w.cell, sizeof(cell), st)) return rc;
            *stopped = cell.stop || cell.half;
            return CVR_OK;
        });
    if (rc) return rc;
    if (cell.zero_x && n) HIP_TRY(hipMemsetAsync(x, 0, vb, st));
    double seconds = 0;
    if (const int rc = a.seconds(st, &seconds)) return rc;
    fill_result(res, cell.iters, cell.status, spmvs, cell.rnorm, cell.bnorm, seconds);
    return CVR_OK;
}

// behind the argument checks
int bicgstab_device(cvr_handle *h, const void *b, void *x, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    if (const int rc = check_handle(h)) return rc;
    Range range("cvr_bicgstab_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) { return bicgstab_solve(h, static_cast<const decltype(t) *>(b), static_cast<decltype(t) *>(x), opt, res, st); });
}

}  // namespace

extern "C" {

int cvr_bicgstab_device(cvr_handle *h, const void *b_dev, void *x_dev, const cvr_cg_options *opt, cvr_cg_result *res, void *stream)
{
    if (const int rc = check_solver_args(h, b_dev, x_dev, opt, res)) return rc;
    return bicgstab_device(h, b_dev, x_dev, opt, res, (hipStream_t)stream);
}

int cvr_bicgstab(cvr_handle *h, const void *b_host, void *x_host, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, b_host, x_host, opt, res)) return rc;
    if (const int rc = check_handle(h)) return rc;
    return solve_from_host(h, b_host, x_host, [&](const void *b, void *x, hipStream_t st) { return bicgstab_device(h, b, x, opt, res, st); });
}

}  // extern "C"
