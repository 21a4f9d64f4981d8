// cvr_pbicgstab.hip -- BiCGSTAB preconditioned by a block-Jacobi object (include/cvr_amd.h: cvr_pbicgstab_device, cvr_pbicgstab): cvr_bicgstab.hip's
// solver with p^ = W p and s^ = W s by the object's apply (cvr_precond.h: apply_pack) in place of a product with a diagonal.  An element of p^ needs its
// whole block of p, so each apply is a launch of its own behind the kernel that writes p or s; per step two SpMVs and seven vector launches:
//   v = A p^
//   bicg_rv_kernel                          the partial sums of r^ . v
//   bicg_s_kernel<T, false, true>           alpha; s = r - alpha v and the partial sums of s . s
//   pbicg_apply_kernel                      s^ = W s
//   t = A s^
//   bicg_half_kernel                        the half-step test (x += alpha p^) or the partial sums of t . s and t . t
//   bicg_update_kernel<T, true, AL>         omega; x += alpha p^ + omega s^ (s^ from its own buffer), r = s - omega t, the partial sums of r . r and r^ . r
//   bicg_direction_kernel<T, false, true>   the stop test; beta; p = r + beta (p - omega v)
//   pbicg_apply_kernel                      p^ = W p
// The bicg_* kernels are cvr_bicg_kernels.h's, the ones cvr_bicgstab_device runs, in the forms that take no diagonal; the apply returns at its top once
// the cell holds a stop or a half-step stop, as they do, so the result does not depend on how many steps the host enqueues between two read-backs.
// (The reference has no solver and no preconditioner: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_bicg_kernels.h"
#include "cvr_precond.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

// z = W r on the solvers' grid, r and z the library's buffers (16-byte aligned); nothing is written once the cell holds a stop or a half-step stop
// (no workgroup of this kernel sets either)
template <typename T>
__global__ __launch_bounds__(kThreads) void pbicg_apply_kernel(const T *__restrict__ wt, int bs, const T *__restrict__ r, T *__restrict__ z, long long n,
                                                               const BiCell *__restrict__ cell)
{
    if (cell->stop | cell->half) return;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T zv[kPack<T>];
        apply_pack<T>(wt, bs, r, n, e, (int)cnt, zv);
        store_pack<T, true>(z, e, (int)cnt, zv);
    }
}

// the library's buffers of one call: p, s, p^ and s^ (x_ext each: p^ and s^ are the SpMV inputs), v, t and r (y_ext each: r takes the scaled product),
// r^, two sets of partial sums that the kernels use in turn, the cell
template <typename T>
struct Workspace {
    T      *p, *s, *phat, *shat, *v, *t, *r, *rhat;
    double *part_a, *part_b;
    BiCell *cell;
};

template <typename T>
void launch_apply(const Workspace<T> &w, const cvr_precond *pc, const T *from, T *to, long long n, hipStream_t st)
{
    launch(pbicg_apply_kernel<T>, st, static_cast<const T *>(pc->d_w), (int)pc->bs, from, to, n, (const BiCell *)w.cell);
}

// step k up to the second SpMV (v = A p^ is enqueued in front): r^ . v, alpha and s, s^
template <typename T>
hipError_t launch_first_half(const Workspace<T> &w, const cvr_precond *pc, long long n, int k, hipStream_t st)
{
    launch(bicg_rv_kernel<T>, st, w.rhat, w.v, n, w.part_a, w.cell);
    launch(bicg_s_kernel<T, false, true>, st, w.r, w.v, (const T *)nullptr, w.s, w.shat, n, w.part_a, w.part_b, w.cell, k);
    launch_apply(w, pc, w.s, w.shat, n, st);
    return hipGetLastError();
}

// the rest of step k (t = A s^ is enqueued in front): the half-step test, the update, the stop test and the new direction, p^
template <typename T>
hipError_t launch_second_half(const Workspace<T> &w, const cvr_precond *pc, T *x, long long n, bool al, int k, double rtol, hipStream_t st)
{
    with_flags([&](auto AL) { launch(bicg_half_kernel<T, AL>, st, x, w.phat, w.s, w.t, n, w.part_b, w.part_a, w.cell, k, rtol); }, al);
    with_flags([&](auto AL) { launch(bicg_update_kernel<T, true, AL>, st, x, w.r, w.phat, w.shat, w.s, w.t, w.rhat, n, w.part_a, w.part_b, w.cell, k); }, al);
    launch(bicg_direction_kernel<T, false, true>, st, w.p, w.phat, w.r, w.v, (const T *)nullptr, n, w.part_b, w.cell, k, rtol);
    launch_apply(w, pc, w.p, w.phat, n, st);
    return hipGetLastError();
}

// cvr_bicgstab.hip's bicgstab_solve with W in place of minv
template <typename T>
int pbicgstab_solve(cvr_handle *h, const cvr_precond *pc, const T *b, T *x, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    const long long n = h->info.nrows;
    const size_t    vb = sizeof(T) * (size_t)n;
    const bool      al = (((uintptr_t)b | (uintptr_t)x) & 15u) == 0;

    Arena        a;
    const size_t nx = x_ext_bytes(h), ny = y_ext_bytes(h), npart = sizeof(double) * 2 * kBlocks;
    const size_t op = a.add(nx), os = a.add(nx), ophat = a.add(nx), oshat = a.add(nx), ov = a.add(ny), ot = a.add(ny), orr = a.add(ny), orhat = a.add(vec_bytes(h));
    const size_t oa = a.add(npart), ob = a.add(npart), ocell = a.add(sizeof(BiCell));
    HIP_TRY(a.alloc());
    const Workspace<T> w{a.at<T>(op), a.at<T>(os), a.at<T>(ophat), a.at<T>(oshat), a.at<T>(ov), a.at<T>(ot), a.at<T>(orr), a.at<T>(orhat),
                         a.at<double>(oa), a.at<double>(ob), a.at<BiCell>(ocell)};
    if (const int rc = a.begin(st)) return rc;

    // the pad slots of the SpMV inputs; p = x0 for the moment, r = b; r = b - A x0; then r^, p and the start's sums, the cell, p^ = W p
    for (T *q : {w.p, w.phat, w.shat})
        if (const int rc = zero_pad_slot(q, vb, sizeof(T), st)) return rc;
    if (const int rc = start_residual(h, w.p, w.r, x, b, n, st)) return rc;
    int spmvs = 1;
    with_flags([&](auto AL) { launch(bicg_init_kernel<T, false, AL>, st, b, (const T *)nullptr, w.r, w.rhat, w.p, w.phat, n, w.part_b); }, al);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bicg_check_kernel, dim3(1), dim3(kThreads), 0, st, w.part_b, opt->rtol, w.cell);
    HIP_TRY(hipGetLastError());
    launch_apply(w, pc, w.p, w.phat, n, st);
    HIP_TRY(hipGetLastError());

    BiCell    cell{};
    const int rc = run_batches(
        opt,
        [&](int k) -> int {
            HIP_TRY(run_spmv(h, w.phat, w.v, st));
            HIP_TRY(launch_first_half(w, pc, n, k, st));
            HIP_TRY(run_spmv(h, w.shat, w.t, st));
            HIP_TRY(launch_second_half(w, pc, x, n, al, k, opt->rtol, st));
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

// what the entry points check before any device work and before the handle is looked at
int check_args(const void *h, const cvr_precond *p, const void *b, const void *x, const cvr_cg_options *opt, const cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, b, x, opt, res)) return rc;
    return check_precond_args(p, opt, "cvr_pbicgstab");
}

// ... and what they ask of the handle and of the pair
int check_handle(const cvr_handle *h, const cvr_precond *p)
{
    if (const int rc = check_square_preprocessed(h, "cvr_pbicgstab", "BiCGSTAB needs")) return rc;
    if (const int rc = check_precond_pair(h, p, "cvr_pbicgstab")) return rc;
    return check_block_jacobi(p, "cvr_pbicgstab");
}

int pbicgstab_device(cvr_handle *h, const cvr_precond *p, const void *b, void *x, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    Range range("cvr_pbicgstab_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) { return pbicgstab_solve(h, p, static_cast<const decltype(t) *>(b), static_cast<decltype(t) *>(x), opt, res, st); });
}

}  // namespace

extern "C" {

int cvr_pbicgstab_device(cvr_handle *h, const cvr_precond *p, const void *b_dev, void *x_dev, const cvr_cg_options *opt, cvr_cg_result *res, void *stream)
{
    if (const int rc = check_args(h, p, b_dev, x_dev, opt, res)) return rc;
    if (const int rc = check_handle(h, p)) return rc;
    return pbicgstab_device(h, p, b_dev, x_dev, opt, res, (hipStream_t)stream);
}

int cvr_pbicgstab(cvr_handle *h, const cvr_precond *p, const void *b_host, void *x_host, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_args(h, p, b_host, x_host, opt, res)) return rc;
    if (const int rc = check_handle(h, p)) return rc;
    return solve_from_host(h, b_host, x_host, [&](const void *b, void *x, hipStream_t st) { return pbicgstab_device(h, p, b, x, opt, res, st); });
}

}  // extern "C"
