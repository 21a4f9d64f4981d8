// cvr_cg.hip -- conjugate gradients on the device (include/cvr_amd.h: cvr_cg_device, cvr_cg): the solver loop around the handle's SpMV, its fused
// vector kernels and a stop test without a host round trip per iteration.  Per step, beside the SpMV q = A p (run_spmv: cvr_spmv_device's path):
//   cg_pq_kernel         the partial sums of p . q
//   cg_update_kernel     alpha = r.z / p.q from those partials (summed in every workgroup, the same order everywhere: power_step_kernel's pattern);
//                        x += alpha p, r -= alpha q, z = minv .* r and the partial sums of r . r and r . z in one pass
//   cg_direction_kernel  r.r and r.z from those partials; the stop test; beta = r.z / r.z of the step before; p = z + beta p
// about eleven vector passes per step (p q | x p r q x r | z p p), all in 16-byte packets.  Sums are fp64 in a fixed tree (cvr_iter.hip's: strided share
// per thread, lanes by butterfly, wavefronts in order, workgroups' partials by a fixed tree again); no atomics, so a call gives the same bits every time.
// The scalars that outlive a kernel sit in a state cell (CgCell) that workgroup 0 writes: a kernel that finds the stop records it there and every later
// kernel of the batch returns without writing -- the result does not depend on how many steps the host enqueues between two read-backs.
// The host side is cvr_krylov.h's driver: the cell and the kernels are in cvr_cg_kernels.h (cvr_precond.hip's cvr_pcg_device runs them too), this file
// adds the step and the read-back.
// (The reference has no solver: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_cg_kernels.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

// the three vector launches of step k (the SpMV q = A p is enqueued in front of them); without a preconditioner z is r
template <typename T>
hipError_t launch_step(const Workspace<T> &w, T *x, const T *minv, long long n, bool al, int k, double rtol, hipStream_t st)
{
    launch(cg_pq_kernel<T>, st, w.p, w.q, n, w.part_pq, w.cell);
    with_flags([&](auto PRE, auto AL) { launch(cg_update_kernel<T, PRE, AL>, st, x, w.r, w.z, w.p, w.q, minv, n, w.part_pq, w.part, w.cell, k); }, minv != nullptr, al);
    with_flags([&](auto PRE) { launch(cg_direction_kernel<T, PRE>, st, w.p, PRE ? w.z : w.r, n, w.part, w.cell, k, rtol); }, minv != nullptr);
    return hipGetLastError();
}

// cvr_krylov.h's driver with CG's start, step and cell
template <typename T>
int cg_solve(cvr_handle *h, const T *b, T *x, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    const long long n = h->info.nrows;
    const size_t    vb = sizeof(T) * (size_t)n;
    const T        *minv = static_cast<const T *>(opt->minv_dev);
    const bool      al = (((uintptr_t)b | (uintptr_t)x | (uintptr_t)minv) & 15u) == 0;

    Arena        a;
    const size_t op = a.add(x_ext_bytes(h)), oq = a.add(y_ext_bytes(h)), orr = a.add(y_ext_bytes(h)), oz = a.add(minv ? vec_bytes(h) : 0);
    const size_t opq = a.add(sizeof(double) * kBlocks), opart = a.add(sizeof(double) * 3 * kBlocks), ocell = a.add(sizeof(CgCell));
    HIP_TRY(a.alloc());
    const Workspace<T> w{a.at<T>(op), a.at<T>(oq), a.at<T>(orr), minv ? a.at<T>(oz) : nullptr, a.at<double>(opq), a.at<double>(opart), a.at<CgCell>(ocell)};
    if (const int rc = a.begin(st)) return rc;

    // p = x0 for the moment (with its pad slot), r = b; r = b - A x0; then z, p and the start's sums
    if (const int rc = zero_pad_slot(w.p, vb, sizeof(T), st)) return rc;
    if (const int rc = start_residual(h, w.p, w.r, x, b, n, st)) return rc;
    int spmvs = 1;
    with_flags([&](auto PRE, auto AL) { launch(cg_init_kernel<T, PRE, AL>, st, b, minv, w.r, w.z, w.p, n, w.part); }, minv != nullptr, al);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cg_check_kernel, dim3(1), dim3(kThreads), 0, st, w.part, minv ? 1 : 0, opt->rtol, w.cell);
    HIP_TRY(hipGetLastError());

    CgCell cell{};
    const int rc = run_batches(
        opt,
        [&](int k) -> int {
            HIP_TRY(run_spmv(h, w.p, w.q, st));
            spmvs++;
            HIP_TRY(launch_step(w, x, minv, n, al, k, opt->rtol, st));
            return CVR_OK;
        },
        [&](int, bool *stopped) -> int {
            if (const int rc = read_cell(&cell, w.cell, sizeof(cell), st)) return rc;
            *stopped = cell.stop != 0;
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
int cg_device(cvr_handle *h, const void *b, void *x, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    if (const int rc = check_square_preprocessed(h, "cvr_cg", "conjugate gradients need")) return rc;
    Range range("cvr_cg_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) { return cg_solve(h, static_cast<const decltype(t) *>(b), static_cast<decltype(t) *>(x), opt, res, st); });
}

}  // namespace

extern "C" {

void cvr_cg_default_options(cvr_cg_options *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->max_iters = 1000;
    opt->check_every = 0;
    opt->rtol = 1e-8;
}

int cvr_cg_device(cvr_handle *h, const void *b_dev, void *x_dev, const cvr_cg_options *opt, cvr_cg_result *res, void *stream)
{
    if (const int rc = check_solver_args(h, b_dev, x_dev, opt, res)) return rc;
    return cg_device(h, b_dev, x_dev, opt, res, (hipStream_t)stream);
}

int cvr_cg(cvr_handle *h, const void *b_host, void *x_host, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, b_host, x_host, opt, res)) return rc;
    if (const int rc = check_square_preprocessed(h, "cvr_cg", "conjugate gradients need")) return rc;
    return solve_from_host(h, b_host, x_host, [&](const void *b, void *x, hipStream_t st) { return cg_device(h, b, x, opt, res, st); });
}

}  // extern "C"
