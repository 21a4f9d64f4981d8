// cvr_cg.hip -- conjugate gradients on the device (include/cvr_amd.h: cvr_cg_device, cvr_cg, cvr_pcg_device, cvr_pcg): the solver loop around the
// handle's SpMV, its fused vector kernels and a stop test without a host round trip per iteration.  Per step, beside the SpMV q = A p (run_spmv:
// cvr_spmv_device's path):
//   cg_pq_kernel         the partial sums of p . q
//   cg_update_kernel     alpha = r.z / p.q from those partials (summed in every workgroup, the same order everywhere: power_step_kernel's pattern);
//                        x += alpha p, r -= alpha q, z = minv .* r and the partial sums of r . r and r . z in one pass
//   cg_direction_kernel  r.r and r.z from those partials; the stop test; beta = r.z / r.z of the step before; p = z + beta p
// about eleven vector passes per step (p q | x p r q x r | z p p), all in 16-byte packets.  Sums are fp64 in a fixed tree (cvr_iter.hip's: strided share
// per thread, lanes by butterfly, wavefronts in order, workgroups' partials by a fixed tree again); no atomics, so a call gives the same bits every time.
// The scalars that outlive a kernel sit in a state cell (CgCell) that workgroup 0 writes: a kernel that finds the stop records it there and every later
// kernel of the batch returns without writing -- the result does not depend on how many steps the host enqueues between two read-backs.
// The preconditioner is an argument of the one solve function: none (z is r), the diagonal opt->minv_dev (fused into the update), or a cvr_precond
// object of either kind, whose apply (cvr_precond.h: precond_cg_apply) is enqueued between cg_update_kernel<T, false, AL> and
// cg_direction_kernel<T, true> and forms z with the partial sums of r . z -- 3 + 1 launches per step with block-Jacobi, 3 + degree launches and
// degree SpMVs with the Chebyshev kind.
// The host side is cvr_krylov.h's driver: the cell and the kernels are in cvr_cg_kernels.h, this file adds the step and the read-back.
// (The reference has no solver and no preconditioner: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_cg_kernels.h"
#include "cvr_precond.h"

namespace cvrh {
namespace krylov {
namespace {

// one workgroup: the start's sums into the state cell, and the stop test of the start vector.
// (The solver's one kernel that is no template: here and not in cvr_cg_kernels.h, so that a file which includes the header for the cell gets no copy.)
__global__ __launch_bounds__(kThreads) void cg_check_kernel(const double *__restrict__ part, int pre, double rtol, CgCell *__restrict__ cell)
{
    __shared__ double sh[3][kWaves];
    double s[3];
    sum_partials<3>(part, s, sh);
    if (threadIdx.x != 0) return;
    CgCell c;
    c.bb = s[2]; c.bnorm = sqrt(s[2]);
    c.rr = s[0]; c.rnorm = sqrt(s[0]);
    c.rz[0] = pre ? s[1] : s[0]; c.rz[1] = 0;
    c.stop = 0; c.status = CVR_CG_MAX_ITERS; c.iters = 0; c.zero_x = 0;
    if (c.bb == 0) { c.zero_x = 1; c.rr = 0; c.rnorm = 0; c.status = CVR_CG_CONVERGED; c.stop = 1; }
    // (an Inf in b makes both norms infinite, and Inf <= rtol * Inf holds: a residual that is not finite never counts as converged -- step 0 then
    // finds p . q not finite and records the breakdown)
    else if (c.rnorm <= rtol * c.bnorm && c.rnorm <= kDblMax) { c.status = CVR_CG_CONVERGED; c.stop = 1; }
    *cell = c;
}

}  // namespace
}  // namespace krylov
}  // namespace cvrh

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

// cvr_krylov.h's driver with CG's start, step and cell.  pc: a preconditioner object or null; with one, minv is null (the entry points see to it),
// so the kernels around its apply come in their forms without a diagonal, and the direction takes z and r . z from the apply
template <typename T>
int cg_solve(cvr_handle *h, const cvr_precond *pc, const T *b, T *x, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    const long long n = h->info.nrows;
    const size_t    vb = sizeof(T) * (size_t)n;
    const T        *minv = static_cast<const T *>(opt->minv_dev);
    const bool      al = (((uintptr_t)b | (uintptr_t)x | (uintptr_t)minv) & 15u) == 0, has_z = minv || pc;

    Arena        a;
    const size_t op = a.add(x_ext_bytes(h)), oq = a.add(y_ext_bytes(h)), orr = a.add(y_ext_bytes(h)), oz = a.add(has_z ? vec_bytes(h) : 0);
    const size_t opq = a.add(sizeof(double) * kBlocks), opart = a.add(sizeof(double) * 3 * kBlocks), ocell = a.add(sizeof(CgCell));
    HIP_TRY(a.alloc());
    const Workspace<T> w{a.at<T>(op), a.at<T>(oq), a.at<T>(orr), has_z ? a.at<T>(oz) : nullptr, a.at<double>(opq), a.at<double>(opart), a.at<CgCell>(ocell)};
    if (const int rc = a.begin(st)) return rc;

    // p = x0 for the moment (with its pad slot), r = b; r = b - A x0; then z, p and the start's sums (with an object: p = r, then z = M r, p = z and r . z)
    if (const int rc = zero_pad_slot(w.p, vb, sizeof(T), st)) return rc;
    if (const int rc = start_residual(h, w.p, w.r, x, b, n, st)) return rc;
    int spmvs = 1;
    with_flags([&](auto PRE, auto AL) { launch(cg_init_kernel<T, PRE, AL>, st, b, minv, (const T *)w.r, w.z, w.p, n, w.part); }, minv != nullptr, al);
    HIP_TRY(hipGetLastError());
    if (pc)
        if (const int rc = precond_cg_apply<T>(pc, w.r, w.z, w.p, w.part + kBlocks, w.cell, true, st, &spmvs)) return rc;
    hipLaunchKernelGGL(cg_check_kernel, dim3(1), dim3(kThreads), 0, st, w.part, has_z ? 1 : 0, opt->rtol, w.cell);
    HIP_TRY(hipGetLastError());

    CgCell cell{};
    const int rc = run_batches(
        opt,
        [&](int k) -> int {          // the SpMV q = A p and the three vector launches of step k, the object's apply between the last two
            HIP_TRY(run_spmv(h, w.p, w.q, st));
            spmvs++;
            launch(cg_pq_kernel<T>, st, w.p, w.q, n, w.part_pq, w.cell);
            with_flags([&](auto PRE, auto AL) { launch(cg_update_kernel<T, PRE, AL>, st, x, w.r, w.z, w.p, w.q, minv, n, w.part_pq, w.part, w.cell, k); }, minv != nullptr, al);
            if (pc) {
                HIP_TRY(hipGetLastError());
                if (const int rc = precond_cg_apply<T>(pc, w.r, w.z, w.p, w.part + kBlocks, w.cell, false, st, &spmvs)) return rc;
            }
            with_flags([&](auto PRE) { launch(cg_direction_kernel<T, PRE>, st, w.p, PRE ? w.z : w.r, n, w.part, w.cell, k, opt->rtol); }, has_z);
            HIP_TRY(hipGetLastError());
            return CVR_OK;
        },
        [&](int, bool *stopped) -> int {
            if (const int rc = read_cell(&cell, w.cell, sizeof(cell), st)) return rc;
            *stopped = cell.stop != 0;
            return CVR_OK;
        });
    if (rc) return rc;
    return finish_solve(a, st, x, vb, cell, spmvs, res);
}

// behind the argument checks (and, with an object, behind those of the handle and the pair: check_pcg)
int cg_device(cvr_handle *h, const cvr_precond *pc, const void *b, void *x, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    if (!pc)
        if (const int rc = check_square_preprocessed(h, "cvr_cg", "conjugate gradients need")) return rc;
    Range range(pc ? "cvr_pcg_device" : "cvr_cg_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) { return cg_solve(h, pc, static_cast<const decltype(t) *>(b), static_cast<decltype(t) *>(x), opt, res, st); });
}

// what cvr_pcg_device and cvr_pcg check: the solver's arguments and the object's before the handle is looked at, then the handle and the pair
int check_pcg(const cvr_handle *h, const cvr_precond *p, const void *b, const void *x, const cvr_cg_options *opt, const cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, b, x, opt, res)) return rc;
    if (const int rc = check_precond_args(p, opt, "cvr_pcg")) return rc;
    if (const int rc = check_square_preprocessed(h, "cvr_pcg", "conjugate gradients need")) return rc;
    return check_precond_pair(h, p, "cvr_pcg");
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
    return cg_device(h, nullptr, b_dev, x_dev, opt, res, (hipStream_t)stream);
}

int cvr_cg(cvr_handle *h, const void *b_host, void *x_host, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, b_host, x_host, opt, res)) return rc;
    if (const int rc = check_square_preprocessed(h, "cvr_cg", "conjugate gradients need")) return rc;
    return solve_from_host(h, b_host, x_host, [&](const void *b, void *x, hipStream_t st) { return cg_device(h, nullptr, b, x, opt, res, st); });
}

int cvr_pcg_device(cvr_handle *h, const cvr_precond *p, const void *b_dev, void *x_dev, const cvr_cg_options *opt, cvr_cg_result *res, void *stream)
{
    if (const int rc = check_pcg(h, p, b_dev, x_dev, opt, res)) return rc;
    return cg_device(h, p, b_dev, x_dev, opt, res, (hipStream_t)stream);
}

int cvr_pcg(cvr_handle *h, const cvr_precond *p, const void *b_host, void *x_host, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_pcg(h, p, b_host, x_host, opt, res)) return rc;
    return solve_from_host(h, b_host, x_host, [&](const void *b, void *x, hipStream_t st) { return cg_device(h, p, b, x, opt, res, st); });
}

}  // extern "C"
