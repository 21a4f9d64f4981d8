// cvr_bicgstab.hip -- BiCGSTAB on the device for nonsymmetric A (include/cvr_amd.h: cvr_bicgstab_device, cvr_bicgstab, cvr_pbicgstab_device,
// cvr_pbicgstab): cvr_cg.hip's plan with the other recurrence.  Right-preconditioned, shadow residual r^ = r0; per step two SpMVs through run_spmv
// (cvr_spmv_device's path) and five vector launches:
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
// The preconditioner is an argument of the one solve function: none, the diagonal opt->minv_dev (fused into the kernels above), or a block-Jacobi
// object (cvr_pbicgstab*).  An element of W p needs its whole block of p, so with an object s^ = W s and p^ = W p are launches of their own
// (pbicg_apply_kernel, by cvr_precond.h's apply_pack) behind bicg_s_kernel and bicg_direction_kernel, which then run in their forms without a
// diagonal, <T, false, true>; bicg_update_kernel<T, true, AL> reads s^ from its own buffer: seven vector launches per step.  The apply returns at its
// top once the cell holds a stop or a half-step stop, as the bicg_* kernels do.  An ILU(0) object (cvr_ilu0.hip) is taken in the same two places: its
// apply is launches_lower + launches_upper launches of its own under the same rule.
// The host side is cvr_krylov.h's driver: this file adds the step and the read-back; the cell and the bicg_* kernels are in cvr_bicg_kernels.h.
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

// the library's buffers of one call: p and s (x_ext each: the SpMV inputs without a preconditioner), p^ and s^ (x_ext each, with one: then they are
// the SpMV inputs), v, t and r (y_ext each: r takes the scaled product), r^, two sets of partial sums that the kernels use in turn, the cell
template <typename T>
struct Workspace {
    T      *p, *s, *phat, *shat, *v, *t, *r, *rhat;
    double *part_a, *part_b;
    BiCell *cell;
};

// to = W from, with an object; an ILU(0) object's apply is its own launches (cvr_precond.h: ilu0_apply), under the same rule: behind a stop or a
// half-step stop nothing is written
template <typename T>
void launch_apply(const Workspace<T> &w, const cvr_precond *pc, const T *from, T *to, long long n, hipStream_t st)
{
    if (pc->kind == kPrecondIlu0) {
        Ilu0Gate gate;
        gate.stop = &w.cell->stop;          // stop and half: two adjacent words
        gate.nstop = 2;
        (void)ilu0_apply<T, T>(pc, from, to, gate, st);          // (a launch error stays in hipGetLastError for the caller)
        return;
    }
    launch(pbicg_apply_kernel<T>, st, static_cast<const T *>(pc->d_w), (int)pc->bs, from, to, n, (const BiCell *)w.cell);
}
static_assert(offsetof(BiCell, half) == offsetof(BiCell, stop) + sizeof(int32_t), "the gate reads stop and half as two adjacent words");

// step k up to the second SpMV: r^ . v, then alpha and s, s^ (the SpMV v = A p^ is enqueued in front).  (A kernel whose only caller's array is minv
// has no <T, false, false> form: AL || !PRE.  With an object minv is null.)
template <typename T>
hipError_t launch_first_half(const Workspace<T> &w, const cvr_precond *pc, const T *minv, long long n, bool al, int k, hipStream_t st)
{
    launch(bicg_rv_kernel<T>, st, w.rhat, w.v, n, w.part_a, w.cell);
    with_flags([&](auto PRE, auto AL) { launch(bicg_s_kernel<T, PRE, AL || !PRE>, st, w.r, w.v, minv, w.s, w.shat, n, w.part_a, w.part_b, w.cell, k); }, minv != nullptr, al);
    if (pc) launch_apply(w, pc, w.s, w.shat, n, st);
    return hipGetLastError();
}

// the rest of step k (the SpMV t = A s^ is enqueued in front): the half-step test, the update (s^ from its own buffer with either preconditioner),
// the stop test and the new direction, p^
template <typename T>
hipError_t launch_second_half(const Workspace<T> &w, const cvr_precond *pc, T *x, const T *minv, long long n, bool al, int k, double rtol, hipStream_t st)
{
    const T *ph = w.phat ? w.phat : w.p, *sh = w.shat ? w.shat : w.s;
    with_flags([&](auto AL) { launch(bicg_half_kernel<T, AL>, st, x, ph, w.s, w.t, n, w.part_b, w.part_a, w.cell, k, rtol); }, al);
    with_flags([&](auto PRE, auto AL) { launch(bicg_update_kernel<T, PRE, AL>, st, x, w.r, ph, sh, w.s, w.t, w.rhat, n, w.part_a, w.part_b, w.cell, k); }, w.shat != nullptr, al);
    with_flags([&](auto PRE, auto AL) { launch(bicg_direction_kernel<T, PRE, AL || !PRE>, st, w.p, w.phat, w.r, w.v, minv, n, w.part_b, w.cell, k, rtol); }, minv != nullptr, al);
    if (pc) launch_apply(w, pc, w.p, w.phat, n, st);
    return hipGetLastError();
}

// cvr_krylov.h's driver with BiCGSTAB's start, step and cell.  pc: a block-Jacobi object or null; with one, minv is null (the entry points see to it)
template <typename T>
int bicgstab_solve(cvr_handle *h, const cvr_precond *pc, const T *b, T *x, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    const long long n = h->info.nrows;
    const size_t    vb = sizeof(T) * (size_t)n;
    const T        *minv = static_cast<const T *>(opt->minv_dev);
    const bool      al = (((uintptr_t)b | (uintptr_t)x | (uintptr_t)minv) & 15u) == 0, hats = minv || pc;

    Arena        a;
    const size_t nx = x_ext_bytes(h), ny = y_ext_bytes(h), nh = hats ? nx : 0, npart = sizeof(double) * 2 * kBlocks;
    const size_t op = a.add(nx), os = a.add(nx), ophat = a.add(nh), oshat = a.add(nh), ov = a.add(ny), ot = a.add(ny), orr = a.add(ny), orhat = a.add(vec_bytes(h));
    const size_t oa = a.add(npart), ob = a.add(npart), ocell = a.add(sizeof(BiCell));
    HIP_TRY(a.alloc());
    const Workspace<T> w{a.at<T>(op), a.at<T>(os), hats ? a.at<T>(ophat) : nullptr, hats ? a.at<T>(oshat) : nullptr, a.at<T>(ov), a.at<T>(ot), a.at<T>(orr), a.at<T>(orhat),
                         a.at<double>(oa), a.at<double>(ob), a.at<BiCell>(ocell)};
    if (const int rc = a.begin(st)) return rc;

    // the pad slots of the SpMV inputs (p carries x0 into the scaled product; s's is cleared beside the diagonal too, not beside an object);
    // p = x0 for the moment, r = b; r = b - A x0; then r^, p, p^ and the start's sums, the cell; with an object p^ = W p
    for (T *q : {w.p, pc ? nullptr : w.s, w.phat, w.shat})
        if (q)
            if (const int rc = zero_pad_slot(q, vb, sizeof(T), st)) return rc;
    if (const int rc = start_residual(h, w.p, w.r, x, b, n, st)) return rc;
    int spmvs = 1;
    with_flags([&](auto PRE, auto AL) { launch(bicg_init_kernel<T, PRE, AL>, st, b, minv, w.r, w.rhat, w.p, w.phat, n, w.part_b); }, minv != nullptr, al);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bicg_check_kernel, dim3(1), dim3(kThreads), 0, st, w.part_b, opt->rtol, w.cell);
    HIP_TRY(hipGetLastError());
    if (pc) {
        launch_apply(w, pc, w.p, w.phat, n, st);
        HIP_TRY(hipGetLastError());
    }

    const T  *ph = w.phat ? w.phat : w.p, *sh = w.shat ? w.shat : w.s;
    BiCell    cell{};
    const int rc = run_batches(
        opt,
        [&](int k) -> int {
            HIP_TRY(run_spmv(h, ph, w.v, st));
            HIP_TRY(launch_first_half(w, pc, minv, n, al, k, st));
            HIP_TRY(run_spmv(h, sh, w.t, st));
            HIP_TRY(launch_second_half(w, pc, x, minv, n, al, k, opt->rtol, st));
            spmvs += 2;
            return CVR_OK;
        },
        [&](int, bool *stopped) -> int {
            if (const int rc = read_cell(&cell, w.cell, sizeof(cell), st)) return rc;
            *stopped = cell.stop || cell.half;
            return CVR_OK;
        });
    if (rc) return rc;
    return finish_solve(a, st, x, vb, cell, spmvs, res);
}

// what cvr_pbicgstab_device and cvr_pbicgstab check: the solver's arguments and the object's before the handle is looked at, then the handle and the pair
int check_pbicgstab(const cvr_handle *h, const cvr_precond *p, const void *b, const void *x, const cvr_cg_options *opt, const cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, b, x, opt, res)) return rc;
    if (const int rc = check_precond_args(p, opt, "cvr_pbicgstab")) return rc;
    if (const int rc = check_square_preprocessed(h, "cvr_pbicgstab", "BiCGSTAB needs")) return rc;
    if (const int rc = check_precond_pair(h, p, "cvr_pbicgstab")) return rc;
    return check_block_jacobi_or_ilu0(p, "cvr_pbicgstab");
}

int check_handle(const cvr_handle *h) { return check_square_preprocessed(h, "cvr_bicgstab", "BiCGSTAB needs"); }

// behind the argument checks (and, with an object, behind those of the handle and the pair: check_pbicgstab)
int bicgstab_device(cvr_handle *h, const cvr_precond *pc, const void *b, void *x, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    if (!pc)
        if (const int rc = check_handle(h)) return rc;
    Range range(pc ? "cvr_pbicgstab_device" : "cvr_bicgstab_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) { return bicgstab_solve(h, pc, static_cast<const decltype(t) *>(b), static_cast<decltype(t) *>(x), opt, res, st); });
}

}  // namespace

extern "C" {

int cvr_bicgstab_device(cvr_handle *h, const void *b_dev, void *x_dev, const cvr_cg_options *opt, cvr_cg_result *res, void *stream)
{
    if (const int rc = check_solver_args(h, b_dev, x_dev, opt, res)) return rc;
    return bicgstab_device(h, nullptr, b_dev, x_dev, opt, res, (hipStream_t)stream);
}

int cvr_bicgstab(cvr_handle *h, const void *b_host, void *x_host, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, b_host, x_host, opt, res)) return rc;
    if (const int rc = check_handle(h)) return rc;
    return solve_from_host(h, b_host, x_host, [&](const void *b, void *x, hipStream_t st) { return bicgstab_device(h, nullptr, b, x, opt, res, st); });
}

int cvr_pbicgstab_device(cvr_handle *h, const cvr_precond *p, const void *b_dev, void *x_dev, const cvr_cg_options *opt, cvr_cg_result *res, void *stream)
{
    if (const int rc = check_pbicgstab(h, p, b_dev, x_dev, opt, res)) return rc;
    return bicgstab_device(h, p, b_dev, x_dev, opt, res, (hipStream_t)stream);
}

int cvr_pbicgstab(cvr_handle *h, const cvr_precond *p, const void *b_host, void *x_host, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_pbicgstab(h, p, b_host, x_host, opt, res)) return rc;
    return solve_from_host(h, b_host, x_host, [&](const void *b, void *x, hipStream_t st) { return bicgstab_device(h, p, b, x, opt, res, st); });
}

}  // extern "C"
