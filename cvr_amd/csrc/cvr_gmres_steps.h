// cvr_gmres_steps.h -- what a GMRES(m) step enqueues, shared by the two files that run the recurrence (cvr_gmres.hip: cvr_gmres*, cvr_pgmres*;
// cvr_fgmres.hip: cvr_fgmres*): the call's buffers, the block-Jacobi apply under the stop rule, the cycle's start and the step behind w = A z_j.
// What each kernel does: cvr_gmres.hip's head.  Both files get the same code, so a step has the same bits in both.
#pragma once
#include "cvr_krylov.h"
#include "cvr_gmres_kernels.h"
#include "cvr_precond.h"

namespace cvrh {
namespace krylov {
namespace {

// z = W v on the solvers' grid, v and z the library's buffers (16-byte aligned); nothing is written once the cell holds a stop (no workgroup of this
// kernel sets it)
template <typename T>
__global__ __launch_bounds__(kThreads) void pgmres_apply_kernel(const T *__restrict__ wt, int bs, const T *__restrict__ v, T *__restrict__ z, long long n,
                                                                const GmresCell *__restrict__ cell)
{
    if (cell->hd.stop) return;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T zv[kPack<T>];
        apply_pack<T>(wt, bs, v, n, e, (int)cnt, zv);
        store_pack<T, true>(z, e, (int)cnt, zv);
    }
}

// the library's buffers of one call: restart + 1 basis vectors and (with a preconditioner) z (x_ext each: SpMV inputs), w and r (y_ext each: r takes
// the scaled product), with an object u (n doubles), the partial sums of the dots (one set per column) and of r . r, b . b and w . w, the cell
template <typename T>
struct Workspace {
    T         *V, *z, *w, *r;
    T         *zu;          // with an ILU(0) object: M^-1 u on its way into x (n values)
    double    *u, *part_h, *part_s;
    GmresCell *cell;
    long long  stride;          // of the basis, in values
    T         *basis(int i) const { return V + (long long)i * stride; }
};

// z = W v, with an object; an ILU(0) object's apply is its own launches (cvr_precond.h: ilu0_apply), under the same rule: behind a stop nothing is written
template <typename T>
void launch_apply(const Workspace<T> &w, const cvr_precond *pc, const T *v, long long n, hipStream_t st)
{
    if (pc->kind == kPrecondIlu0) {
        Ilu0Gate gate;
        gate.stop = &w.cell->hd.stop;
        gate.nstop = 1;
        (void)ilu0_apply<T, T>(pc, v, w.z, gate, st);          // (a launch error stays in hipGetLastError for the caller)
        return;
    }
    launch(pgmres_apply_kernel<T>, st, static_cast<const T *>(pc->d_w), (int)pc->bs, v, w.z, n, (const GmresCell *)w.cell);
}

// behind the scaled product r = b - A x: the sums, the cycle's start and, with an object, z_0.  (gmres_rr_kernel reads b, the one caller's array, only
// at the call's start; beside an object gmres_begin_kernel, which reads none, runs in its aligned form.)
template <typename T>
hipError_t launch_begin(const Workspace<T> &w, const cvr_precond *pc, const T *b, const T *minv, long long n, bool al, double rtol, bool first, hipStream_t st)
{
    with_flags([&](auto FIRST, auto AL) { launch(gmres_rr_kernel<T, FIRST, AL || !FIRST>, st, w.r, b, n, w.part_s, w.cell); }, first, al);
    with_flags([&](auto PRE, auto AL) { launch(gmres_begin_kernel<T, PRE, AL>, st, w.r, minv, w.basis(0), w.z, n, w.part_s, rtol, first ? 1 : 0, w.cell); }, minv != nullptr, al || pc);
    if (pc) launch_apply(w, pc, w.basis(0), n, st);
    return hipGetLastError();
}

// step k with column j behind w = A z_j: the two Gram-Schmidt passes, the finish and, with an object, z_(j+1)
template <typename T>
hipError_t launch_step(const Workspace<T> &w, const cvr_precond *pc, const T *minv, long long n, bool al, int j, int k, int m, int max_iters, double rtol, hipStream_t st)
{
    launch(gmres_dots_kernel<T>, st, w.V, w.stride, w.w, n, j + 1, w.part_h, w.cell);
    launch(gmres_update_kernel<T, false>, st, w.V, w.stride, w.w, n, j, w.part_h, w.part_s, w.cell);
    launch(gmres_dots_kernel<T>, st, w.V, w.stride, w.w, n, j + 1, w.part_h, w.cell);
    launch(gmres_update_kernel<T, true>, st, w.V, w.stride, w.w, n, j, w.part_h, w.part_s, w.cell);
    // (v_(j+1) and z_(j+1) are written only when j + 1 < m and k + 1 < max_iters, which the host knows as well: basis vector m is never a column; it
    // carries x into the scaled product.  A stop the finish finds is in the cell.  minv is the kernel's one caller's array: without it there is no
    // unaligned form)
    with_flags([&](auto PRE, auto AL) { launch(gmres_finish_kernel<T, PRE, AL || !PRE>, st, w.w, minv, w.basis(j + 1), w.z, n, w.part_s, w.cell, j, k, m, max_iters, rtol); }, minv != nullptr, al);
    if (pc && j + 1 < m && k + 1 < max_iters) launch_apply(w, pc, w.basis(j + 1), n, st);
    return hipGetLastError();
}

inline int check_restart(int32_t restart)
{
    if (restart < 1 || restart > kMaxM) return fail(CVR_ERR_INVALID, "restart = %d: must be in 1 .. %d", restart, kMaxM);
    return CVR_OK;
}

}  // namespace
}  // namespace krylov
}  // namespace cvrh
