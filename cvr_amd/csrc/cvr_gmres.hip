// cvr_gmres.hip -- restarted GMRES(m) on the device for any nonsingular A (include/cvr_amd.h: cvr_gmres_device, cvr_gmres, cvr_pgmres_device,
// cvr_pgmres): cvr_bicgstab.hip's plan with an Arnoldi basis.  Right-preconditioned; per step one SpMV through run_spmv (cvr_spmv_device's path) and
// five vector launches, whatever the column j:
//   w = A z_j                  (z_j = minv .* v_j, written with v_j; v_j itself without a preconditioner)
//   gmres_dots_kernel          the partial sums of v_i . w for i = 0..j, the columns in compile-time groups of up to 8 with w's packet loaded once per group
//   gmres_update_kernel        h_i from those partials (summed in every workgroup, the same order everywhere); w -= sum h_i v_i in one pass over the basis
//   gmres_dots_kernel          the same on the new w (classical Gram-Schmidt, applied twice)
//   gmres_update_kernel        d_i, w -= sum d_i v_i and the partial sums of w . w; workgroup 0: H_i = h_i + d_i and the earlier rotations on the column
//   gmres_finish_kernel        H_(j+1) = sqrt(w . w), the new rotation, the stop test into the state cell; v_(j+1) = w / H_(j+1) (and z_(j+1))
// so a step reads the basis four times and w seven times over (w once per group of 8 columns in the dots), in 16-byte packets.  x is formed once per
// cycle (gmres_x_kernel: the small triangular solve is one thread's work in the kernel that finds the need), behind which the next cycle starts from the true
// residual (the scaled product, gmres_rr_kernel, gmres_begin_kernel).  The sums, the grid and the packet helpers are cvr_krylov.h's; every sum has its
// own 1024 partials, so its bits do not depend on the group it was formed in.  The scalars sit in a state cell (GmresCell) under BiCell's rule: thread 0
// of workgroup 0 writes it, and a value a kernel reads is one that a kernel BEFORE it wrote.  The kernel that finds a stop records it and every later
// kernel of the batch returns without writing, so the result does not depend on how many steps the host enqueues between two read-backs.
// The preconditioner is an argument of the one solve function: none, the diagonal opt->minv_dev (fused into the kernels above), or a block-Jacobi
// object (cvr_pgmres*).  An element of W v needs its whole block of v, so with an object z_j = W v_j is a launch of its own (pgmres_apply_kernel, by
// cvr_precond.h's apply_pack) behind gmres_begin_kernel and gmres_finish_kernel, which then run in their forms without a diagonal, <T, false, true>
// (not enqueued where the host knows that no v_(j+1) is formed: the cycle's or the call's last step).  x is then formed by two launches, because W
// needs the combination u of a whole block: pgmres_u_kernel (gmres_x_kernel's loop over the owed columns, u kept in fp64 in a buffer of n doubles)
// and pgmres_x_kernel (x = T(double(x) + W u), the apply's sum with u where it has double(r)), both under gmres_x_kernel's guard.
// An ILU(0) object (cvr_ilu0.hip) is taken in the same places, its apply being launches_lower + launches_upper launches of its own: z_j = M^-1 v_j
// under the stop rule, and for x the sweeps on the fp64 u (L's sweep reads u where it has double(r)) into a buffer zu of the call, then
// cvr_ilu0.hip's ilu0_add_to_x (x = T(double(x) + double(zu))), all under gmres_x_kernel's guard.
// The host side is cvr_krylov.h's driver: this file adds the step and the read-back (with the owed x in front of it); the cell and the gmres_*
// kernels are in cvr_gmres_kernels.h, the buffers and what a cycle's start and a step enqueue in cvr_gmres_steps.h (cvr_fgmres.hip runs the same).
// (The reference has no solver and no preconditioner: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_gmres_steps.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

// u of the columns the cell says are owed, when the step that said so lies in (lo, hi] (gmres_x_kernel's guard): per value u = +0, u = u + y_i double(v_i)
// for i ascending, stored as it is, in fp64.  Reads the cell only.
template <typename T>
__global__ __launch_bounds__(kThreads) void pgmres_u_kernel(double *__restrict__ ubuf, const T *__restrict__ V, long long stride, long long n,
                                                            const GmresCell *__restrict__ cell, int lo, int hi)
{
    __shared__ double ys[kMaxM];
    const int q = cell->hd.owed, at = cell->hd.owed_at;
    if (q <= 0 || at <= lo || at > hi) return;
    for (int i = threadIdx.x; i < q; i += kThreads) ys[i] = cell->y[i];
    __syncthreads();
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        double u[kPack<T>];
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) u[l] = 0;
        CVR_GMRES_GROUPS(add_group, q, ys, u);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) if (l < cnt) ubuf[e + l] = u[l];
    }
}

// ... and x from it, under the same guard: x_i = T(double(x_i) + (t_0 + t_1 + ..)), t_j = double(W[i][j]) * u[k bs + j], the apply's sum.  Reads the cell
// only.  AL: x, the caller's array, is 16-byte aligned.
template <typename T, bool AL>
__global__ __launch_bounds__(kThreads) void pgmres_x_kernel(T *__restrict__ x, const T *__restrict__ wt, int bs, const double *__restrict__ ubuf, long long n,
                                                            const GmresCell *__restrict__ cell, int lo, int hi)
{
    const int q = cell->hd.owed, at = cell->hd.owed_at;
    if (q <= 0 || at <= lo || at > hi) return;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T      xv[kPack<T>];
        double sv[kPack<T>];
        load_pack<T, AL>(x, e, (int)cnt, xv);
        apply_sums<T, double>(wt, bs, ubuf, n, e, (int)cnt, sv);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) xv[l] = (T)((double)xv[l] + sv[l]);
        store_pack<T, AL>(x, e, (int)cnt, xv);
    }
}

int check_handle(const cvr_handle *h) { return check_square_preprocessed(h, "cvr_gmres", "GMRES needs"); }

// cvr_krylov.h's driver with GMRES's cycle start, step and cell.  pc: a block-Jacobi object or null; with one, minv is null (the entry points see to it)
template <typename T>
int gmres_solve(cvr_handle *h, const cvr_precond *pc, const T *b, T *x, int m, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    const long long n = h->info.nrows;
    const size_t    vb = sizeof(T) * (size_t)n;
    const T        *minv = static_cast<const T *>(opt->minv_dev);
    const bool      al = (((uintptr_t)b | (uintptr_t)x | (uintptr_t)minv) & 15u) == 0, has_z = minv || pc;

    Arena        a;
    const size_t nx = Arena::slot(x_ext_bytes(h));          // a basis vector: whole slots, so the stride is a whole number of values
    const size_t oV = a.add((size_t)(m + 1) * nx), oz = a.add(has_z ? nx : 0), ow = a.add(y_ext_bytes(h)), orr = a.add(y_ext_bytes(h));
    const size_t ou = a.add(pc ? sizeof(double) * (size_t)std::max<long long>(n, 1) : 0), ozu = a.add(pc && pc->kind == kPrecondIlu0 ? vec_bytes(h) : 0);
    const size_t oh = a.add(sizeof(double) * (size_t)m * kBlocks), os = a.add(sizeof(double) * 2 * kBlocks), ocell = a.add(sizeof(GmresCell));
    const hipError_t e = a.alloc();
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(CVR_ERR_NOMEM, "%s: no device memory for %d basis vectors (%zu bytes)", pc ? "cvr_pgmres" : "cvr_gmres", m + 1, a.total());
    }
    HIP_TRY(e);
    const Workspace<T> w{a.at<T>(oV), has_z ? a.at<T>(oz) : nullptr, a.at<T>(ow), a.at<T>(orr), a.at<T>(ozu), pc ? a.at<double>(ou) : nullptr, a.at<double>(oh), a.at<double>(os),
                         a.at<GmresCell>(ocell), (long long)(nx / sizeof(T))};
    if (const int rc = a.begin(st)) return rc;

    // the pad slots of the SpMV inputs; basis vector 1 carries x into the scaled product (it is a column only from step 1 of a cycle on), r = b;
    // r = b - A x; then the sums, the stop test, v_0 and z_0
    for (int i = 0; i <= m; i++)
        if (const int rc = zero_pad_slot(w.basis(i), vb, sizeof(T), st)) return rc;
    if (w.z)
        if (const int rc = zero_pad_slot(w.z, vb, sizeof(T), st)) return rc;
    auto residual = [&](bool first) -> int {
        if (const int rc = start_residual(h, w.basis(1), w.r, x, b, n, st)) return rc;
        HIP_TRY(launch_begin(w, pc, b, minv, n, al, opt->rtol, first, st));
        return CVR_OK;
    };
    if (const int rc = residual(true)) return rc;
    int spmvs = 1;

    GmresHead hd{};
    int       x_lo = 0;          // the steps whose finish the x-forming kernels have looked at
    auto form_x = [&](int hi) -> int {
        if (hi > x_lo) {
            if (pc && pc->kind == kPrecondIlu0) {          // u, then the two sweeps on the fp64 u, then x: all under gmres_x_kernel's guard
                launch(pgmres_u_kernel<T>, st, w.u, (const T *)w.V, w.stride, n, (const GmresCell *)w.cell, x_lo, hi);
                HIP_TRY(hipGetLastError());
                Ilu0Gate gate;
                gate.owed = &w.cell->hd.owed;          // owed and owed_at: two adjacent words
                gate.lo = x_lo;
                gate.hi = hi;
                if (const int rc = ilu0_apply<T, double>(pc, (const double *)w.u, w.zu, gate, st)) return rc;
                if (const int rc = ilu0_add_to_x<T>(x, (const T *)w.zu, n, gate, al, st)) return rc;
            } else if (pc) {
                launch(pgmres_u_kernel<T>, st, w.u, (const T *)w.V, w.stride, n, (const GmresCell *)w.cell, x_lo, hi);
                with_flags([&](auto AL) { launch(pgmres_x_kernel<T, AL>, st, x, static_cast<const T *>(pc->d_w), (int)pc->bs, (const double *)w.u, n, (const GmresCell *)w.cell, x_lo, hi); }, al);
            } else {
                with_flags([&](auto PRE, auto AL) { launch(gmres_x_kernel<T, PRE, AL>, st, x, minv, w.V, w.stride, n, w.cell, x_lo, hi); }, minv != nullptr, al);
            }
            HIP_TRY(hipGetLastError());
        }
        x_lo = hi;
        return CVR_OK;
    };
    const int rc = run_batches(
        opt,
        [&](int k) -> int {
            const int j = k % m;
            if (j == 0 && k > 0) {          // the cycle before is full: its x, then the next one from the true residual
                if (const int rc = form_x(k)) return rc;
                if (const int rc = residual(false)) return rc;
                spmvs++;
            }
            HIP_TRY(run_spmv(h, w.z ? w.z : w.basis(j), w.w, st));
            HIP_TRY(launch_step(w, pc, minv, n, al, j, k, m, opt->max_iters, opt->rtol, st));
            spmvs++;
            return CVR_OK;
        },
        [&](int done, bool *stopped) -> int {
            if (const int rc = form_x(done)) return rc;
            if (const int rc = read_cell(&hd, &w.cell->hd, sizeof(hd), st)) return rc;
            *stopped = hd.stop != 0;
            return CVR_OK;
        });
    if (rc) return rc;
    return finish_solve(a, st, x, vb, hd, spmvs, res);
}

// what cvr_pgmres_device and cvr_pgmres check: the solver's arguments, the object's and the restart before the handle is looked at, then the handle
// and the pair
int check_pgmres(const cvr_handle *h, const cvr_precond *p, const void *b, const void *x, int32_t restart, const cvr_cg_options *opt, const cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, b, x, opt, res)) return rc;
    if (const int rc = check_precond_args(p, opt, "cvr_pgmres")) return rc;
    if (const int rc = check_restart(restart)) return rc;
    if (const int rc = check_square_preprocessed(h, "cvr_pgmres", "GMRES needs")) return rc;
    if (const int rc = check_precond_pair(h, p, "cvr_pgmres")) return rc;
    return check_block_jacobi_or_ilu0(p, "cvr_pgmres");
}

// behind the argument checks (and, with an object, behind those of the handle and the pair: check_pgmres)
int gmres_device(cvr_handle *h, const cvr_precond *pc, const void *b, void *x, int m, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    if (!pc)
        if (const int rc = check_handle(h)) return rc;
    Range range(pc ? "cvr_pgmres_device" : "cvr_gmres_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) { return gmres_solve(h, pc, static_cast<const decltype(t) *>(b), static_cast<decltype(t) *>(x), m, opt, res, st); });
}

static_assert(offsetof(GmresHead, owed_at) == offsetof(GmresHead, owed) + sizeof(int32_t), "the gate reads owed and owed_at as two adjacent words");

}  // namespace

extern "C" {

int cvr_gmres_device(cvr_handle *h, const void *b_dev, void *x_dev, int32_t restart, const cvr_cg_options *opt, cvr_cg_result *res, void *stream)
{
    if (const int rc = check_solver_args(h, b_dev, x_dev, opt, res)) return rc;
    if (const int rc = check_restart(restart)) return rc;
    return gmres_device(h, nullptr, b_dev, x_dev, restart, opt, res, (hipStream_t)stream);
}

int cvr_gmres(cvr_handle *h, const void *b_host, void *x_host, int32_t restart, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, b_host, x_host, opt, res)) return rc;
    if (const int rc = check_restart(restart)) return rc;
    if (const int rc = check_handle(h)) return rc;
    return solve_from_host(h, b_host, x_host, [&](const void *b, void *x, hipStream_t st) { return gmres_device(h, nullptr, b, x, restart, opt, res, st); });
}

int cvr_pgmres_device(cvr_handle *h, const cvr_precond *p, const void *b_dev, void *x_dev, int32_t restart, const cvr_cg_options *opt, cvr_cg_result *res, void *stream)
{
    if (const int rc = check_pgmres(h, p, b_dev, x_dev, restart, opt, res)) return rc;
    return gmres_device(h, p, b_dev, x_dev, restart, opt, res, (hipStream_t)stream);
}

int cvr_pgmres(cvr_handle *h, const cvr_precond *p, const void *b_host, void *x_host, int32_t restart, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_pgmres(h, p, b_host, x_host, restart, opt, res)) return rc;
    return solve_from_host(h, b_host, x_host, [&](const void *b, void *x, hipStream_t st) { return gmres_device(h, p, b, x, restart, opt, res, st); });
}

}  // extern "C"
