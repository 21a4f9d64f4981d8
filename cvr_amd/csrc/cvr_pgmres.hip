// cvr_pgmres.hip -- restarted GMRES(m) preconditioned by a block-Jacobi object (include/cvr_amd.h: cvr_pgmres_device, cvr_pgmres): cvr_gmres.hip's solver
// with z_j = W v_j by the object's apply (cvr_precond.h: apply_pack) in place of a product with a diagonal.  An element of z needs its whole block of v, so
// the apply is a launch of its own behind the kernel that writes v; per step one SpMV and six vector launches:
//   w = A z_j
//   gmres_dots_kernel, gmres_update_kernel<T, false>, gmres_dots_kernel, gmres_update_kernel<T, true>     the two Gram-Schmidt passes
//   gmres_finish_kernel<T, false, true>     the rotation and the stop test; v_(j+1)
//   pgmres_apply_kernel                     z_(j+1) = W v_(j+1) (not enqueued where the host knows that no v_(j+1) is formed: the cycle's or the call's last step)
// and behind gmres_begin_kernel<T, false, true> at a cycle's start z_0 = W v_0.  x is formed by two launches, because W needs the combination u of a whole
// block: pgmres_u_kernel (gmres_x_kernel's loop over the owed columns, u kept in fp64 in a buffer of n doubles) and pgmres_x_kernel
// (x = T(double(x) + W u), the apply's sum with u where it has double(r)), both under gmres_x_kernel's guard.
// The gmres_* kernels are cvr_gmres_kernels.h's, the ones cvr_gmres_device runs, in the forms that take no diagonal; the apply returns at its top once the
// cell holds a stop, as they do, so the result does not depend on how many steps the host enqueues between two read-backs.
// (The reference has no solver and no preconditioner: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_gmres_kernels.h"
#include "cvr_precond.h"

using namespace cvrh;
using namespace cvrh::krylov;

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

// the library's buffers of one call: restart + 1 basis vectors and z (x_ext each: SpMV inputs), w and r (y_ext each: r takes the scaled product), u (n
// doubles), the partial sums of the dots (one set per column) and of r . r, b . b and w . w, the cell
template <typename T>
struct Workspace {
    T         *V, *z, *w, *r;
    double    *u, *part_h, *part_s;
    GmresCell *cell;
    long long  stride;          // of the basis, in values
    T         *basis(int i) const { return V + (long long)i * stride; }
};

template <typename T>
void launch_apply(const Workspace<T> &w, const cvr_precond *pc, const T *v, long long n, hipStream_t st)
{
    launch(pgmres_apply_kernel<T>, st, static_cast<const T *>(pc->d_w), (int)pc->bs, v, w.z, n, (const GmresCell *)w.cell);
}

// behind the scaled product r = b - A x: the sums, the cycle's start and z_0
template <typename T>
hipError_t launch_begin(const Workspace<T> &w, const cvr_precond *pc, const T *b, long long n, bool al, double rtol, bool first, hipStream_t st)
{
    with_flags([&](auto FIRST, auto AL) { launch(gmres_rr_kernel<T, FIRST, AL || !FIRST>, st, w.r, b, n, w.part_s, w.cell); }, first, al);
    launch(gmres_begin_kernel<T, false, true>, st, w.r, (const T *)nullptr, w.basis(0), w.z, n, w.part_s, rtol, first ? 1 : 0, w.cell);
    launch_apply(w, pc, w.basis(0), n, st);
    return hipGetLastError();
}

// step k with column j behind w = A z_j: the two Gram-Schmidt passes, the finish and z_(j+1)
template <typename T>
hipError_t launch_step(const Workspace<T> &w, const cvr_precond *pc, long long n, int j, int k, int m, int max_iters, double rtol, hipStream_t st)
{
    launch(gmres_dots_kernel<T>, st, w.V, w.stride, w.w, n, j + 1, w.part_h, w.cell);
    launch(gmres_update_kernel<T, false>, st, w.V, w.stride, w.w, n, j, w.part_h, w.part_s, w.cell);
    launch(gmres_dots_kernel<T>, st, w.V, w.stride, w.w, n, j + 1, w.part_h, w.cell);
    launch(gmres_update_kernel<T, true>, st, w.V, w.stride, w.w, n, j, w.part_h, w.part_s, w.cell);
    launch(gmres_finish_kernel<T, false, true>, st, w.w, (const T *)nullptr, w.basis(j + 1), w.z, n, w.part_s, w.cell, j, k, m, max_iters, rtol);
    // (the finish writes v_(j+1) only when j + 1 < m and k + 1 < max_iters, which the host knows as well; a stop it finds is in the cell)
    if (j + 1 < m && k + 1 < max_iters) launch_apply(w, pc, w.basis(j + 1), n, st);
    return hipGetLastError();
}

int check_restart(int32_t restart)
{
    if (restart < 1 || restart > kMaxM) return fail(CVR_ERR_INVALID, "restart = %d: must be in 1 .. %d", restart, kMaxM);
    return CVR_OK;
}

// cvr_gmres.hip's gmres_solve with W in place of minv
template <typename T>
int pgmres_solve(cvr_handle *h, const cvr_precond *pc, const T *b, T *x, int m, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    const long long n = h->info.nrows;
    const size_t    vb = sizeof(T) * (size_t)n;
    const bool      al = (((uintptr_t)b | (uintptr_t)x) & 15u) == 0;

    Arena        a;
    const size_t nx = Arena::slot(x_ext_bytes(h));          // a basis vector: whole slots, so the stride is a whole number of values
    const size_t oV = a.add((size_t)(m + 1) * nx), oz = a.add(nx), ow = a.add(y_ext_bytes(h)), orr = a.add(y_ext_bytes(h));
    const size_t ou = a.add(sizeof(double) * (size_t)std::max<long long>(n, 1));
    const size_t oh = a.add(sizeof(double) * (size_t)m * kBlocks), os = a.add(sizeof(double) * 2 * kBlocks), ocell = a.add(sizeof(GmresCell));
    const hipError_t e = a.alloc();
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(CVR_ERR_NOMEM, "cvr_pgmres: no device memory for %d basis vectors (%zu bytes)", m + 1, a.total());
    }
    HIP_TRY(e);
    const Workspace<T> w{a.at<T>(oV), a.at<T>(oz), a.at<T>(ow), a.at<T>(orr), a.at<double>(ou), a.at<double>(oh), a.at<double>(os), a.at<GmresCell>(ocell), (long long)(nx / sizeof(T))};
    if (const int rc = a.begin(st)) return rc;

    // the pad slots of the SpMV inputs; basis vector 1 carries x into the scaled product (it is a column only from step 1 of a cycle on), r = b;
    // r = b - A x; then the sums, the stop test, v_0 and z_0
    for (int i = 0; i <= m; i++)
        if (const int rc = zero_pad_slot(w.basis(i), vb, sizeof(T), st)) return rc;
    if (const int rc = zero_pad_slot(w.z, vb, sizeof(T), st)) return rc;
    auto residual = [&](bool first) -> int {
        if (const int rc = start_residual(h, w.basis(1), w.r, x, b, n, st)) return rc;
        HIP_TRY(launch_begin(w, pc, b, n, al, opt->rtol, first, st));
        return CVR_OK;
    };
    if (const int rc = residual(true)) return rc;
    int spmvs = 1;

    GmresHead hd{};
    int       x_lo = 0;          // the steps whose finish the x-forming kernels have looked at
    auto form_x = [&](int hi) -> int {
        if (hi > x_lo) {
            launch(pgmres_u_kernel<T>, st, w.u, (const T *)w.V, w.stride, n, (const GmresCell *)w.cell, x_lo, hi);
            with_flags([&](auto AL) { launch(pgmres_x_kernel<T, AL>, st, x, static_cast<const T *>(pc->d_w), (int)pc->bs, (const double *)w.u, n, (const GmresCell *)w.cell, x_lo, hi); }, al);
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
            HIP_TRY(run_spmv(h, w.z, w.w, st));
            HIP_TRY(launch_step(w, pc, n, j, k, m, opt->max_iters, opt->rtol, st));
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
    if (hd.zero_x && n) HIP_TRY(hipMemsetAsync(x, 0, vb, st));
    double seconds = 0;
    if (const int rc = a.seconds(st, &seconds)) return rc;
    fill_result(res, hd.iters, hd.status, spmvs, hd.rnorm, hd.bnorm, seconds);
    return CVR_OK;
}

// what the entry points check before any device work and before the handle is looked at
int check_args(const void *h, const cvr_precond *p, const void *b, const void *x, int32_t restart, const cvr_cg_options *opt, const cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, b, x, opt, res)) return rc;
    if (const int rc = check_precond_args(p, opt, "cvr_pgmres")) return rc;
    return check_restart(restart);
}

// ... and what they ask of the handle and of the pair
int check_handle(const cvr_handle *h, const cvr_precond *p)
{
    if (const int rc = check_square_preprocessed(h, "cvr_pgmres", "GMRES needs")) return rc;
    if (const int rc = check_precond_pair(h, p, "cvr_pgmres")) return rc;
    return check_block_jacobi(p, "cvr_pgmres");
}

int pgmres_device(cvr_handle *h, const cvr_precond *p, const void *b, void *x, int m, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    Range range("cvr_pgmres_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) { return pgmres_solve(h, p, static_cast<const decltype(t) *>(b), static_cast<decltype(t) *>(x), m, opt, res, st); });
}

}  // namespace

extern "C" {

int cvr_pgmres_device(cvr_handle *h, const cvr_precond *p, const void *b_dev, void *x_dev, int32_t restart, const cvr_cg_options *opt, cvr_cg_result *res, void *stream)
{
    if (const int rc = check_args(h, p, b_dev, x_dev, restart, opt, res)) return rc;
    if (const int rc = check_handle(h, p)) return rc;
    return pgmres_device(h, p, b_dev, x_dev, restart, opt, res, (hipStream_t)stream);
}

int cvr_pgmres(cvr_handle *h, const cvr_precond *p, const void *b_host, void *x_host, int32_t restart, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_args(h, p, b_host, x_host, restart, opt, res)) return rc;
    if (const int rc = check_handle(h, p)) return rc;
    return solve_from_host(h, b_host, x_host, [&](const void *b, void *x, hipStream_t st) { return pgmres_device(h, p, b, x, restart, opt, res, st); });
}

}  // extern "C"
