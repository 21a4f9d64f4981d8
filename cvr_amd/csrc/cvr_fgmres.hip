// cvr_fgmres.hip -- flexible restarted GMRES(m) on the device (include/cvr_amd.h: cvr_fgmres_device, cvr_fgmres; Saad, SIAM J. Sci. Comput. 14, 1993):
// cvr_gmres.hip's recurrence on the same kernels (cvr_gmres_kernels.h) through the same cycle start and step (cvr_gmres_steps.h), with one thing
// changed: z_j = M_j^-1 v_j is KEPT for every column (Z: `restart` vectors beside the restart + 1 of the basis, in the call's one arena), and x is
// formed as x + Z y.  So no apply runs outside the steps, nothing needs a form of M^-1 for an fp64 combination (no u, no zu), and M_j may differ from
// step to step: every kind of cvr_precond is taken through its table's `apply` (what cvr_precond_apply_device calls), and so is a caller's function.
// Per step: the apply into column j of Z (enqueued behind the kernel that forms v_j), w = A z_j through run_spmv with that column as its input, and
// launch_step's five launches in their forms without a diagonal, <T, false, true>.
// Forming x: gmres_x_kernel<T, false, AL> given Z and Z's stride computes, per element, u = +0; u = u + y_i double(Z_i) for i ascending;
// x = T(double(x) + u) under its guard (owed, owed_at in (lo, hi]) in one launch on the CVR_GMRES_GROUPS sums -- the header's arithmetic bit for bit
// (the kernel reads its basis argument only there), so there is no x kernel of this file's own.
// Without an object and without a function Z IS the basis (the same pointer and stride, nothing copied, nothing applied): every launch is then
// gmres_solve's without minv_dev, in its order, on the same arguments, hence the same bits.
// Stops inside a batch.  Block-Jacobi keeps its gated kernel (pgmres_apply_kernel writing column j) and ILU(0) its sweeps under an Ilu0Gate on the
// stop word: behind a stop they write nothing.  The other kinds' applies and the callback are NOT gated: behind a stop they still run, on whatever
// the unwritten v holds, and write columns of Z.  That is harmless because of the order of the steps.  The finish of step k with column j that
// finds a stop owes columns 0 .. j (a breakdown: 0 .. j - 1), all written before it.  The apply enqueued behind that finish writes column j + 1, the
// one behind the next step column j + 2, and so on upwards: none of 0 .. j.  Column 0 is written again only at a cycle's wrap, and there form_x(k) is
// enqueued BEFORE the residual and before the apply into column 0 (it also stands in front of every read-back), so the owed columns are read
// before anything overwrites them; once x is formed, the guard (owed_at <= lo) keeps every later x launch out.  A stop that the cycle's start finds
// owes nothing.  Products and kernels of the steps behind a stop run as in cvr_gmres.hip: the product into w, which nothing reads, the gated
// kernels as no-ops.  Hence x and the result do not depend on check_every.
// spmv_count counts the handle's own products enqueued (1 + the steps + the restarts): PrecondOps::apply reports none (only cg_apply has *spmvs), so
// the products inside an object's apply (Chebyshev, FSAI, AMG) are not in it.
// The host side is cvr_krylov.h's driver, as in cvr_gmres.hip.
#include "cvr_gmres_steps.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

// the call's preconditioner: an object, a function, or neither
struct Flex {
    const cvr_precond *pc;
    cvr_apply_fn       fn;
    void              *ctx;
    bool               any() const { return pc || fn; }
};

// z = M_k^-1 v for step k, enqueued (or, by a callback, complete) on st; v a basis vector, z a column of Z
template <typename T>
int apply_column(const Flex &f, const GmresCell *cell, const T *v, T *z, long long n, int k, hipStream_t st)
{
    if (f.fn) {
        const int rc = f.fn(f.ctx, v, z, (int64_t)n, (void *)st);
        if (rc) return fail(CVR_ERR_STATE, "cvr_fgmres: the apply callback returned %d at step %d", rc, k);
        return CVR_OK;
    }
    if (f.pc->kind == kPrecondBlockJacobi) {
        launch(pgmres_apply_kernel<T>, st, static_cast<const T *>(f.pc->d_w), (int)f.pc->bs, v, z, n, cell);
        HIP_TRY(hipGetLastError());
        return CVR_OK;
    }
    if (f.pc->kind == kPrecondIlu0) {
        Ilu0Gate gate;
        gate.stop = &cell->hd.stop;
        gate.nstop = 1;
        return ilu0_apply<T, T>(f.pc, v, z, gate, st);
    }
    if (n == 0) return CVR_OK;          // (as cvr_precond_apply_device)
    return f.pc->ops->apply(f.pc, v, z, st);
}

template <typename T>
int fgmres_solve(cvr_handle *h, const Flex &f, const T *b, T *x, int m, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    const long long n = h->info.nrows;
    const size_t    vb = sizeof(T) * (size_t)n;
    const bool      al = (((uintptr_t)b | (uintptr_t)x) & 15u) == 0;

    Arena        a;
    const size_t nx = Arena::slot(x_ext_bytes(h));          // a basis vector or a column of Z: whole slots, so the stride is a whole number of values
    const size_t oV = a.add((size_t)(m + 1) * nx), oZ = a.add(f.any() ? (size_t)m * nx : 0), ow = a.add(y_ext_bytes(h)), orr = a.add(y_ext_bytes(h));
    const size_t oh = a.add(sizeof(double) * (size_t)m * kBlocks), os = a.add(sizeof(double) * 2 * kBlocks), ocell = a.add(sizeof(GmresCell));
    const hipError_t e = a.alloc();
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(CVR_ERR_NOMEM, "cvr_fgmres: no device memory for %d basis vectors and %d preconditioned vectors (%zu bytes)", m + 1, f.any() ? m : 0, a.total());
    }
    HIP_TRY(e);
    const Workspace<T> w{a.at<T>(oV), nullptr, a.at<T>(ow), a.at<T>(orr), nullptr, nullptr, a.at<double>(oh), a.at<double>(os), a.at<GmresCell>(ocell), (long long)(nx / sizeof(T))};
    T *const           Z = f.any() ? a.at<T>(oZ) : w.V;          // neither: Z aliases the basis
    auto               zcol = [&](int j) { return Z + (long long)j * w.stride; };
    if (const int rc = a.begin(st)) return rc;

    for (int i = 0; i <= m; i++)
        if (const int rc = zero_pad_slot(w.basis(i), vb, sizeof(T), st)) return rc;
    if (f.any())
        for (int i = 0; i < m; i++)
            if (const int rc = zero_pad_slot(zcol(i), vb, sizeof(T), st)) return rc;
    // r = b - A x, the sums, the stop test and v_0; then z_0 for step k, where a step follows
    auto residual = [&](bool first, int k) -> int {
        if (const int rc = start_residual(h, w.basis(1), w.r, x, b, n, st)) return rc;
        HIP_TRY(launch_begin(w, nullptr, b, (const T *)nullptr, n, al, opt->rtol, first, st));
        if (f.any() && k < opt->max_iters) return apply_column<T>(f, w.cell, w.basis(0), zcol(0), n, k, st);
        return CVR_OK;
    };
    if (const int rc = residual(true, 0)) return rc;
    int spmvs = 1;

    GmresHead hd{};
    int       x_lo = 0;          // the steps whose finish the x-forming kernel has looked at
    auto form_x = [&](int hi) -> int {
        if (hi > x_lo) {
            with_flags([&](auto AL) { launch(gmres_x_kernel<T, false, AL>, st, x, (const T *)nullptr, (const T *)Z, w.stride, n, (const GmresCell *)w.cell, x_lo, hi); }, al);
            HIP_TRY(hipGetLastError());
        }
        x_lo = hi;
        return CVR_OK;
    };
    const int rc = run_batches(
        opt,
        [&](int k) -> int {
            const int j = k % m;
            if (j == 0 && k > 0) {          // the cycle before is full: its x (which reads Z) in front of the residual and of the apply into column 0
                if (const int rc = form_x(k)) return rc;
                if (const int rc = residual(false, k)) return rc;
                spmvs++;
            }
            HIP_TRY(run_spmv(h, zcol(j), w.w, st));
            HIP_TRY(launch_step(w, nullptr, (const T *)nullptr, n, al, j, k, m, opt->max_iters, opt->rtol, st));
            spmvs++;
            if (f.any() && j + 1 < m && k + 1 < opt->max_iters)          // launch_step's rule: where the host knows that a v_(j+1) is formed
                return apply_column<T>(f, w.cell, w.basis(j + 1), zcol(j + 1), n, k + 1, st);
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

// what both entry points check, in the header's order: cvr_pgmres' argument checks (a null p allowed), one preconditioner per call, the restart,
// then the handle and, with an object, the pair
int check_fgmres(const cvr_handle *h, const cvr_precond *p, cvr_apply_fn fn, const void *b, const void *x, int32_t restart, const cvr_cg_options *opt, const cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, b, x, opt, res)) return rc;
    if (p && fn) return fail(CVR_ERR_INVALID, "cvr_fgmres: a preconditioner object and an apply callback are both set: one preconditioner per call");
    if (p)
        if (const int rc = check_precond_args(p, opt, "cvr_fgmres")) return rc;
    if (fn && opt->minv_dev) return fail(CVR_ERR_INVALID, "cvr_fgmres: minv_dev is set beside an apply callback: one preconditioner per call");
    if (opt->minv_dev) return fail(CVR_ERR_INVALID, "cvr_fgmres: minv_dev is set: cvr_fgmres takes an object or a callback (cvr_gmres takes a diagonal)");
    if (const int rc = check_restart(restart)) return rc;
    if (const int rc = check_square_preprocessed(h, "cvr_fgmres", "GMRES needs")) return rc;
    if (p)
        if (const int rc = check_precond_pair(h, p, "cvr_fgmres")) return rc;
    return CVR_OK;
}

// behind check_fgmres
int fgmres_device(cvr_handle *h, const Flex &f, const void *b, void *x, int m, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    Range range("cvr_fgmres_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) { return fgmres_solve(h, f, static_cast<const decltype(t) *>(b), static_cast<decltype(t) *>(x), m, opt, res, st); });
}

}  // namespace

extern "C" {

int cvr_fgmres_device(cvr_handle *h, const cvr_precond *p, cvr_apply_fn fn, void *ctx, const void *b_dev, void *x_dev, int32_t restart, const cvr_cg_options *opt,
                      cvr_cg_result *res, void *stream)
{
    if (const int rc = check_fgmres(h, p, fn, b_dev, x_dev, restart, opt, res)) return rc;
    return fgmres_device(h, Flex{p, fn, ctx}, b_dev, x_dev, restart, opt, res, (hipStream_t)stream);
}

int cvr_fgmres(cvr_handle *h, const cvr_precond *p, cvr_apply_fn fn, void *ctx, const void *b_host, void *x_host, int32_t restart, const cvr_cg_options *opt,
               cvr_cg_result *res)
{
    if (const int rc = check_fgmres(h, p, fn, b_host, x_host, restart, opt, res)) return rc;
    const Flex f{p, fn, ctx};
    return solve_from_host(h, b_host, x_host, [&](const void *b, void *x, hipStream_t st) { return fgmres_device(h, f, b, x, restart, opt, res, st); });
}

}  // extern "C"
