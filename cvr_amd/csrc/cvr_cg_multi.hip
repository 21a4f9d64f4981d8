// cvr_cg_multi.hip -- conjugate gradients for up to kSpmmBlock right-hand sides at once (include/cvr_amd.h: cvr_cg_multi_device, cvr_cg_multi,
// cvr_pcg_multi_device, cvr_pcg_multi):
// cvr_cg.hip's loop around the k-wide product (launch_spmm), so a step reads the image once for all columns, takes four launches instead of four
// per column, and one read-back serves the block.  B, X and the library's P, Q, R, Z are row-major blocks, row i = the values of all columns at i.
// Column j gets bit for bit what cvr_cg_device gives for b = B[:, j], x0 = X[:, j]: the product's columns are cvr_spmv_device's bit for bit, the
// elementwise arithmetic is the same expression per value, and the sums keep cvr_cg.hip's tree -- the thread that owns rows e .. e + kPack - 1 of a
// single vector (CVR_KRYLOV_PACKETS) owns those rows of every column and adds each column's terms in the same order, then store_partials /
// sum_partials run per column over that column's own kBlocks partials.
// The columns of a row are handled in sub-blocks of kPack<T> columns (16 bytes: one wide load where the leading dimension and the base allow it),
// unrolled over the kSpmmBlock columns there can be, so a column's accumulators and scalars are registers; nvec itself is a runtime argument.
// Every column has its own state cell.  A column that has stopped is not written any more (its bit in the kernels' `live` mask is clear; its
// values are still loaded and computed with where they share a sub-block with a live column, and dropped); the others go on.
// The preconditioner is an argument of the one solve function: none, the diagonal opt->minv_dev, or an object whose kind has a k-wide apply
// (PrecondOps::cgm_apply: block-Jacobi's pcgm_apply_kernel, cvr_pcg_multi.hip; a cvr_precond_amg_block object's cycle, cvr_amg_block.hip), which is enqueued between cgm_update_kernel<T, false, LV, AL> and
// cgm_direction_kernel<T, true, LV>: column j then gets bit for bit what cvr_pcg_device gives for b = B[:, j], x0 = X[:, j].
// The host side is cvr_krylov.h's driver: the cells and the kernels are in cvr_cg_multi_kernels.h, this file adds the step and the read-back of all
// columns.
#include "cvr_cg_multi_kernels.h"
#include "cvr_precond.h"

namespace cvrh {
namespace krylov {
namespace {

// one workgroup: every column's start sums into its cell, and the stop test of its start vector (cvr_cg.hip's cg_check_kernel per column).
// (The solver's one kernel that is no template: here and not in cvr_cg_multi_kernels.h, so that a file which includes the header for the cells gets no copy.)
__global__ __launch_bounds__(kThreads) void cgm_check_kernel(const double *__restrict__ part, int pre, double rtol, int nvec, CgCell *__restrict__ cells)
{
    __shared__ double sh[kCols][kSets][kWaves];
    for (int col = 0; col < nvec; col++) {
        double s[kSets];
        sum_partials<kSets>(part + (size_t)col * kSets * kBlocks, s, sh[col]);
        if (threadIdx.x != 0) continue;
        CgCell c;
        c.bb = s[2]; c.bnorm = sqrt(s[2]);
        c.rr = s[0]; c.rnorm = sqrt(s[0]);
        c.rz[0] = pre ? s[1] : s[0]; c.rz[1] = 0;
        c.stop = 0; c.status = CVR_CG_MAX_ITERS; c.iters = 0; c.zero_x = 0;
        if (c.bb == 0) { c.zero_x = 1; c.rr = 0; c.rnorm = 0; c.status = CVR_CG_CONVERGED; c.stop = 1; }
        else if (c.rnorm <= rtol * c.bnorm && c.rnorm <= kDblMax) { c.status = CVR_CG_CONVERGED; c.stop = 1; }
        cells[col] = c;
    }
}

}  // namespace
}  // namespace krylov
}  // namespace cvrh

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

// the object's apply on the call's blocks, through its kind's table: Z = M R and r . z per column; at the start P = Z too
template <typename T>
int launch_apply(const Workspace<T> &w, const Call<T> &c, const cvr_precond *pc, bool start, hipStream_t st, int *spmms)
{
    return precond_cgm_apply<T>(pc, w.r, w.z, w.p, c.n, c.nvec, c.lv, w.part, w.cells, start, st, spmms);
}

// the three vector launches of step k (the product Q = A P is enqueued in front of them), four with an object: its apply in front of the direction.
// Without a preconditioner z is r.
template <typename T>
int launch_step(const Workspace<T> &w, const Call<T> &c, const cvr_precond *pc, int k, hipStream_t st, int *spmms)
{
    with_flags([&](auto LV) { launch(cgm_pq_kernel<T, LV>, st, w.p, w.q, c.n, c.nvec, w.part_pq, w.cells); }, c.lv);
    with_flags([&](auto PRE, auto LV, auto AL) { launch(cgm_update_kernel<T, PRE, LV, AL>, st, c.x, c.ldx, w.r, w.z, w.p, w.q, c.minv, c.n, c.nvec, w.part_pq, w.part, w.cells, k); },
               c.minv != nullptr, c.lv, c.al);
    if (pc) {
        HIP_TRY(hipGetLastError());
        if (const int rc = launch_apply(w, c, pc, false, st, spmms)) return rc;
    }
    with_flags([&](auto PRE, auto LV) { launch(cgm_direction_kernel<T, PRE, LV>, st, w.p, PRE ? w.z : w.r, c.n, c.nvec, w.part, w.cells, k, c.rtol); }, w.z != nullptr, c.lv);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

// cvr_krylov.h's driver with the block's start, step and cells.  pc: an object behind check_multi, or null; with one, minv is null (the entry points see to it)
template <typename T>
int cg_multi_solve(cvr_handle *h, const cvr_precond *pc, bool single, const T *B, int64_t ldb, T *X, int64_t ldx, int32_t nvec, const cvr_cg_options *opt,
                   cvr_cg_result *res, hipStream_t st)
{
    const long long n = h->info.nrows;
    Call<T>         c{B, ldb, X, ldx, static_cast<const T *>(opt->minv_dev), n, nvec, false, false, opt->rtol};
    c.lv = nvec % kPack<T> == 0;
    c.al = (((uintptr_t)B | (uintptr_t)X | (uintptr_t)c.minv) & 15u) == 0 && ldb % kPack<T> == 0 && ldx % kPack<T> == 0;
    const bool has_z = c.minv || pc;

    Arena        a;
    const size_t op = a.add(x_ext_bytes(h, nvec)), oq = a.add(y_ext_bytes(h, nvec)), orr = a.add(y_ext_bytes(h, nvec)), oz = a.add(has_z ? vec_bytes(h, nvec) : 0);
    const size_t opq = a.add(sizeof(double) * kCols * kBlocks), opart = a.add(sizeof(double) * kCols * kSets * kBlocks), ocells = a.add(sizeof(CgCell) * kCols);
    HIP_TRY(a.alloc());
    const Workspace<T> w{a.at<T>(op), a.at<T>(oq), a.at<T>(orr), has_z ? a.at<T>(oz) : nullptr, a.at<double>(opq), a.at<double>(opart), a.at<CgCell>(ocells)};
    if (const int rc = a.begin(st)) return rc;

    // P = X0 for the moment (with its zero row), Q = A X0; then R, Z, P and the start's sums (with an object: P = R, then Z = W R, P = Z and r . z)
    launch(cgm_start_kernel<T>, st, X, (long long)ldx, w.p, n, nvec);
    HIP_TRY(hipGetLastError());
    if (const int rc = product(h, single, w, nvec, st)) return rc;
    int spmms = 1;
    with_flags([&](auto PRE, auto LV, auto AL) { launch(cgm_init_kernel<T, PRE, LV, AL>, st, c.b, c.ldb, c.minv, w.q, w.r, w.z, w.p, c.n, c.nvec, w.part); }, c.minv != nullptr, c.lv, c.al);
    HIP_TRY(hipGetLastError());
    if (pc)
        if (const int rc = launch_apply(w, c, pc, true, st, &spmms)) return rc;
    hipLaunchKernelGGL(cgm_check_kernel, dim3(1), dim3(kThreads), 0, st, w.part, has_z ? 1 : 0, opt->rtol, nvec, w.cells);
    HIP_TRY(hipGetLastError());

    CgCell    cells[kCols] = {};
    const int rc = run_batches(
        opt,
        [&](int k) -> int {
            if (const int rc = product(h, single, w, nvec, st)) return rc;
            spmms++;
            return launch_step(w, c, pc, k, st, &spmms);
        },
        [&](int, bool *stopped) -> int {          // stopped: every column has
            if (const int rc = read_cell(cells, w.cells, sizeof(CgCell) * (size_t)nvec, st)) return rc;
            *stopped = true;
            for (int j = 0; j < nvec; j++) *stopped = *stopped && cells[j].stop;
            return CVR_OK;
        });
    if (rc) return rc;
    uint32_t zero = 0;
    for (int j = 0; j < nvec; j++) if (cells[j].zero_x) zero |= 1u << j;
    if (zero && n) {
        launch(cgm_zero_kernel<T>, st, X, (long long)ldx, n, nvec, zero);
        HIP_TRY(hipGetLastError());
    }
    double seconds = 0;
    if (const int rc = a.seconds(st, &seconds)) return rc;
    for (int j = 0; j < nvec; j++) fill_result(&res[j], cells[j].iters, cells[j].status, spmms, cells[j].rnorm, cells[j].bnorm, seconds);
    return CVR_OK;
}

// behind the argument checks (and, with an object, behind those of the handle and the pair: check_pcg_multi)
int cg_multi_device(cvr_handle *h, const cvr_precond *pc, const void *B, int64_t ldb, void *X, int64_t ldx, int32_t nvec, const cvr_cg_options *opt,
                    cvr_cg_result *res, hipStream_t st)
{
    const bool single = nvec == 1 && ldb == 1 && ldx == 1;
    if (!pc)
        if (const int rc = check_handle(h, nvec, single, "cvr_cg_multi")) return rc;
    Range range(pc ? "cvr_pcg_multi_device" : "cvr_cg_multi_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) {
        return cg_multi_solve(h, pc, single, static_cast<const decltype(t) *>(B), ldb, static_cast<decltype(t) *>(X), ldx, nvec, opt, res, st);
    });
}

// what cvr_pcg_multi_device and cvr_pcg_multi check: the solver's arguments, the object's and the block's before the handle is looked at, then the
// handle and the pair
int check_pcg_multi(const cvr_handle *h, const cvr_precond *p, const void *B, const void *X, int32_t nvec, int64_t ldb, int64_t ldx, const cvr_cg_options *opt,
                    const cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, B, X, opt, res)) return rc;
    if (const int rc = check_precond_args(p, opt, "cvr_pcg_multi")) return rc;
    if (const int rc = check_block_args(nvec, ldb, ldx)) return rc;
    if (const int rc = check_handle(h, nvec, nvec == 1 && ldb == 1 && ldx == 1, "cvr_pcg_multi")) return rc;
    if (const int rc = check_precond_pair(h, p, "cvr_pcg_multi")) return rc;
    return check_multi(p, nvec, "cvr_pcg_multi");
}

}  // namespace

extern "C" {

int cvr_cg_multi_device(cvr_handle *h, const void *B_dev, int64_t ldb, void *X_dev, int64_t ldx, int32_t nvec, const cvr_cg_options *opt, cvr_cg_result *res,
                        void *stream)
{
    if (const int rc = check_solver_args(h, B_dev, X_dev, opt, res)) return rc;
    if (const int rc = check_block_args(nvec, ldb, ldx)) return rc;
    return cg_multi_device(h, nullptr, B_dev, ldb, X_dev, ldx, nvec, opt, res, (hipStream_t)stream);
}

int cvr_cg_multi(cvr_handle *h, const void *B_host, void *X_host, int32_t nvec, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, B_host, X_host, opt, res)) return rc;
    if (const int rc = check_block_args(nvec, nvec, nvec)) return rc;
    if (const int rc = check_handle(h, nvec, nvec == 1, "cvr_cg_multi")) return rc;
    return solve_block_from_host(h, B_host, X_host, nvec, [&](const void *B, void *X, hipStream_t st) { return cg_multi_device(h, nullptr, B, nvec, X, nvec, nvec, opt, res, st); });
}

int cvr_pcg_multi_device(cvr_handle *h, const cvr_precond *p, const void *B_dev, int64_t ldb, void *X_dev, int64_t ldx, int32_t nvec, const cvr_cg_options *opt,
                         cvr_cg_result *res, void *stream)
{
    if (const int rc = check_pcg_multi(h, p, B_dev, X_dev, nvec, ldb, ldx, opt, res)) return rc;
    return cg_multi_device(h, p, B_dev, ldb, X_dev, ldx, nvec, opt, res, (hipStream_t)stream);
}

int cvr_pcg_multi(cvr_handle *h, const cvr_precond *p, const void *B_host, void *X_host, int32_t nvec, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_pcg_multi(h, p, B_host, X_host, nvec, nvec, nvec, opt, res)) return rc;
    return solve_block_from_host(h, B_host, X_host, nvec, [&](const void *B, void *X, hipStream_t st) { return cg_multi_device(h, p, B, nvec, X, nvec, nvec, opt, res, st); });
}

}  // extern "C"
