// cvr_minres.hip -- MINRES (Paige & Saunders, SIAM J. Numer. Anal. 12, 1975) on the device for (A - shift I) x = b with A symmetric, indefinite and
// singular consistent systems included (include/cvr_amd.h: cvr_minres_device, cvr_minres): cvr_cg.hip's plan with the symmetric Lanczos process and
// one Givens rotation per step.  Per step, beside the SpMV q = A v (run_spmv: cvr_spmv_device's path), three vector launches:
//   minres_yp_kernel   y' = (q - shift v) - (beta / oldb) r1 in r1's place (dead from here on) and the partial sums of v . y'
//   minres_r_kernel    alfa = v . y' from those partials; y = y' - (alfa / beta) r2 in the same buffer, z = minv .* y and the partial sums of y . z
//   minres_x_kernel    alfa and beta' = sqrt(y . z) from the two sets of partials, the rotation, the breakdown test, w = ((v - oldeps w1) - delta w2) / gamma
//                      in w1's place, x += phi w, the stop test; not stopped: v = z / beta'
// The two r buffers and the two w buffers swap roles by the step's parity (y becomes r2, r2 becomes r1; w becomes w2, w2 becomes w1), so no pass copies
// a vector.  17 vector passes per step with a diagonal preconditioner (q v r1 y' | y' r2 minv y z | x v w1 w2 x w z v, less two at the stop and r1 at
// step 0), 15 without one (no minv, no z: z is y itself), all in 16-byte packets; the sums, the grid and the packet helpers are cvr_krylov.h's, so a call
// gives the same bits every time.
// The scalars that outlive a kernel sit in a state cell (MinresCell) that workgroup 0 writes, double-buffered by step parity where a workgroup reads what
// another one of the same launch writes; the kernel that finds a stop records it there and every later kernel of the batch returns without writing -- the
// result does not depend on how many steps the host enqueues between two read-backs.
// The host side is cvr_krylov.h's driver: the cell and the kernels are in cvr_minres_kernels.h, this file adds the step and the read-back.
// (The reference has no solver: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_minres_kernels.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

// the library's buffers of one call: v (x_ext: an SpMV input, x0 at the start), q (y_ext), the two r (r[0] y_ext: it takes the scaled product), the
// two w, z (with minv_dev only), three sets of partial sums (v . y' | r2 . z | -; at the start b . b | b . M^-1 b | r2 . z), the cell
template <typename T>
struct Workspace {
    T          *v, *q, *r[2], *w[2], *z;
    double     *part;
    MinresCell *cell;
};

int check_shift(double shift)
{
    if (!std::isfinite(shift)) return fail(CVR_ERR_INVALID, "cvr_minres: shift = %g: must be finite", shift);
    return CVR_OK;
}

// what comes before any device work and before the handle is looked at
int check_args(const cvr_handle *h, const void *b, const void *x, double shift, const cvr_cg_options *opt, const cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, b, x, opt, res)) return rc;
    return check_shift(shift);
}

// the three vector launches of step k (the SpMV q = A v is enqueued in front of them); without a preconditioner z is the new r2
template <typename T>
hipError_t launch_step(const Workspace<T> &w, T *x, const T *minv, long long n, bool al_x, bool al_minv, int k, double shift, double rtol, hipStream_t st)
{
    T *r2 = w.r[k & 1], *r1 = w.r[(k + 1) & 1];          // y' and y are written in r1's place: the next step's r2
    with_flags([&](auto SHIFT, auto R1) { launch(minres_yp_kernel<T, SHIFT, R1>, st, w.q, w.v, r1, n, w.part, w.cell, k, shift); }, shift != 0, k > 0);
    with_flags([&](auto PRE, auto AL) { launch(minres_r_kernel<T, PRE, AL || !PRE>, st, r1, r2, minv, w.z, n, w.part, w.part + kBlocks, w.cell, k); }, minv != nullptr, al_minv);
    with_flags([&](auto AL) { launch(minres_x_kernel<T, AL>, st, x, w.v, w.w[k & 1], w.w[(k + 1) & 1], minv ? w.z : r1, n, w.part, w.cell, k, rtol); }, al_x);
    return hipGetLastError();
}

// cvr_krylov.h's driver with MINRES's start, step and cell
template <typename T>
int minres_solve(cvr_handle *h, const T *b, T *x, double shift, const cvr_cg_options *opt, cvr_cg_result *res, cvr_minres_info *info, hipStream_t st)
{
    const long long n = h->info.nrows;
    const size_t    vb = sizeof(T) * (size_t)n;
    const T        *minv = static_cast<const T *>(opt->minv_dev);
    const bool      al_b = (((uintptr_t)b | (uintptr_t)minv) & 15u) == 0, al_x = ((uintptr_t)x & 15u) == 0, al_minv = ((uintptr_t)minv & 15u) == 0;

    Arena        a;
    const size_t ov = a.add(x_ext_bytes(h)), oq = a.add(y_ext_bytes(h)), or0 = a.add(y_ext_bytes(h)), or1 = a.add(vec_bytes(h));
    const size_t ow = a.add(2 * Arena::slot(vec_bytes(h))), oz = a.add(minv ? vec_bytes(h) : 0);
    const size_t opart = a.add(sizeof(double) * 3 * kBlocks), ocell = a.add(sizeof(MinresCell));
    HIP_TRY(a.alloc());
    const Workspace<T> w{a.at<T>(ov), a.at<T>(oq), {a.at<T>(or0), a.at<T>(or1)}, {a.at<T>(ow), a.at<T>(ow + Arena::slot(vec_bytes(h)))}, minv ? a.at<T>(oz) : nullptr,
                         a.at<double>(opart), a.at<MinresCell>(ocell)};
    if (const int rc = a.begin(st)) return rc;

    // v = x0 for the moment (with its pad slot), r2 = b; r2 = b - A x0; w1 = w2 = 0; then r2 += shift x0, z, the start's sums, the cell and the first v
    if (const int rc = zero_pad_slot(w.v, vb, sizeof(T), st)) return rc;
    if (const int rc = start_residual(h, w.v, w.r[0], x, b, n, st)) return rc;
    int spmvs = 1;
    HIP_TRY(hipMemsetAsync(w.w[0], 0, 2 * Arena::slot(vec_bytes(h)), st));
    with_flags([&](auto PRE, auto AL) { launch(minres_init_kernel<T, PRE, AL>, st, b, minv, w.v, w.r[0], w.z, n, shift, w.part); }, minv != nullptr, al_b);
    launch(minres_start_kernel<T>, st, minv ? w.z : w.r[0], w.v, n, w.part, minv ? 1 : 0, w.cell, opt->rtol);
    HIP_TRY(hipGetLastError());

    MinresCell cell{};
    const int  rc = run_batches(
        opt,
        [&](int k) -> int {
            HIP_TRY(run_spmv(h, w.v, w.q, st));
            spmvs++;
            HIP_TRY(launch_step(w, x, minv, n, al_x, al_minv, k, shift, opt->rtol, st));
            return CVR_OK;
        },
        [&](int, bool *stopped) -> int {
            if (const int rc = read_cell(&cell, w.cell, sizeof(cell), st)) return rc;
            *stopped = cell.stop != 0;
            return CVR_OK;
        });
    if (rc) return rc;
    if (const int rc = finish_solve(a, st, x, vb, cell, spmvs, res)) return rc;
    if (info) {
        memset(info, 0, sizeof(*info));
        info->anorm = cell.anorm;
        info->acond = cell.acond;
    }
    return CVR_OK;
}

// behind the argument checks
int minres_device(cvr_handle *h, const void *b, void *x, double shift, const cvr_cg_options *opt, cvr_cg_result *res, cvr_minres_info *info, hipStream_t st)
{
    if (const int rc = check_square_preprocessed(h, "cvr_minres", "MINRES needs")) return rc;
    Range range("cvr_minres_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) { return minres_solve(h, static_cast<const decltype(t) *>(b), static_cast<decltype(t) *>(x), shift, opt, res, info, st); });
}

}  // namespace

extern "C" {

int cvr_minres_device(cvr_handle *h, const void *b_dev, void *x_dev, double shift, const cvr_cg_options *opt, cvr_cg_result *res, cvr_minres_info *info, void *stream)
{
    if (const int rc = check_args(h, b_dev, x_dev, shift, opt, res)) return rc;
    return minres_device(h, b_dev, x_dev, shift, opt, res, info, (hipStream_t)stream);
}

int cvr_minres(cvr_handle *h, const void *b_host, void *x_host, double shift, const cvr_cg_options *opt, cvr_cg_result *res, cvr_minres_info *info)
{
    if (const int rc = check_args(h, b_host, x_host, shift, opt, res)) return rc;
    if (const int rc = check_square_preprocessed(h, "cvr_minres", "MINRES needs")) return rc;
    return solve_from_host(h, b_host, x_host, [&](const void *b, void *x, hipStream_t st) { return minres_device(h, b, x, shift, opt, res, info, st); });
}

}  // extern "C"
