// cvr_svds.hip -- the nev largest singular values of A, of any shape, with their left and right vectors on the device (include/cvr_amd.h:
// cvr_svds_device, cvr_svds, cvr_svd_host): Golub-Kahan-Lanczos bidiagonalisation with full two-sided reorthogonalisation and a thick restart on Ritz
// vectors (Baglama and Reichel, SIAM J. Sci. Comput. 27, 2005; Hernandez, Roman and Tomas, ETNA 31, 2008), the rectangular twin of cvr_lanczos.hip.
// Two handles, A (nrows x ncols) and A^T (usually cvr_options.transpose = 1 on the same CSR), as in cvr_lsqr.hip.  Step j is two halves, each a
// product through run_spmv (cvr_spmv_device's path) and five vector launches (three in the left half of step 0, which has no column to work against):
//   w = A v_j
//   svds_dots_kernel      the partial sums of u_i . w for i < j (cvr_basis_groups.h's dot_group, GMRES's)
//   svds_update_kernel    the coefficients from those partials; w -= sum c_i u_i in one pass over the basis and the partial sums of w . w
//   svds_dots_kernel      the same on the new w (classical Gram-Schmidt, applied twice)
//   svds_update_kernel    the same, and the partial sums of w . w
//   svds_finish_kernel    alpha_j = sqrt(w . w), the breakdown test and the closed-space test (w . w of the two passes) into the state cell;
//                         u_j = w / alpha_j
//   z = A^T u_j, and the same five over ncols values against v_0 .. v_j: beta_(j+1) = sqrt(z . z), v_(j+1) = z / beta_(j+1)
// Within a cycle nothing is read back: alpha and beta sit in the state cell (SvdCell), which the host reads once per cycle; it then takes the
// projected matrix apart (svd_small: cvr_svdsmall.cpp), tests the wanted triplets and, to go on, enqueues the restart: lanczos_restart_kernel
// (cvr_lanczos_kernels.h, as it is) once per basis into a block of its own, the blocks copied back over the bases, and v_m into v_k.  The returned
// vectors are the same kernel's output into the caller's arrays.  The kernel that finds a breakdown or a closed space records it and every later
// kernel of the cycle returns without writing.  The host side is cvr_krylov.h's pieces (Arena, zero_pad_slot, launch, with_value_type, with_flags).
// (The reference has no solver: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_lanczos_kernels.h"
#include "cvr_svds_kernels.h"

namespace cvrh {
int svd_small(int p, int q, const double *b, int ldb, double *s, double *uq, int lduq, double *vp, int ldvp);          // cvr_svdsmall.cpp
}

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

static_assert(kSvdMaxM == kEigMaxM, "the restart product's coefficient rows are kEigMaxM wide");
constexpr double kEps23 = CVR_EIG_EPS23;
constexpr int    kLd = kSvdMaxM + 1;          // the leading dimension of the host's small matrices

// what comes before any device work and before a handle is looked at, in the header's order
int check_args(const void *a, const void *at, const void *v0, const double *svals, const void *U, int64_t ldu, const void *V, int64_t ldv,
               const cvr_svd_options *opt, const cvr_svd_result *res)
{
    if (!a) return fail(CVR_ERR_INVALID, "cvr_svds: null a");
    if (!at) return fail(CVR_ERR_INVALID, "cvr_svds: null handle of the transpose");
    if (!v0) return fail(CVR_ERR_INVALID, "cvr_svds: null v0");
    if (!svals) return fail(CVR_ERR_INVALID, "cvr_svds: null svals");
    if (!opt) return fail(CVR_ERR_INVALID, "cvr_svds: null opt");
    if (!res) return fail(CVR_ERR_INVALID, "cvr_svds: null res");
    if (opt->nev < 1) return fail(CVR_ERR_INVALID, "cvr_svds: nev = %d: must be at least 1", opt->nev);
    if (opt->ncv != 0 && (opt->ncv < (int64_t)opt->nev + 2 || opt->ncv > CVR_SVD_MAX_NCV))
        return fail(CVR_ERR_INVALID, "cvr_svds: ncv = %d: must be 0 or in nev + 2 .. %d", opt->ncv, CVR_SVD_MAX_NCV);
    if (opt->max_restarts < 0) return fail(CVR_ERR_INVALID, "cvr_svds: max_restarts = %d: must not be negative", opt->max_restarts);
    if (opt->reserved0 != 0) return fail(CVR_ERR_INVALID, "cvr_svd_options.reserved0 = %d: must be 0", opt->reserved0);
    if (!(opt->tol >= 0) || !std::isfinite(opt->tol)) return fail(CVR_ERR_INVALID, "cvr_svds: tol = %g: must be finite and not negative", opt->tol);
    for (int i = 0; i < 4; i++)
        if (opt->reserved[i] != 0) return fail(CVR_ERR_INVALID, "cvr_svd_options.reserved[%d] = %d: must be 0", i, opt->reserved[i]);
    if (U && ldu < 1) return fail(CVR_ERR_INVALID, "cvr_svds: ldu = %lld: must be at least 1", (long long)ldu);
    if (V && ldv < 1) return fail(CVR_ERR_INVALID, "cvr_svds: ldv = %lld: must be at least 1", (long long)ldv);
    return CVR_OK;
}

// ... and what follows on the handles; *m: ncv with the default resolved
int check_handles(const cvr_handle *a, const cvr_handle *at, const void *U, int64_t ldu, const void *V, int64_t ldv, const cvr_svd_options *opt, int *m)
{
    if (!a->converted || !at->converted) return fail(CVR_ERR_STATE, "cvr_svds before cvr_preprocess");
    if (at->info.nrows != a->info.ncols || at->info.ncols != a->info.nrows)
        return fail(CVR_ERR_INVALID, "cvr_svds: A is %lld x %lld, the handle of its transpose %lld x %lld", (long long)a->info.nrows, (long long)a->info.ncols,
                    (long long)at->info.nrows, (long long)at->info.ncols);
    if (a->vsz != at->vsz) return fail(CVR_ERR_INVALID, "cvr_svds: the two handles hold different value types");
    if (a->device != at->device) return fail(CVR_ERR_INVALID, "cvr_svds: the two handles are on devices %d and %d", a->device, at->device);
    const int64_t small = std::min(a->info.nrows, a->info.ncols);
    const int64_t ncv = opt->ncv ? opt->ncv : std::min<int64_t>({small, std::max<int64_t>(2 * (int64_t)opt->nev + 1, 20), CVR_SVD_MAX_NCV});
    if (ncv > small) return fail(CVR_ERR_INVALID, "cvr_svds: ncv = %lld exceeds min(nrows, ncols) = %lld", (long long)ncv, (long long)small);
    if (ncv < (int64_t)opt->nev + 2)
        return fail(CVR_ERR_INVALID, "cvr_svds: the default ncv = %lld is below nev + 2 = %lld (min(nrows, ncols) = %lld)", (long long)ncv, (long long)opt->nev + 2, (long long)small);
    if (U && ldu < a->info.nrows) return fail(CVR_ERR_INVALID, "cvr_svds: ldu = %lld is below nrows = %lld", (long long)ldu, (long long)a->info.nrows);
    if (V && ldv < a->info.ncols) return fail(CVR_ERR_INVALID, "cvr_svds: ldv = %lld is below ncols = %lld", (long long)ldv, (long long)a->info.ncols);
    *m = (int)ncv;
    return CVR_OK;
}

// One basis of the call: its columns (SpMV inputs of one handle: whole slots, element `len` of each stays 0) and the block that takes the restart's output
template <typename T>
struct Basis {
    T         *cols, *out;
    long long  stride, len;          // in values
    T         *col(int i) const { return cols + (long long)i * stride; }
};

// the library's buffers of one call: the right basis (m + 1 columns over ncols values, A's inputs), the left one (m columns over nrows values, A^T's
// inputs), w (A's y_ext), z (A^T's y_ext), the partial sums of the dots (one set per column) and of v0 . v0 / w . w, the restart's coefficients, the cell
template <typename T>
struct Workspace {
    Basis<T>  V, U;
    T        *w, *z;
    double   *part_h, *part_s, *S;
    SvdCell  *cell;
};

// one half step: `x` (the product's output, over b.len values) against the first ncols columns of b; the new column is `next`
template <typename T, bool LEFT>
hipError_t launch_half(const Workspace<T> &w, const Basis<T> &b, T *x, int ncols, T *next, int j, hipStream_t st)
{
    if (ncols) launch(svds_dots_kernel<T>, st, (const T *)b.cols, b.stride, (const T *)x, b.len, ncols, w.part_h, (const SvdCell *)w.cell);
    launch(svds_update_kernel<T, false>, st, (const T *)b.cols, b.stride, x, b.len, ncols, (const double *)w.part_h, w.part_s, (const SvdCell *)w.cell);
    if (ncols) launch(svds_dots_kernel<T>, st, (const T *)b.cols, b.stride, (const T *)x, b.len, ncols, w.part_h, (const SvdCell *)w.cell);
    launch(svds_update_kernel<T, true>, st, (const T *)b.cols, b.stride, x, b.len, ncols, (const double *)w.part_h, w.part_s, (const SvdCell *)w.cell);
    launch(svds_finish_kernel<T, LEFT>, st, (const T *)x, next, b.len, (const double *)w.part_s, w.cell, j);
    return hipGetLastError();
}

// out[:, c] = B[:, 0..rows-1] . S[:, c] for c < nout, S's column c at S + c * kLd; `coef` is the host's copy of the coefficients, which lives until
// the stream is synchronised (one per product of a cycle: the copy is asynchronous)
template <typename T>
int launch_product(const Workspace<T> &w, const Basis<T> &b, int rows, const double *S, int nout, std::vector<double> &coef, T *out, long long ldo, bool al,
                   hipStream_t st)
{
    coef.assign((size_t)rows * kEigMaxM, 0.0);
    for (int l = 0; l < rows; l++)
        for (int c = 0; c < nout; c++) coef[(size_t)l * kEigMaxM + c] = S[(size_t)c * kLd + l];
    HIP_TRY(hipMemcpyAsync(w.S, coef.data(), sizeof(double) * coef.size(), hipMemcpyHostToDevice, st));
    with_flags([&](auto AL) { launch(lanczos_restart_kernel<T, AL>, st, (const T *)b.cols, b.stride, rows, (const double *)w.S, nout, out, ldo, b.len); }, al);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

template <typename T>
int svds_solve(cvr_handle *a, cvr_handle *at, const T *v0, double *svals, T *Uo, int64_t ldu, T *Vo, int64_t ldv, int m, const cvr_svd_options *opt,
               cvr_svd_result *res, hipStream_t st)
{
    const long long nr = a->info.nrows, nc = a->info.ncols;
    const int       nev = opt->nev, kmax = nev + (m - nev) / 2;
    const bool      al_v0 = ((uintptr_t)v0 & 15u) == 0;
    const bool      al_u = Uo && (((uintptr_t)Uo | (uintptr_t)(ldu * (int64_t)sizeof(T))) & 15u) == 0;
    const bool      al_v = Vo && (((uintptr_t)Vo | (uintptr_t)(ldv * (int64_t)sizeof(T))) & 15u) == 0;

    Arena        ar;
    const size_t nxv = Arena::slot(sizeof(T) * (size_t)std::max<int64_t>(a->info.x_elems, nc + 1));           // a right column: an input of A
    const size_t nxu = Arena::slot(sizeof(T) * (size_t)std::max<int64_t>(at->info.x_elems, nr + 1));          // a left column: an input of A^T
    const size_t oV = ar.add((size_t)(m + 1) * nxv), oU = ar.add((size_t)m * nxu);
    const size_t ow = ar.add(sizeof(T) * (size_t)std::max<int64_t>({a->info.yext_elems, nr, 1})), oz = ar.add(sizeof(T) * (size_t)std::max<int64_t>({at->info.yext_elems, nc, 1}));
    const size_t ooV = ar.add((size_t)kmax * nxv), ooU = ar.add((size_t)kmax * nxu);
    const size_t oh = ar.add(sizeof(double) * (size_t)m * kBlocks), os = ar.add(sizeof(double) * 2 * kBlocks), oS = ar.add(sizeof(double) * kEigMaxM * kEigMaxM);
    const size_t ocell = ar.add(sizeof(SvdCell));
    const hipError_t e = ar.alloc();
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(CVR_ERR_NOMEM, "cvr_svds: no device memory for %d basis vectors (%zu bytes)", 2 * m + 1 + 2 * kmax, ar.total());
    }
    HIP_TRY(e);
    const Workspace<T> w{{ar.at<T>(oV), ar.at<T>(ooV), (long long)(nxv / sizeof(T)), nc}, {ar.at<T>(oU), ar.at<T>(ooU), (long long)(nxu / sizeof(T)), nr},
                         ar.at<T>(ow), ar.at<T>(oz), ar.at<double>(oh), ar.at<double>(os), ar.at<double>(oS), ar.at<SvdCell>(ocell)};
    if (const int rc = ar.begin(st)) return rc;

    // the pad slots of the SpMV inputs (the output blocks are copied back slot by slot: their pad slots too); s = v0 . v0, the cell and v_0
    for (int i = 0; i <= m; i++)
        if (const int rc = zero_pad_slot(w.V.col(i), sizeof(T) * (size_t)nc, sizeof(T), st)) return rc;
    for (int i = 0; i < m; i++)
        if (const int rc = zero_pad_slot(w.U.col(i), sizeof(T) * (size_t)nr, sizeof(T), st)) return rc;
    for (int i = 0; i < kmax; i++) {
        if (const int rc = zero_pad_slot(w.V.out + (long long)i * w.V.stride, sizeof(T) * (size_t)nc, sizeof(T), st)) return rc;
        if (const int rc = zero_pad_slot(w.U.out + (long long)i * w.U.stride, sizeof(T) * (size_t)nr, sizeof(T), st)) return rc;
    }
    with_flags([&](auto AL) {
        launch(lanczos_vv_kernel<T, AL>, st, v0, nc, w.part_s);
        launch(svds_begin_kernel<T, AL>, st, v0, w.V.col(0), nc, (const double *)w.part_s, w.cell);
    }, al_v0);
    HIP_TRY(hipGetLastError());

    std::vector<double> sigma(kLd), spike(kLd), B((size_t)kLd * kLd), sv(kLd), Q((size_t)kLd * kLd), P((size_t)kLd * kLd), est(kLd), coef_u, coef_v;
    SvdCell             cell{};
    int                 k = 0, restarts = 0, spmvs = 0, nconv = 0, status = CVR_EIG_MAX_RESTARTS, nret = 0;
    double              worst = 0;
    for (;;) {
        for (int j = k; j < m; j++) {
            HIP_TRY(run_spmv(a, w.V.col(j), w.w, st));
            HIP_TRY((launch_half<T, true>(w, w.U, w.w, j, w.U.col(j), j, st)));
            HIP_TRY(run_spmv(at, w.U.col(j), w.z, st));
            HIP_TRY((launch_half<T, false>(w, w.V, w.z, j + 1, w.V.col(j + 1), j, st)));
            spmvs += 2;
        }
        if (const int rc = read_cell(&cell, w.cell, sizeof(cell), st)) return rc;
        if (cell.status == CVR_EIG_BREAKDOWN) {
            status = CVR_EIG_BREAKDOWN;
            nconv = 0;
            break;
        }
        // the projected matrix: p rows (left vectors) by q columns (right vectors); a closed left half leaves one column more than rows
        const bool closed_l = cell.status == kSvdClosedLeft, closed = closed_l || cell.status == kSvdClosedRight;
        const int  p = closed_l ? cell.j : closed ? cell.j + 1 : m, q = closed_l ? p + 1 : p;
        if (p == 0) {          // A v_0 == 0: nothing to return
            status = CVR_EIG_INVARIANT;
            nconv = 0;
            break;
        }
        std::fill(B.begin(), B.end(), 0.0);
        for (int c = 0; c < k && c < p; c++) {
            B[(size_t)c * kLd + c] = sigma[c];
            if (k < q) B[(size_t)k * kLd + c] = spike[c];
        }
        for (int j = k; j < p; j++) {
            B[(size_t)j * kLd + j] = cell.alpha[j];
            if (j + 1 < q) B[(size_t)(j + 1) * kLd + j] = cell.beta[j + 1];
        }
        if (svd_small(p, q, B.data(), kLd, sv.data(), Q.data(), kLd, P.data(), kLd))
            return fail(CVR_ERR_INTERNAL, "cvr_svds: the projected problem of %d x %d did not converge", p, q);
        // the wanted triplets, descending, their estimates and the count of converged ones
        const int    want = std::min(nev, p);
        const double bq = closed ? 0.0 : cell.beta[m];
        nconv = 0;
        worst = 0;
        for (int c = 0; c < want; c++) {
            const double scale = std::max(kEps23, sv[c]);
            est[c] = std::fabs(bq * Q[(size_t)c * kLd + p - 1]);
            if (est[c] <= opt->tol * scale) nconv++;
            worst = std::max(worst, est[c] / scale);
        }
        const bool all = closed || nconv == nev;
        if (all || restarts == opt->max_restarts) {
            status = closed ? (p >= nev ? CVR_EIG_CONVERGED : CVR_EIG_INVARIANT) : all ? CVR_EIG_CONVERGED : CVR_EIG_MAX_RESTARTS;
            if (closed) nconv = want;
            nret = want;
            for (int c = 0; c < want; c++) svals[c] = sv[c];
            if (Uo)
                if (const int rc = launch_product(w, w.U, p, Q.data(), want, coef_u, Uo, (long long)ldu, al_u, st)) return rc;
            if (Vo)
                if (const int rc = launch_product(w, w.V, q, P.data(), want, coef_v, Vo, (long long)ldv, al_v, st)) return rc;
            break;
        }
        // the thick restart: keep the kk leading Ritz triplets
        const int kk = nev + std::min(nconv, (m - nev) / 2);
        for (int c = 0; c < kk; c++) {
            sigma[c] = sv[c];
            spike[c] = cell.beta[m] * Q[(size_t)c * kLd + m - 1];
        }
        if (const int rc = launch_product(w, w.U, m, Q.data(), kk, coef_u, w.U.out, w.U.stride, true, st)) return rc;
        if (const int rc = launch_product(w, w.V, m, P.data(), kk, coef_v, w.V.out, w.V.stride, true, st)) return rc;
        HIP_TRY(hipMemcpyAsync(w.U.cols, w.U.out, (size_t)kk * nxu, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(w.V.cols, w.V.out, (size_t)kk * nxv, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(w.V.col(kk), w.V.col(m), sizeof(T) * (size_t)nc, hipMemcpyDeviceToDevice, st));
        k = kk;
        restarts++;
    }
    double seconds = 0;
    if (const int rc = ar.seconds(st, &seconds)) return rc;
    memset(res, 0, sizeof(*res));
    res->nconv = nconv;
    res->status = status;
    res->restarts = restarts;
    res->spmv_count = spmvs;
    res->seconds = seconds;
    res->max_estimate = nret ? worst : 0.0;
    return CVR_OK;
}

// behind the argument checks
int svds_device(cvr_handle *a, cvr_handle *at, const void *v0, double *svals, void *U, int64_t ldu, void *V, int64_t ldv, const cvr_svd_options *opt,
                cvr_svd_result *res, hipStream_t st)
{
    int m = 0;
    if (const int rc = check_handles(a, at, U, ldu, V, ldv, opt, &m)) return rc;
    Range range("cvr_svds_device");
    HIP_TRY(hipSetDevice(a->device));
    return with_value_type(a, [&](auto t) {
        using T = decltype(t);
        return svds_solve(a, at, static_cast<const T *>(v0), svals, static_cast<T *>(U), ldu, static_cast<T *>(V), ldv, m, opt, res, st);
    });
}

}  // namespace

extern "C" {

void cvr_svd_default_options(cvr_svd_options *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->nev = 1;
    opt->ncv = 0;
    opt->max_restarts = 100;
    opt->tol = 1e-8;
}

int cvr_svds_device(cvr_handle *a, cvr_handle *at, const void *v0_dev, double *svals_host, void *U_dev, int64_t ldu, void *V_dev, int64_t ldv,
                    const cvr_svd_options *opt, cvr_svd_result *res, void *stream)
{
    if (const int rc = check_args(a, at, v0_dev, svals_host, U_dev, ldu, V_dev, ldv, opt, res)) return rc;
    return svds_device(a, at, v0_dev, svals_host, U_dev, ldu, V_dev, ldv, opt, res, (hipStream_t)stream);
}

int cvr_svds(cvr_handle *a, cvr_handle *at, const void *v0_host, double *svals_host, void *U_host, int64_t ldu, void *V_host, int64_t ldv,
             const cvr_svd_options *opt, cvr_svd_result *res)
{
    if (const int rc = check_args(a, at, v0_host, svals_host, U_host, ldu, V_host, ldv, opt, res)) return rc;
    int m = 0;
    if (const int rc = check_handles(a, at, U_host, ldu, V_host, ldv, opt, &m)) return rc;
    HIP_TRY(hipSetDevice(a->device));
    // v0 rides in A's own x (ncols + 1 values); the vectors come back through a block of the call: nev columns of nrows values, then nev of ncols
    const size_t ub = a->vsz * (size_t)a->info.nrows, vb = a->vsz * (size_t)a->info.ncols, nev = (size_t)opt->nev;
    uint8_t     *block = nullptr;
    if (U_host || V_host) {
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&block), std::max<size_t>((ub + vb) * nev, 16));
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            return fail(CVR_ERR_NOMEM, "cvr_svds: no device memory for %d pairs of vectors", opt->nev);
        }
        HIP_TRY(e);
    }
    uint8_t *ublock = U_host ? block : nullptr, *vblock = V_host ? block + ub * nev : nullptr;
    auto     run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(a->d_x, v0_host, vb, hipMemcpyHostToDevice, a->stream));
        if (const int rc = svds_device(a, at, a->d_x, svals_host, ublock, a->info.nrows, vblock, a->info.ncols, opt, res, a->stream)) return rc;
        const int nret = res->status == CVR_EIG_BREAKDOWN ? 0 : res->status == CVR_EIG_INVARIANT ? res->nconv : opt->nev;
        if (ublock && nret) HIP_TRY(hipMemcpy2DAsync(U_host, a->vsz * (size_t)ldu, ublock, ub, ub, (size_t)nret, hipMemcpyDeviceToHost, a->stream));
        if (vblock && nret) HIP_TRY(hipMemcpy2DAsync(V_host, a->vsz * (size_t)ldv, vblock, vb, vb, (size_t)nret, hipMemcpyDeviceToHost, a->stream));
        HIP_TRY(hipStreamSynchronize(a->stream));
        return CVR_OK;
    };
    const int rc = run();
    if (block) (void)hipFree(block);
    return rc;
}

int cvr_svd_host(int32_t p, int32_t q, const double *b, int32_t ldb, double *s, double *uq, int32_t lduq, double *vp, int32_t ldvp)
{
    if (p < 1 || q < p || q > CVR_SVD_MAX_NCV + 1) return fail(CVR_ERR_INVALID, "cvr_svd_host: p = %d, q = %d: must be 1 <= p <= q <= %d", p, q, CVR_SVD_MAX_NCV + 1);
    if (!b || !s) return fail(CVR_ERR_INVALID, "cvr_svd_host: null b or s");
    if (ldb < p || (uq && lduq < p) || (vp && ldvp < q))
        return fail(CVR_ERR_INVALID, "cvr_svd_host: ldb = %d, lduq = %d, ldvp = %d: must be at least p = %d, p and q = %d", ldb, lduq, ldvp, p, q);
    for (int j = 0; j < q; j++)
        for (int i = 0; i < p; i++)
            if (!std::isfinite(b[(size_t)j * ldb + i])) return fail(CVR_ERR_INVALID, "cvr_svd_host: b(%d, %d) is not finite", i, j);
    if (svd_small(p, q, b, ldb, s, uq, lduq, vp, ldvp)) return fail(CVR_ERR_INTERNAL, "cvr_svd_host: no convergence");
    return CVR_OK;
}

}  // extern "C"
