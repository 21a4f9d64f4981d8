// cvr_lanczos.hip -- a few extreme eigenpairs of a symmetric A on the device (include/cvr_amd.h: cvr_eigsh_device, cvr_eigsh, cvr_sym_eig_host): the
// Lanczos process with full reorthogonalisation and the thick restart of Wu and Simon (SIAM J. Matrix Anal. Appl. 22, 2000), on cvr_gmres.hip's plan.
// Per step with basis column j, beside the SpMV w = A v_j (run_spmv: cvr_spmv_device's path), five vector launches, whatever j:
//   lanczos_dots_kernel      the partial sums of v_i . w for i = 0..j (cvr_basis_groups.h's dot_group, GMRES's)
//   lanczos_update_kernel    h_i from those partials; w -= sum h_i v_i in one pass over the basis and the partial sums of w . w; workgroup 0 keeps h_j
//   lanczos_dots_kernel      the same on the new w (classical Gram-Schmidt, applied twice)
//   lanczos_update_kernel    d_i, w -= sum d_i v_i and the partial sums of w . w; workgroup 0: alpha_j = h_j + d_j
//   lanczos_finish_kernel    beta_(j+1) = sqrt(w . w), the breakdown test and the closed-space test (w . w of the two passes) into the state cell;
//                            v_(j+1) = w / beta_(j+1)
// Within a cycle nothing is read back: alpha and beta sit in the state cell (LanCell), which the host reads once per cycle; it then solves the projected
// problem (cvr_sym_eig_host: cvr_symeig.cpp), tests the wanted pairs and, to go on, enqueues the restart:
//   lanczos_restart_kernel   V_out[:, 0..k-1] = V[:, 0..m-1] . S[:, kept], a tall-skinny product: a thread owns its 16-byte packets, the output columns in
//                            compile-time groups of up to 8 (fp64 accumulators in registers), the input columns streamed 8 packets at a time, S in LDS
//   two device copies        V_out back over v_0 .. v_(k-1) (the product's output is a block of its own: no workgroup reads a column another one writes),
//                            and v_m into v_k
// The returned vectors are the same kernel's output into the caller's array.  The kernel that finds a breakdown or a closed space records it and every later
// kernel of the cycle returns without writing.  The host side is cvr_krylov.h's pieces (Arena, zero_pad_slot, launch, with_value_type, with_flags).
// (The reference has no solver: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_lanczos_kernels.h"

namespace cvrh {
int sym_eig(int m, const double *a, int lda, double *w, double *z, int ldz);          // cvr_symeig.cpp
}

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

constexpr double kEps23 = CVR_EIG_EPS23;

// what comes before any device work and before the handle is looked at, in the header's order
int check_args(const void *h, const void *v0, const double *evals, const void *evecs, int64_t ldv, const cvr_eig_options *opt, const cvr_eig_result *res)
{
    if (!h) return fail(CVR_ERR_INVALID, "cvr_eigsh: null h");
    if (!v0) return fail(CVR_ERR_INVALID, "cvr_eigsh: null v0");
    if (!evals) return fail(CVR_ERR_INVALID, "cvr_eigsh: null evals");
    if (!opt) return fail(CVR_ERR_INVALID, "cvr_eigsh: null opt");
    if (!res) return fail(CVR_ERR_INVALID, "cvr_eigsh: null res");
    if (opt->nev < 1) return fail(CVR_ERR_INVALID, "cvr_eigsh: nev = %d: must be at least 1", opt->nev);
    if (opt->ncv != 0 && (opt->ncv < (int64_t)opt->nev + 2 || opt->ncv > CVR_EIG_MAX_NCV))
        return fail(CVR_ERR_INVALID, "cvr_eigsh: ncv = %d: must be 0 or in nev + 2 .. %d", opt->ncv, CVR_EIG_MAX_NCV);
    if (opt->which != CVR_EIG_LARGEST && opt->which != CVR_EIG_SMALLEST) return fail(CVR_ERR_INVALID, "cvr_eigsh: which = %d: must be CVR_EIG_LARGEST or CVR_EIG_SMALLEST", opt->which);
    if (opt->max_restarts < 0) return fail(CVR_ERR_INVALID, "cvr_eigsh: max_restarts = %d: must not be negative", opt->max_restarts);
    if (!(opt->tol >= 0) || !std::isfinite(opt->tol)) return fail(CVR_ERR_INVALID, "cvr_eigsh: tol = %g: must be finite and not negative", opt->tol);
    for (int i = 0; i < 4; i++)
        if (opt->reserved[i] != 0) return fail(CVR_ERR_INVALID, "cvr_eig_options.reserved[%d] = %d: must be 0", i, opt->reserved[i]);
    if (evecs && ldv < 1) return fail(CVR_ERR_INVALID, "cvr_eigsh: ldv = %lld: must be at least 1", (long long)ldv);
    return CVR_OK;
}

// ... and what follows on the handle; *m: ncv with the default resolved
int check_handle(const cvr_handle *h, const void *evecs, int64_t ldv, const cvr_eig_options *opt, int *m)
{
    if (const int rc = check_square_preprocessed(h, "cvr_eigsh", "the eigensolver needs")) return rc;
    const int64_t n = h->info.nrows;
    const int64_t ncv = opt->ncv ? opt->ncv : std::min<int64_t>({n, std::max<int64_t>(2 * (int64_t)opt->nev + 1, 20), CVR_EIG_MAX_NCV});
    if (ncv > n) return fail(CVR_ERR_INVALID, "cvr_eigsh: ncv = %lld exceeds n = %lld", (long long)ncv, (long long)n);
    if (ncv < (int64_t)opt->nev + 2) return fail(CVR_ERR_INVALID, "cvr_eigsh: the default ncv = %lld is below nev + 2 = %lld (n = %lld)", (long long)ncv, (long long)opt->nev + 2, (long long)n);
    if (evecs && ldv < n) return fail(CVR_ERR_INVALID, "cvr_eigsh: ldv = %lld is below n = %lld", (long long)ldv, (long long)n);
    *m = (int)ncv;
    return CVR_OK;
}

// the library's buffers of one call: m + 1 basis vectors (x_ext each: SpMV inputs), w (y_ext), the restart's output block, the partial sums of the dots (one
// set per column) and of v0 . v0 / w . w, the restart's coefficients, the cell
template <typename T>
struct Workspace {
    T         *V, *w, *out;
    double    *part_h, *part_s, *S;
    LanCell   *cell;
    long long  stride;          // of the basis and of the output block, in values
    T         *basis(int i) const { return V + (long long)i * stride; }
};

template <typename T>
hipError_t launch_step(const Workspace<T> &w, long long n, int j, hipStream_t st)
{
    launch(lanczos_dots_kernel<T>, st, (const T *)w.V, w.stride, (const T *)w.w, n, j + 1, w.part_h, (const LanCell *)w.cell);
    launch(lanczos_update_kernel<T, false>, st, (const T *)w.V, w.stride, w.w, n, j, (const double *)w.part_h, w.part_s, w.cell);
    launch(lanczos_dots_kernel<T>, st, (const T *)w.V, w.stride, (const T *)w.w, n, j + 1, w.part_h, (const LanCell *)w.cell);
    launch(lanczos_update_kernel<T, true>, st, (const T *)w.V, w.stride, w.w, n, j, (const double *)w.part_h, w.part_s, w.cell);
    launch(lanczos_finish_kernel<T>, st, (const T *)w.w, w.basis(j + 1), n, (const double *)w.part_s, w.cell, j);
    return hipGetLastError();
}

// out[:, c] = V[:, 0..q-1] . S[:, sel[c]] for c < nout; `coef` is the host's copy of the coefficients, which lives until the stream is synchronised
template <typename T>
int launch_product(const Workspace<T> &w, int q, const double *S, int lds, const int *sel, int nout, std::vector<double> &coef, T *out, long long ldo, bool al, long long n,
                   hipStream_t st)
{
    coef.assign((size_t)q * kEigMaxM, 0.0);
    for (int l = 0; l < q; l++)
        for (int c = 0; c < nout; c++) coef[(size_t)l * kEigMaxM + c] = S[(size_t)sel[c] * lds + l];
    HIP_TRY(hipMemcpyAsync(w.S, coef.data(), sizeof(double) * coef.size(), hipMemcpyHostToDevice, st));
    with_flags([&](auto AL) { launch(lanczos_restart_kernel<T, AL>, st, (const T *)w.V, w.stride, q, (const double *)w.S, nout, out, ldo, n); }, al);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

template <typename T>
int eigsh_solve(cvr_handle *h, const T *v0, double *evals, T *evecs, int64_t ldv, int m, const cvr_eig_options *opt, cvr_eig_result *res, hipStream_t st)
{
    const long long n = h->info.nrows;
    const size_t    vb = sizeof(T) * (size_t)n;
    const int       nev = opt->nev, kmax = nev + (m - nev) / 2;
    const bool      al_v0 = ((uintptr_t)v0 & 15u) == 0, al_out = evecs && (((uintptr_t)evecs | (uintptr_t)(ldv * (int64_t)sizeof(T))) & 15u) == 0;

    Arena        a;
    const size_t nx = Arena::slot(x_ext_bytes(h));          // a basis vector: whole slots, so the stride is a whole number of values
    const size_t oV = a.add((size_t)(m + 1) * nx), ow = a.add(y_ext_bytes(h)), oo = a.add((size_t)kmax * nx);
    const size_t oh = a.add(sizeof(double) * (size_t)m * kBlocks), os = a.add(sizeof(double) * 2 * kBlocks), oS = a.add(sizeof(double) * kEigMaxM * kEigMaxM);
    const size_t ocell = a.add(sizeof(LanCell));
    const hipError_t e = a.alloc();
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(CVR_ERR_NOMEM, "cvr_eigsh: no device memory for %d basis vectors (%zu bytes)", m + 1 + kmax, a.total());
    }
    HIP_TRY(e);
    const Workspace<T> w{a.at<T>(oV), a.at<T>(ow), a.at<T>(oo), a.at<double>(oh), a.at<double>(os), a.at<double>(oS), a.at<LanCell>(ocell), (long long)(nx / sizeof(T))};
    if (const int rc = a.begin(st)) return rc;

    // the pad slots of the SpMV inputs (the output block is copied back slot by slot: its pad slots too); s = v0 . v0, the cell and v_0
    for (int i = 0; i <= m; i++)
        if (const int rc = zero_pad_slot(w.basis(i), vb, sizeof(T), st)) return rc;
    for (int i = 0; i < kmax; i++)
        if (const int rc = zero_pad_slot(w.out + (long long)i * w.stride, vb, sizeof(T), st)) return rc;
    with_flags([&](auto AL) {
        launch(lanczos_vv_kernel<T, AL>, st, v0, n, w.part_s);
        launch(lanczos_begin_kernel<T, AL>, st, v0, w.basis(0), n, (const double *)w.part_s, w.cell);
    }, al_v0);
    HIP_TRY(hipGetLastError());

    std::vector<double> theta(kEigMaxM), arrow(kEigMaxM), P((size_t)kEigMaxM * kEigMaxM), ev(kEigMaxM), S((size_t)kEigMaxM * kEigMaxM), coef;
    std::vector<double> est(kEigMaxM);
    int                 sel[kEigMaxM];
    LanCell             cell{};
    int                 k = 0, restarts = 0, spmvs = 0, nconv = 0, status = CVR_EIG_MAX_RESTARTS, nret = 0;
    double              worst = 0;
    for (;;) {
        for (int j = k; j < m; j++) {
            HIP_TRY(run_spmv(h, w.basis(j), w.w, st));
            HIP_TRY(launch_step(w, n, j, st));
            spmvs++;
        }
        if (const int rc = read_cell(&cell, w.cell, sizeof(cell), st)) return rc;
        if (cell.status == CVR_EIG_BREAKDOWN) {
            status = CVR_EIG_BREAKDOWN;
            nconv = 0;
            break;
        }
        const bool closed = cell.status == kEigInvariant;
        const int  q = closed ? cell.q : m;
        // the projected matrix, its lower triangle: the kept Ritz values with their arrow in row k, the tridiagonal beyond
        std::fill(P.begin(), P.begin() + (size_t)q * q, 0.0);
        for (int c = 0; c < k; c++) {
            P[(size_t)c * q + c] = theta[c];
            P[(size_t)c * q + k] = arrow[c];
        }
        for (int j = k; j < q; j++) {
            P[(size_t)j * q + j] = cell.alpha[j];
            if (j + 1 < q) P[(size_t)j * q + j + 1] = cell.beta[j + 1];
        }
        if (sym_eig(q, P.data(), q, ev.data(), S.data(), q)) return fail(CVR_ERR_INTERNAL, "cvr_eigsh: the projected problem of %d columns did not converge", q);
        // the wanted pairs, ascending, their estimates and the count of converged ones
        const int    want = std::min(nev, q), lo = opt->which == CVR_EIG_LARGEST ? q - want : 0;
        const double bq = closed ? 0.0 : cell.beta[q];
        nconv = 0;
        worst = 0;
        for (int c = 0; c < want; c++) {
            const double th = ev[lo + c], scale = std::max(kEps23, std::fabs(th));
            est[c] = std::fabs(bq * S[(size_t)(lo + c) * q + q - 1]);
            if (est[c] <= opt->tol * scale) nconv++;
            worst = std::max(worst, est[c] / scale);
        }
        const bool all = closed || nconv == nev;
        if (all || restarts == opt->max_restarts) {
            status = closed ? (q >= nev ? CVR_EIG_CONVERGED : CVR_EIG_INVARIANT) : all ? CVR_EIG_CONVERGED : CVR_EIG_MAX_RESTARTS;
            if (closed) nconv = want;
            nret = want;
            for (int c = 0; c < want; c++) {
                evals[c] = ev[lo + c];
                sel[c] = lo + c;
            }
            if (evecs)
                if (const int rc = launch_product(w, q, S.data(), q, sel, want, coef, evecs, (long long)ldv, al_out, n, st)) return rc;
            break;
        }
        // the thick restart: keep the kk Ritz pairs at the wanted end
        const int kk = nev + std::min(nconv, (m - nev) / 2), klo = opt->which == CVR_EIG_LARGEST ? m - kk : 0;
        for (int c = 0; c < kk; c++) {
            sel[c] = klo + c;
            theta[c] = ev[klo + c];
            arrow[c] = cell.beta[m] * S[(size_t)(klo + c) * m + m - 1];
        }
        if (const int rc = launch_product(w, m, S.data(), m, sel, kk, coef, w.out, w.stride, true, n, st)) return rc;
        HIP_TRY(hipMemcpyAsync(w.V, w.out, (size_t)kk * nx, hipMemcpyDeviceToDevice, st));
        if (vb) HIP_TRY(hipMemcpyAsync(w.basis(kk), w.basis(m), vb, hipMemcpyDeviceToDevice, st));
        k = kk;
        restarts++;
    }
    double seconds = 0;
    if (const int rc = a.seconds(st, &seconds)) return rc;
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
int eigsh_device(cvr_handle *h, const void *v0, double *evals, void *evecs, int64_t ldv, const cvr_eig_options *opt, cvr_eig_result *res, hipStream_t st)
{
    int m = 0;
    if (const int rc = check_handle(h, evecs, ldv, opt, &m)) return rc;
    Range range("cvr_eigsh_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) { return eigsh_solve(h, static_cast<const decltype(t) *>(v0), evals, static_cast<decltype(t) *>(evecs), ldv, m, opt, res, st); });
}

}  // namespace

extern "C" {

void cvr_eig_default_options(cvr_eig_options *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->nev = 1;
    opt->ncv = 0;
    opt->which = CVR_EIG_LARGEST;
    opt->max_restarts = 100;
    opt->tol = 1e-8;
}

int cvr_eigsh_device(cvr_handle *h, const void *v0_dev, double *evals_host, void *evecs_dev, int64_t ldv, const cvr_eig_options *opt, cvr_eig_result *res, void *stream)
{
    if (const int rc = check_args(h, v0_dev, evals_host, evecs_dev, ldv, opt, res)) return rc;
    return eigsh_device(h, v0_dev, evals_host, evecs_dev, ldv, opt, res, (hipStream_t)stream);
}

int cvr_eigsh(cvr_handle *h, const void *v0_host, double *evals_host, void *evecs_host, int64_t ldv, const cvr_eig_options *opt, cvr_eig_result *res)
{
    if (const int rc = check_args(h, v0_host, evals_host, evecs_host, ldv, opt, res)) return rc;
    int m = 0;
    if (const int rc = check_handle(h, evecs_host, ldv, opt, &m)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    // v0 rides in the handle's own x; the vectors come back through a block of the call (nev columns of n values, contiguous)
    const size_t vb = h->vsz * (size_t)h->info.nrows;
    uint8_t     *block = nullptr;
    if (evecs_host) {
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&block), std::max<size_t>(vb * (size_t)opt->nev, 16));
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            return fail(CVR_ERR_NOMEM, "cvr_eigsh: no device memory for %d vectors", opt->nev);
        }
        HIP_TRY(e);
    }
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(h->d_x, v0_host, vb, hipMemcpyHostToDevice, h->stream));
        if (const int rc = eigsh_device(h, h->d_x, evals_host, block, h->info.nrows, opt, res, h->stream)) return rc;
        const int nret = res->status == CVR_EIG_BREAKDOWN ? 0 : res->status == CVR_EIG_INVARIANT ? res->nconv : opt->nev;
        if (block && nret)
            HIP_TRY(hipMemcpy2DAsync(evecs_host, h->vsz * (size_t)ldv, block, vb, vb, (size_t)nret, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return CVR_OK;
    };
    const int rc = run();
    if (block) (void)hipFree(block);
    return rc;
}

int cvr_sym_eig_host(int32_t m, const double *a, int32_t lda, double *w, double *z, int32_t ldz)
{
    if (m < 1 || m > CVR_EIG_MAX_NCV) return fail(CVR_ERR_INVALID, "cvr_sym_eig_host: m = %d: must be in 1 .. %d", m, CVR_EIG_MAX_NCV);
    if (!a || !w) return fail(CVR_ERR_INVALID, "cvr_sym_eig_host: null a or w");
    if (lda < m || (z && ldz < m)) return fail(CVR_ERR_INVALID, "cvr_sym_eig_host: lda = %d, ldz = %d: must be at least m = %d", lda, ldz, m);
    for (int j = 0; j < m; j++)
        for (int i = j; i < m; i++)
            if (!std::isfinite(a[(size_t)j * lda + i])) return fail(CVR_ERR_INVALID, "cvr_sym_eig_host: a(%d, %d) is not finite", i, j);
    if (sym_eig(m, a, lda, w, z, ldz)) return fail(CVR_ERR_INTERNAL, "cvr_sym_eig_host: no convergence");
    return CVR_OK;
}

}  // extern "C"
