// cvr_lobpcg.hip -- a block of 1 to 8 extreme eigenpairs of a symmetric A on the device, with an optional preconditioner object of any kind
// (include/cvr_amd.h: cvr_lobpcg_device, cvr_lobpcg): LOBPCG of Knyazev (SIAM J. Sci. Comput. 23, 2001) on cvr_krylov.h's plan.  The basis of an
// iteration is S = [X W P], k columns each, with A S = [AX AW AP] beside it; both exist twice, and the combination of an iteration writes the set the
// next one reads (no kernel reads a column another workgroup of the same launch may be writing).  Per iteration, beside the k products A W
// (run_spmv: cvr_spmv_device's path) and the k applies of the object (p->ops->apply: cvr_precond_apply_device's path):
//   lobpcg_residual_kernel   R_c = AX_c - theta_c X_c and the partial sums of R_c . R_c, all columns in one launch
//   lobpcg_dots_kernel       the partial sums of the k x k products X_i . W_c
//   lobpcg_update_kernel     the coefficients from those partials, summed in every workgroup; W_c -= sum_i h_ic X_i; the partial sums of W_c . W_c
//   (the two once more: two passes), lobpcg_scale_kernel: W_c /= ||W_c||
//   lobpcg_gram_kernel       the lower triangles of G = S^T S and H = S^T (A S): a workgroup row (blockIdx.y) per 8 x 8 block, k x k accumulators a thread
//   lobpcg_reduce_kernel     sum_partials' tree of every entry's partials, one workgroup per entry
// then the one read-back of the iteration (G, H, the residual norms, the norms of W), the Rayleigh-Ritz step on the host (Cholesky of G, the library's
// cvr_sym_eig_host of L^-1 H L^-T: rayleigh_ritz below) and
//   lobpcg_combine_kernel    X' = S C, AX' = (A S) C, P' = S C~, AP' = (A S) C~ with C in LDS, and the partial sums of P'_c . P'_c
//   lobpcg_scale_kernel      P'_c and AP'_c divided by ||P'_c||
// The caller's X is read once at the start and written once at the end, by device copies, and not at all behind a breakdown.
// (The reference has no solver: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_precond.h"
#include "cvr_lobpcg_kernels.h"

namespace cvrh {
int sym_eig(int m, const double *a, int lda, double *w, double *z, int ldz);          // cvr_symeig.cpp
}

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

constexpr double kEps23 = CVR_EIG_EPS23;
constexpr int    kRn = 0, kGram = kLobMaxK, kWn = kGram + kLobGramSets, kPn = kWn + kLobMaxK, kRedCount = kPn + kLobMaxK;          // the read-back, in doubles

// what comes before any device work and before the handle is looked at, in the header's order
int check_args(const void *h, const cvr_precond *p, const void *X, int64_t ldx, const double *evals, const double *resnorms, const cvr_lobpcg_options *opt,
               const cvr_lobpcg_result *res)
{
    if (!h) return fail(CVR_ERR_INVALID, "cvr_lobpcg: null h");
    if (!X) return fail(CVR_ERR_INVALID, "cvr_lobpcg: null X");
    if (!evals) return fail(CVR_ERR_INVALID, "cvr_lobpcg: null evals");
    if (!resnorms) return fail(CVR_ERR_INVALID, "cvr_lobpcg: null resnorms");
    if (!opt) return fail(CVR_ERR_INVALID, "cvr_lobpcg: null opt");
    if (!res) return fail(CVR_ERR_INVALID, "cvr_lobpcg: null res");
    if (opt->nev < 1 || opt->nev > CVR_LOBPCG_MAX_BLOCK) return fail(CVR_ERR_INVALID, "cvr_lobpcg: nev = %d: must be in 1 .. %d", opt->nev, CVR_LOBPCG_MAX_BLOCK);
    if (opt->which != CVR_EIG_LARGEST && opt->which != CVR_EIG_SMALLEST) return fail(CVR_ERR_INVALID, "cvr_lobpcg: which = %d: must be CVR_EIG_LARGEST or CVR_EIG_SMALLEST", opt->which);
    if (opt->max_iters < 0) return fail(CVR_ERR_INVALID, "cvr_lobpcg: max_iters = %d: must not be negative", opt->max_iters);
    if (!(opt->tol >= 0) || !std::isfinite(opt->tol)) return fail(CVR_ERR_INVALID, "cvr_lobpcg: tol = %g: must be finite and not negative", opt->tol);
    if (opt->reserved0 != 0) return fail(CVR_ERR_INVALID, "cvr_lobpcg_options.reserved0 = %d: must be 0", opt->reserved0);
    for (int i = 0; i < 4; i++)
        if (opt->reserved[i] != 0) return fail(CVR_ERR_INVALID, "cvr_lobpcg_options.reserved[%d] = %d: must be 0", i, opt->reserved[i]);
    if (ldx < 1) return fail(CVR_ERR_INVALID, "cvr_lobpcg: ldx = %lld: must be at least 1", (long long)ldx);
    if (p && opt->which == CVR_EIG_LARGEST)
        return fail(CVR_ERR_INVALID, "cvr_lobpcg: a preconditioner with CVR_EIG_LARGEST: it approximates the inverse of A and serves the lower end only");
    return CVR_OK;
}

// ... and what follows on the handle
int check_handle(const cvr_handle *h, const cvr_precond *p, int64_t ldx, const cvr_lobpcg_options *opt)
{
    if (const int rc = check_square_preprocessed(h, "cvr_lobpcg", "the eigensolver needs")) return rc;
    const int64_t n = h->info.nrows;
    if (n < 3 * (int64_t)opt->nev) return fail(CVR_ERR_INVALID, "cvr_lobpcg: n = %lld is below 3 * nev = %lld", (long long)n, 3 * (long long)opt->nev);
    if (ldx < n) return fail(CVR_ERR_INVALID, "cvr_lobpcg: ldx = %lld is below n = %lld", (long long)ldx, (long long)n);
    if (p)
        if (const int rc = check_precond_pair(h, p, "cvr_lobpcg")) return rc;
    return CVR_OK;
}

// The Rayleigh-Ritz step of m columns on the host, plain fp64 in a fixed order.  G and H: the lower triangles, element (i, j) with i >= j at
// [i * kLobMaxM + j].  Cholesky G = L L^T column by column; a pivot that is not finite, not > 0 or not > tau * G_jj: returns 1.  Then Y = L^-1 H (forward substitution,
// column by column of the symmetric H), the lower triangle of M = Y L^-T row by row, its eigenpairs by sym_eig, and for the k wanted ones (ascending; the
// upper end with `largest`) c = L^-T z by back substitution: theta[c] and C[l * kLobMaxK + c].  An M that is not finite: returns 2; sym_eig's failure: 3.
int rayleigh_ritz(int m, const double *G, const double *H, int k, bool largest, double tau, double *theta, double *C)
{
    constexpr int ld = kLobMaxM;
    double        L[ld * ld], Y[ld * ld], M[ld * ld], w[ld], Z[ld * ld];
    for (int j = 0; j < m; j++) {
        double s = G[j * ld + j];
        for (int p = 0; p < j; p++) s = s - L[j * ld + p] * L[j * ld + p];
        if (!(s > tau * G[j * ld + j]) || !(s > 0) || !std::isfinite(s)) return 1;
        const double d = std::sqrt(s);
        L[j * ld + j] = d;
        for (int i = j + 1; i < m; i++) {
            double t = G[i * ld + j];
            for (int p = 0; p < j; p++) t = t - L[i * ld + p] * L[j * ld + p];
            L[i * ld + j] = t / d;
        }
    }
    for (int j = 0; j < m; j++)
        for (int i = 0; i < m; i++) {
            double t = i >= j ? H[i * ld + j] : H[j * ld + i];
            for (int p = 0; p < i; p++) t = t - L[i * ld + p] * Y[p * ld + j];
            Y[i * ld + j] = t / L[i * ld + i];
        }
    for (int i = 0; i < m; i++)
        for (int j = 0; j <= i; j++) {
            double t = Y[i * ld + j];
            for (int p = 0; p < j; p++) t = t - M[i * ld + p] * L[j * ld + p];
            M[i * ld + j] = t / L[j * ld + j];
            if (!std::isfinite(M[i * ld + j])) return 2;
        }
    // sym_eig reads element (i, j), i >= j, at a[i + j * lda]: M transposed in place of a copy
    double a[ld * ld];
    for (int i = 0; i < m; i++)
        for (int j = 0; j <= i; j++) a[i + j * ld] = M[i * ld + j];
    if (sym_eig(m, a, ld, w, Z, ld)) return 3;
    const int lo = largest ? m - k : 0;
    std::fill(C, C + (size_t)kLobMaxM * kLobMaxK, 0.0);
    for (int c = 0; c < k; c++) {
        const double *z = Z + (size_t)(lo + c) * ld;
        double        x[ld];
        for (int i = m - 1; i >= 0; i--) {
            double t = z[i];
            for (int p = i + 1; p < m; p++) t = t - L[p * ld + i] * x[p];
            x[i] = t / L[i * ld + i];
        }
        theta[c] = w[lo + c];
        for (int l = 0; l < m; l++) C[l * kLobMaxK + c] = x[l];
    }
    return 0;
}

// f(std::integral_constant<int, KB>()) with KB = k rounded up to 1, 2, 4 or 8
template <typename F>
auto with_block(int k, F &&f)
{
    return k <= 1 ? f(std::integral_constant<int, 1>()) : k <= 2 ? f(std::integral_constant<int, 2>()) : k <= 4 ? f(std::integral_constant<int, 4>())
                                                                                                                  : f(std::integral_constant<int, 8>());
}

// G and H of nb blocks (m = nb k columns) out of the read-back
void unpack_gram(const double *red, int KB, int k, int nb, double *G, double *H)
{
    for (int bi = 0, pair = 0; bi < nb; bi++)
        for (int bj = 0; bj <= bi; bj++, pair++)
            for (int isH = 0; isH < 2; isH++) {
                const double *blk = red + kGram + (size_t)(2 * pair + isH) * KB * KB;
                double       *out = isH ? H : G;
                for (int i = 0; i < k; i++)
                    for (int j = 0; j < k; j++)
                        if (bi * k + i >= bj * k + j) out[(bi * k + i) * kLobMaxM + bj * k + j] = blk[i * KB + j];
            }
}

template <typename T>
int lobpcg_solve(cvr_handle *h, const cvr_precond *pc, T *X, int64_t ldx, double *evals, double *resnorms, const cvr_lobpcg_options *opt, cvr_lobpcg_result *res,
                 hipStream_t st)
{
    const long long n = h->info.nrows;
    const size_t    vb = sizeof(T) * (size_t)n;
    const int       k = opt->nev;
    const bool      largest = opt->which == CVR_EIG_LARGEST;

    // a column is an SpMV input (X at the start, W) or an SpMV output (AX at the start, AW): one stride for all of them
    Arena        a;
    const size_t nx = std::max(Arena::slot(x_ext_bytes(h)), Arena::slot(y_ext_bytes(h)));
    size_t       oS[2], oAS[2];
    for (int s = 0; s < 2; s++) {
        oS[s] = a.add((size_t)3 * k * nx);
        oAS[s] = a.add((size_t)3 * k * nx);
    }
    const size_t oR = a.add((size_t)k * nx);
    const size_t opart = a.add(sizeof(double) * (size_t)(kLobMaxK + kLobGramSets) * kBlocks), oh = a.add(sizeof(double) * (size_t)kLobMaxK * kLobMaxK * kBlocks);
    const size_t own = a.add(sizeof(double) * (size_t)kLobMaxK * kBlocks), opn = a.add(sizeof(double) * (size_t)kLobMaxK * kBlocks);
    const size_t ored = a.add(sizeof(double) * kRedCount), oC = a.add(sizeof(double) * kLobMaxM * kLobMaxK);
    const hipError_t e = a.alloc();
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(CVR_ERR_NOMEM, "cvr_lobpcg: no device memory for %d vectors (%zu bytes)", 13 * k, a.total());
    }
    HIP_TRY(e);
    T              *S[2] = {a.at<T>(oS[0]), a.at<T>(oS[1])}, *AS[2] = {a.at<T>(oAS[0]), a.at<T>(oAS[1])}, *R = a.at<T>(oR);
    double         *part = a.at<double>(opart), *part_h = a.at<double>(oh), *part_wn = a.at<double>(own), *part_pn = a.at<double>(opn);
    double         *red = a.at<double>(ored), *Cdev = a.at<double>(oC);
    const long long stride = (long long)(nx / sizeof(T));
    if (const int rc = a.begin(st)) return rc;

    // every set of partials and the read-back are defined from the start (a block smaller than its compile-time extent leaves sets unwritten); the pad
    // slots of the SpMV inputs; the start block
    HIP_TRY(hipMemsetAsync(part, 0, sizeof(double) * (size_t)(kLobMaxK + kLobGramSets) * kBlocks, st));
    HIP_TRY(hipMemsetAsync(red, 0, sizeof(double) * kRedCount, st));
    for (int s = 0; s < 2; s++)
        for (int c = 0; c < 3 * k; c++)
            if (const int rc = zero_pad_slot(S[s] + c * stride, vb, sizeof(T), st)) return rc;
    for (int c = 0; c < k; c++) HIP_TRY(hipMemcpyAsync(S[0] + c * stride, X + (long long)c * ldx, vb, hipMemcpyDeviceToDevice, st));

    std::vector<double> hred(kRedCount), G((size_t)kLobMaxM * kLobMaxM), H((size_t)kLobMaxM * kLobMaxM), coef((size_t)kLobMaxM * kLobMaxK);
    double              theta[kLobMaxK] = {}, next[kLobMaxK] = {}, rn[kLobMaxK] = {};
    int                 cur = 0, status = CVR_EIG_MAX_ITERS, iterations = 0, nconv = 0, fallbacks = 0, spmvs = 0, applies = 0;
    double              worst = 0;

    // the sums of G and H of nb blocks of set `cur`, summed and read back together with the residual norms in front of them
    auto gram_and_read = [&](int nb, bool with_gram) -> int {
        const int KB = with_block(k, [](auto kb) { return (int)decltype(kb)::value; });
        const int ny = with_gram ? nb * (nb + 1) : 0;
        if (with_gram)
            with_block(k, [&](auto kb) {
                constexpr int KBc = decltype(kb)::value;
                hipLaunchKernelGGL((lobpcg_gram_kernel<T, KBc>), dim3(kBlocks, ny), dim3(kThreads), 0, st, (const T *)S[cur], (const T *)AS[cur], stride, n, k,
                                   part + (size_t)kGram * kBlocks);
                return 0;
            });
        // the gram sets of a block lie KB * KB apart: they begin at set kGram whatever KB is
        hipLaunchKernelGGL(lobpcg_reduce_kernel, dim3(kGram + ny * KB * KB), dim3(kThreads), 0, st, (const double *)part, red);
        HIP_TRY(hipGetLastError());
        return read_cell(hred.data(), red, sizeof(double) * kRedCount, st);
    };
    auto ritz = [&](int nb, double *th) -> int {
        const int KB = with_block(k, [](auto kb) { return (int)decltype(kb)::value; });
        unpack_gram(hred.data(), KB, k, nb, G.data(), H.data());
        return rayleigh_ritz(nb * k, G.data(), H.data(), k, largest, nb < 3 ? 0.0 : sizeof(T) == 4 ? CVR_LOBPCG_PIVOT_F32 : CVR_LOBPCG_PIVOT_F64, th, coef.data());
    };
    auto combine = [&](int m, bool with_p) -> int {
        HIP_TRY(hipMemcpyAsync(Cdev, coef.data(), sizeof(double) * coef.size(), hipMemcpyHostToDevice, st));
        with_block(k, [&](auto kb) {
            constexpr int KBc = decltype(kb)::value;
            if (with_p) launch(lobpcg_combine_kernel<T, KBc, true>, st, (const T *)S[cur], (const T *)AS[cur], stride, n, m, k, (const double *)Cdev, S[cur ^ 1], AS[cur ^ 1], part_pn);
            else launch(lobpcg_combine_kernel<T, KBc, false>, st, (const T *)S[cur], (const T *)AS[cur], stride, n, m, k, (const double *)Cdev, S[cur ^ 1], AS[cur ^ 1], part_pn);
            return 0;
        });
        if (with_p) launch(lobpcg_scale_kernel<T>, st, S[cur ^ 1] + 2 * k * stride, AS[cur ^ 1] + 2 * k * stride, stride, n, k, (const double *)part_pn, red + kPn);
        HIP_TRY(hipGetLastError());
        cur ^= 1;
        return CVR_OK;
    };

    // the start: A X by k products, the Rayleigh-Ritz step on S = [X]
    for (int c = 0; c < k; c++) HIP_TRY(run_spmv(h, S[0] + c * stride, AS[0] + c * stride, st));
    spmvs += k;
    if (const int rc = gram_and_read(1, true)) return rc;
    int rr = ritz(1, theta);
    if (rr == 3) return fail(CVR_ERR_INTERNAL, "cvr_lobpcg: the projected problem of %d columns did not converge", k);
    if (rr) status = CVR_EIG_BREAKDOWN;
    else if (const int rc = combine(k, false)) return rc;

    for (int nb = 2; status != CVR_EIG_BREAKDOWN;) {
        const bool last = iterations == opt->max_iters;
        T         *Xc = S[cur], *Wc = S[cur] + k * stride, *Rc = pc ? R : Wc;
        LobTheta   th;
        for (int c = 0; c < kLobMaxK; c++) th.v[c] = theta[c];
        with_block(k, [&](auto kb) {
            constexpr int KBc = decltype(kb)::value;
            launch(lobpcg_residual_kernel<T, KBc>, st, (const T *)Xc, (const T *)AS[cur], stride, n, k, th, Rc, part);
            return 0;
        });
        if (!last) {
            if (pc) {
                for (int c = 0; c < k; c++)
                    if (const int rc = pc->ops->apply(pc, R + c * stride, Wc + c * stride, st)) return rc;
                applies += k;
            }
            with_block(k, [&](auto kb) {
                constexpr int KBc = decltype(kb)::value;
                for (int pass = 0; pass < 2; pass++) {
                    launch(lobpcg_dots_kernel<T, KBc>, st, (const T *)Xc, (const T *)Wc, stride, n, k, part_h);
                    launch(lobpcg_update_kernel<T, KBc>, st, (const T *)Xc, Wc, stride, n, k, (const double *)part_h, part_wn);
                }
                return 0;
            });
            launch(lobpcg_scale_kernel<T>, st, Wc, (T *)nullptr, stride, n, k, (const double *)part_wn, red + kWn);
            HIP_TRY(hipGetLastError());
            for (int c = 0; c < k; c++) HIP_TRY(run_spmv(h, Wc + c * stride, AS[cur] + (k + c) * stride, st));
            spmvs += k;
        }
        if (const int rc = gram_and_read(nb, !last)) return rc;
        // the residual norms belong to the X of set `cur`: converged, or out of iterations, and that X is the one returned
        bool finite = true;
        nconv = 0;
        worst = 0;
        for (int c = 0; c < k; c++) {
            rn[c] = std::sqrt(hred[kRn + c]);
            finite = finite && std::isfinite(rn[c]) && std::isfinite(theta[c]);
            const double scale = std::max(kEps23, std::fabs(theta[c]));
            if (rn[c] <= opt->tol * scale) nconv++;
            worst = std::max(worst, rn[c] / scale);
        }
        if (!finite) { status = CVR_EIG_BREAKDOWN; break; }
        if (nconv == k) { status = CVR_EIG_CONVERGED; break; }
        if (last) { status = CVR_EIG_MAX_ITERS; break; }
        for (int c = 0; c < k; c++)
            if (!(hred[kWn + c] > 0) || !std::isfinite(hred[kWn + c])) status = CVR_EIG_BREAKDOWN;
        if (status == CVR_EIG_BREAKDOWN) break;
        rr = ritz(nb, next);
        if ((rr == 1 || rr == 2) && nb == 3) {          // P has fallen into the span of X and W: once more without it, on the same sums
            fallbacks++;
            nb = 2;
            rr = ritz(nb, next);
        }
        if (rr == 3) return fail(CVR_ERR_INTERNAL, "cvr_lobpcg: the projected problem of %d columns did not converge", nb * k);
        if (rr) { status = CVR_EIG_BREAKDOWN; break; }
        if (const int rc = combine(nb * k, true)) return rc;
        for (int c = 0; c < k; c++) theta[c] = next[c];
        nb = 3;
        iterations++;
    }
    if (status != CVR_EIG_BREAKDOWN) {
        for (int c = 0; c < k; c++) HIP_TRY(hipMemcpyAsync(X + (long long)c * ldx, S[cur] + c * stride, vb, hipMemcpyDeviceToDevice, st));
        for (int c = 0; c < k; c++) {
            evals[c] = theta[c];
            resnorms[c] = rn[c];
        }
    }
    double seconds = 0;
    if (const int rc = a.seconds(st, &seconds)) return rc;
    memset(res, 0, sizeof(*res));
    res->nconv = status == CVR_EIG_BREAKDOWN ? 0 : nconv;
    res->status = status;
    res->iterations = iterations;
    res->spmv_count = spmvs;
    res->precond_applies = applies;
    res->restarts_without_p = fallbacks;
    res->seconds = seconds;
    res->max_rel_residual = status == CVR_EIG_BREAKDOWN ? 0.0 : worst;
    return CVR_OK;
}

// behind the argument checks
int lobpcg_device(cvr_handle *h, const cvr_precond *p, void *X, int64_t ldx, double *evals, double *resnorms, const cvr_lobpcg_options *opt, cvr_lobpcg_result *res,
                  hipStream_t st)
{
    if (const int rc = check_handle(h, p, ldx, opt)) return rc;
    Range range("cvr_lobpcg_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) { return lobpcg_solve(h, p, static_cast<decltype(t) *>(X), ldx, evals, resnorms, opt, res, st); });
}

}  // namespace

extern "C" {

void cvr_lobpcg_default_options(cvr_lobpcg_options *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->nev = 1;
    opt->which = CVR_EIG_SMALLEST;
    opt->max_iters = 200;
    opt->tol = 1e-8;
}

int cvr_lobpcg_device(cvr_handle *h, const cvr_precond *p, void *X_dev, int64_t ldx, double *evals_host, double *resnorms_host, const cvr_lobpcg_options *opt,
                      cvr_lobpcg_result *res, void *stream)
{
    if (const int rc = check_args(h, p, X_dev, ldx, evals_host, resnorms_host, opt, res)) return rc;
    return lobpcg_device(h, p, X_dev, ldx, evals_host, resnorms_host, opt, res, (hipStream_t)stream);
}

int cvr_lobpcg(cvr_handle *h, const cvr_precond *p, void *X_host, int64_t ldx, double *evals_host, double *resnorms_host, const cvr_lobpcg_options *opt,
               cvr_lobpcg_result *res)
{
    if (const int rc = check_args(h, p, X_host, ldx, evals_host, resnorms_host, opt, res)) return rc;
    if (const int rc = check_handle(h, p, ldx, opt)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    // the block rides in a device array of the call: nev columns of n values, contiguous
    const size_t vb = h->vsz * (size_t)h->info.nrows;
    uint8_t     *block = nullptr;
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&block), std::max<size_t>(vb * (size_t)opt->nev, 16));
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(CVR_ERR_NOMEM, "cvr_lobpcg: no device memory for %d vectors", opt->nev);
    }
    HIP_TRY(e);
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpy2DAsync(block, vb, X_host, h->vsz * (size_t)ldx, vb, (size_t)opt->nev, hipMemcpyHostToDevice, h->stream));
        if (const int rc = lobpcg_device(h, p, block, h->info.nrows, evals_host, resnorms_host, opt, res, h->stream)) return rc;
        if (res->status != CVR_EIG_BREAKDOWN)
            HIP_TRY(hipMemcpy2DAsync(X_host, h->vsz * (size_t)ldx, block, vb, vb, (size_t)opt->nev, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return CVR_OK;
    };
    const int rc = run();
    (void)hipFree(block);
    return rc;
}

}  // extern "C"
