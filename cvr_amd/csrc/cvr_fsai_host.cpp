// cvr_fsai_host.cpp -- the host half of the FSAI preconditioner (include/cvr_amd.h: cvr_fsai_factor_host): the structure checks and the row patterns
// the device set-up uses as well (cvr_fsai.hip), and the factorisation itself in host code, row after row, with the arithmetic of the kernel --
// the small matrix gathered by binary search, the right-looking LDL^T, the back substitution by columns, every fp64 operation rounded on its own
// (this file is compiled without contraction), one rounding to T at the end.  No HIP: it links into a stand-alone host program.
#include "cvr_fsai.h"

#include <new>
#include <vector>

namespace cvrh {
namespace fsai {

int pattern(int64_t n, const int64_t *rp, const int32_t *ci, const char *entry, int64_t *wrp, int64_t *src, Pattern *out)
{
    Pattern p;
    wrp[0] = 0;
    for (int64_t i = 0; i < n; i++) {
        int64_t d = -1, prev = -1;
        for (int64_t q = rp[i]; q < rp[i + 1]; q++) {
            const int64_t c = ci[q];
            if (c <= prev) return fail(CVR_ERR_INVALID, "%s: row %lld: the columns are not strictly increasing (%lld behind %lld)", entry, (long long)i, (long long)c, (long long)prev);
            prev = c;
            if (c == i) d = q;
        }
        if (d < 0) return fail(CVR_ERR_INVALID, "%s: row %lld has no diagonal entry", entry, (long long)i);
        int64_t m = d - rp[i] + 1;
        if (m > kMaxRow) {
            m = kMaxRow;
            p.truncated++;
        }
        if (m > p.max_row) p.max_row = (int32_t)m;
        src[i] = d - m + 1;
        wrp[i + 1] = wrp[i] + m;
    }
    p.nnz = wrp[n];
    *out = p;
    return CVR_OK;
}

namespace {

// entry (r, c) of A as a double, +0 when row r has no column c
template <typename T>
inline double entry_of(const int64_t *rp, const int32_t *ci, const T *va, int64_t r, int32_t c)
{
    int64_t lo = rp[r], hi = rp[r + 1];
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ci[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo < rp[r + 1] && ci[lo] == c ? (double)va[lo] : 0.0;
}

// one row: false when a pivot is not finite or not > 0
template <typename T>
bool factor_row(const int64_t *rp, const int32_t *ci, const T *va, int64_t s0, int m, double *S, double *w, T *wa, T *wb)
{
    const int32_t *p = ci + s0;
    for (int a = 0; a < m; a++)
        for (int b = 0; b <= a; b++) S[a * kLd + b] = entry_of(rp, ci, va, p[a], p[b]);
    // l_ak goes to the mirrored position (k, a); s_a = S[a][k] stays where it is
    for (int k = 0; k < m; k++) {
        const double d = S[k * kLd + k];
        if (!pivot_ok(d)) return false;
        for (int a = k + 1; a < m; a++) S[k * kLd + a] = S[a * kLd + k] / d;
        for (int a = k + 1; a < m; a++) {
            const double lak = S[k * kLd + a];
            for (int b = k + 1; b <= a; b++) S[a * kLd + b] = S[a * kLd + b] - lak * S[b * kLd + k];
        }
    }
    const double dl = S[(m - 1) * kLd + (m - 1)];
    for (int a = 0; a < m; a++) w[a] = a == m - 1 ? 1.0 : 0.0;
    for (int b = m - 1; b >= 1; b--)
        for (int a = 0; a < b; a++) w[a] = w[a] - S[a * kLd + b] * w[b];
    for (int a = 0; a < m; a++) {
        wa[a] = (T)w[a];
        wb[a] = (T)(w[a] / dl);
    }
    return true;
}

template <typename T>
int64_t factor_all(int64_t n, const int64_t *rp, const int32_t *ci, const T *va, const int64_t *wrp, const int64_t *src, T *wa, T *wb)
{
    std::vector<double> S((size_t)kMaxRow * kLd), w((size_t)kMaxRow);
    for (int64_t i = 0; i < n; i++)
        if (!factor_row<T>(rp, ci, va, src[i], (int)(wrp[i + 1] - wrp[i]), S.data(), w.data(), wa + wrp[i], wb + wrp[i])) return i;
    return -1;
}

}  // namespace
}  // namespace fsai
}  // namespace cvrh

using namespace cvrh;

extern "C" int cvr_fsai_factor_host(const cvr_csr_view *csr, int64_t *row_ptr, int32_t *col_idx, void *wa, void *wb, int64_t *bad_row)
{
    if (!csr || !row_ptr || !bad_row) return fail(CVR_ERR_INVALID, "null argument");
    if (csr->arrays_on_device) return fail(CVR_ERR_INVALID, "cvr_fsai_factor_host: the arrays must be host arrays");
    if (csr->nrows != csr->ncols) return fail(CVR_ERR_INVALID, "FSAI needs a square matrix (%lld x %lld)", (long long)csr->nrows, (long long)csr->ncols);
    if (const int rc = check_csr(csr, true)) return rc;
    const int64_t n = csr->nrows;
    *bad_row = -1;
    row_ptr[0] = 0;
    if (n == 0) return CVR_OK;
    if (!col_idx || !wa || !wb) return fail(CVR_ERR_INVALID, "null argument");
    try {
        std::vector<int64_t> src((size_t)n);
        fsai::Pattern        pat;
        if (const int rc = fsai::pattern(n, csr->row_ptr, csr->col_idx, "cvr_fsai_factor_host", row_ptr, src.data(), &pat)) return rc;
        for (int64_t i = 0; i < n; i++)
            for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; e++) col_idx[e] = csr->col_idx[src[(size_t)i] + (e - row_ptr[i])];
        *bad_row = csr->is_f32 ? fsai::factor_all<float>(n, csr->row_ptr, csr->col_idx, static_cast<const float *>(csr->vals), row_ptr, src.data(), static_cast<float *>(wa), static_cast<float *>(wb))
                               : fsai::factor_all<double>(n, csr->row_ptr, csr->col_idx, static_cast<const double *>(csr->vals), row_ptr, src.data(), static_cast<double *>(wa), static_cast<double *>(wb));
    } catch (const std::bad_alloc &) {
        return fail(CVR_ERR_NOMEM, "cvr_fsai_factor_host: out of host memory (%lld rows)", (long long)n);
    }
    if (*bad_row >= 0) return fail(CVR_ERR_STATE, "cvr_fsai_factor_host: the pivot of row %lld is not finite or not > 0", (long long)*bad_row);
    return CVR_OK;
}
