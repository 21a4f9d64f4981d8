// cvr_spgemm_host.cpp -- the host twin of the sparse matrix-matrix product (include/cvr_amd.h: cvr_spgemm_host) and the checks it shares with
// cvr_spgemm_create (cvr_spgemm.hip).  One pass over A's rows with a dense marker array of B's ncols entries: O(products) and a sort of each row's
// columns.  C(i, j) = +0 + a[p] * b[q] + .. in ascending p, the product and the sum each rounded once in the matrix's type (this file is compiled
// without contraction), which is what the device kernels compute slot by slot.  No HIP: it links into a stand-alone host program.
#include "cvr_spgemm.h"

#include <algorithm>
#include <new>
#include <vector>

namespace cvrh {
namespace spgemm {

int check_pair(const cvr_csr_view *a, const cvr_csr_view *b, const char *entry)
{
    if (a->nrows < 0 || a->ncols < 0 || b->nrows < 0 || b->ncols < 0) return fail(CVR_ERR_INVALID, "null or negative-size CSR view");
    if ((a->is_f32 != 0) != (b->is_f32 != 0)) return fail(CVR_ERR_INVALID, "%s: A and B differ in is_f32 (%d and %d)", entry, a->is_f32, b->is_f32);
    if (a->ncols != b->nrows) return fail(CVR_ERR_INVALID, "%s: the inner dimensions differ: A is %lld x %lld, B is %lld x %lld", entry, (long long)a->nrows, (long long)a->ncols, (long long)b->nrows, (long long)b->ncols);
    if (b->ncols >= (int64_t)0x7fffffff) return fail(CVR_ERR_INVALID, "%s: B's ncols (%lld) must stay below 2^31 - 1", entry, (long long)b->ncols);
    return CVR_OK;
}

int check_view(const cvr_csr_view *c)
{
    if (c->nrows < 0 || c->ncols < 0) return fail(CVR_ERR_INVALID, "null or negative-size CSR view");
    if (c->nrows > 0 && !c->row_ptr) return fail(CVR_ERR_INVALID, "row_ptr is null");
    if (c->ncols >= (int64_t)0x7fffffff) return fail(CVR_ERR_INVALID, "ncols (%lld) must stay below 2^31 - 1", (long long)c->ncols);
    if (c->nrows == 0) return CVR_OK;
    if (c->row_ptr[0] < 0) return fail(CVR_ERR_INVALID, "row_ptr[0] < 0");
    for (int64_t r = 0; r < c->nrows; r++)
        if (c->row_ptr[r + 1] < c->row_ptr[r]) return fail(CVR_ERR_INVALID, "row_ptr decreases at row %lld", (long long)r);
    const int64_t j0 = c->row_ptr[0], j1 = c->row_ptr[c->nrows];
    if (j1 > 0 && (!c->col_idx || !c->vals)) return fail(CVR_ERR_INVALID, "col_idx / vals is null");
    for (int64_t j = j0; j < j1; j++)
        if (c->col_idx[j] < 0 || c->col_idx[j] >= c->ncols) return fail(CVR_ERR_INVALID, "col_idx[%lld] = %d outside [0, %lld)", (long long)j, c->col_idx[j], (long long)c->ncols);
    return CVR_OK;
}

int64_t first_unsorted_row(int64_t nrows, const int64_t *rp, const int32_t *ci)
{
    for (int64_t r = 0; r < nrows; r++)
        for (int64_t q = rp[r] + 1; q < rp[r + 1]; q++)
            if (ci[q] <= ci[q - 1]) return r;
    return -1;
}

int fail_unsorted(const char *entry, int64_t row)
{
    return fail(CVR_ERR_INVALID, "%s: B row %lld: the columns are not strictly increasing", entry, (long long)row);
}

namespace {

template <typename T>
void product(const cvr_csr_view *a, const cvr_csr_view *b, int64_t *crp, int32_t *cci, T *cva)
{
    const T *av = static_cast<const T *>(a->vals), *bv = static_cast<const T *>(b->vals);
    std::vector<int64_t> mark((size_t)b->ncols, -1);
    std::vector<T>       acc(cci ? (size_t)b->ncols : 0, T(0));
    std::vector<int32_t> touched;
    int64_t              at = 0;
    crp[0] = 0;
    for (int64_t i = 0; i < a->nrows; i++) {
        touched.clear();
        for (int64_t p = a->row_ptr[i]; p < a->row_ptr[i + 1]; p++) {
            const int64_t k = a->col_idx[p];
            for (int64_t q = b->row_ptr[k]; q < b->row_ptr[k + 1]; q++) {
                const int32_t j = b->col_idx[q];
                if (mark[(size_t)j] != i) {
                    mark[(size_t)j] = i;
                    touched.push_back(j);
                    if (cci) acc[(size_t)j] = T(0);
                }
                if (cci) {
                    const T t = av[p] * bv[q];
                    acc[(size_t)j] = acc[(size_t)j] + t;
                }
            }
        }
        if (cci) {
            std::sort(touched.begin(), touched.end());
            for (size_t t = 0; t < touched.size(); t++) {
                cci[at + (int64_t)t] = touched[t];
                cva[at + (int64_t)t] = acc[(size_t)touched[t]];
            }
        }
        at += (int64_t)touched.size();
        crp[i + 1] = at;
    }
}

}  // namespace
}  // namespace spgemm
}  // namespace cvrh

using namespace cvrh;

extern "C" int cvr_spgemm_host(const cvr_csr_view *a, const cvr_csr_view *b, int64_t *c_row_ptr, int32_t *c_col_idx, void *c_vals, int64_t *bad_row)
{
    if (bad_row) *bad_row = -1;
    if (!a || !b || !c_row_ptr || !bad_row) return fail(CVR_ERR_INVALID, "null argument");
    if ((c_col_idx == nullptr) != (c_vals == nullptr)) return fail(CVR_ERR_INVALID, "cvr_spgemm_host: c_col_idx and c_vals go together (both NULL: row_ptr only)");
    if (a->arrays_on_device || b->arrays_on_device) return fail(CVR_ERR_INVALID, "cvr_spgemm_host: the arrays must be host arrays");
    if (const int rc = spgemm::check_pair(a, b, "cvr_spgemm_host")) return rc;
    if (const int rc = spgemm::check_view(a)) return rc;
    if (const int rc = spgemm::check_view(b)) return rc;
    const int64_t bad = spgemm::first_unsorted_row(b->nrows, b->row_ptr, b->col_idx);
    if (bad >= 0) {
        *bad_row = bad;
        return spgemm::fail_unsorted("cvr_spgemm_host", bad);
    }
    try {
        if (a->is_f32) spgemm::product<float>(a, b, c_row_ptr, c_col_idx, static_cast<float *>(c_vals));
        else spgemm::product<double>(a, b, c_row_ptr, c_col_idx, static_cast<double *>(c_vals));
    } catch (const std::bad_alloc &) {
        return fail(CVR_ERR_NOMEM, "cvr_spgemm_host: out of host memory for the marker array (%lld columns)", (long long)b->ncols);
    }
    return CVR_OK;
}
