// cvr_amg_mis2_host.cpp -- the host half of the MIS(2) aggregation (include/cvr_amd.h: cvr_amg_mis2_aggregate_host, cvr_amg_mis2_setup_host and
// the info of such a hierarchy): the strong neighbours, the rounds of the distance-2 maximal independent set on hashed keys, the numbering of
// the roots and the two join passes, every step a loop over the rows that reads the state before it only -- what the kernels of
// cvr_amg_mis2.hip do with a thread per row.  The set-up around it is cvr_amg_host.cpp's with cvr_amg_smoothed_host.cpp's coarsening step.
// No HIP: with those two files and cvr_spgemm_host.cpp it links into a stand-alone host program.
#include "cvr_amg.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

namespace cvrh {
namespace amg {

namespace {

template <typename T>
int64_t aggregate_t(int64_t n, const int64_t *rp, const int32_t *ci, const T *va, double strength, int32_t *agg, int32_t *rounds)
{
    *rounds = 0;
    if (n == 0) return 0;
    const double        s2 = strength * strength;
    const int64_t       j0 = rp[0], nnz = rp[n] - j0;
    std::vector<double> diag((size_t)n, 0.0);
    for (int64_t i = 0; i < n; i++)
        for (int64_t q = rp[i]; q < rp[i + 1]; q++)
            if (ci[q] == i) diag[(size_t)i] = (double)va[q];
    std::vector<uint8_t> strong((size_t)nnz, 0);          // the flags of the strong entries, taken once
    for (int64_t i = 0; i < n; i++)
        for (int64_t q = rp[i]; q < rp[i + 1]; q++) {
            const int64_t j = ci[q];
            const double  a = (double)va[q];
            strong[(size_t)(q - j0)] = j != i && a != 0 && a * a >= (s2 * diag[(size_t)i]) * diag[(size_t)j];
        }
    std::vector<uint8_t>  state((size_t)n, (uint8_t)kMis2Undecided);
    std::vector<uint64_t> m1((size_t)n, 0);
    int64_t               undecided = n;
    while (undecided > 0) {
        ++*rounds;
        for (int64_t i = 0; i < n; i++) {
            uint64_t m = mis2_key(state[(size_t)i], (uint32_t)i);
            for (int64_t q = rp[i]; q < rp[i + 1]; q++)
                if (strong[(size_t)(q - j0)]) m = std::max(m, mis2_key(state[(size_t)ci[q]], (uint32_t)ci[q]));
            m1[(size_t)i] = m;
        }
        undecided = 0;
        for (int64_t i = 0; i < n; i++) {          // (reads m1 and row i's own state only: the states change in place)
            if (state[(size_t)i] != kMis2Undecided) continue;
            uint64_t m = m1[(size_t)i];
            for (int64_t q = rp[i]; q < rp[i + 1]; q++)
                if (strong[(size_t)(q - j0)]) m = std::max(m, m1[(size_t)ci[q]]);
            if (m == mis2_key(kMis2Undecided, (uint32_t)i)) state[(size_t)i] = (uint8_t)kMis2Root;
            else if ((m >> 62) == kMis2Root) state[(size_t)i] = (uint8_t)kMis2Out;
            else undecided++;
        }
    }
    std::vector<int32_t> one((size_t)n, -1);
    int64_t              nc = 0;
    for (int64_t i = 0; i < n; i++)
        if (state[(size_t)i] == kMis2Root) one[(size_t)i] = (int32_t)nc++;
    // the strong neighbour with the largest |a_ij| among those that `from` has assigned; ties: the lowest j stays
    auto join = [&](int64_t i, const std::vector<int32_t> &from) {
        double  best = -1;
        int32_t to = -1;
        for (int64_t q = rp[i]; q < rp[i + 1]; q++) {
            if (!strong[(size_t)(q - j0)]) continue;
            const int32_t aj = from[(size_t)ci[q]];
            const double  m = std::fabs((double)va[q]);
            if (aj >= 0 && m > best) {
                best = m;
                to = aj;
            }
        }
        return to;
    };
    std::vector<int32_t> roots(one);          // pass 1 reads the roots only
    for (int64_t i = 0; i < n; i++)
        if (roots[(size_t)i] < 0) one[(size_t)i] = join(i, roots);
    for (int64_t i = 0; i < n; i++) agg[i] = one[(size_t)i] >= 0 ? one[(size_t)i] : join(i, one);          // pass 2 reads pass 1's result only
    return nc;
}

}  // namespace

int64_t mis2_aggregate(int64_t n, const int64_t *rp, const int32_t *ci, const void *va, int is_f32, double strength, int32_t *agg, int32_t *rounds)
{
    return is_f32 ? aggregate_t<float>(n, rp, ci, static_cast<const float *>(va), strength, agg, rounds)
                  : aggregate_t<double>(n, rp, ci, static_cast<const double *>(va), strength, agg, rounds);
}

void fill_mis2_info(const Hierarchy &H, cvr_amg_mis2_info *info)
{
    memset(info, 0, sizeof(*info));
    if (!H.mis2) return;
    info->mis2 = 1;
    for (size_t l = 0; l + 1 < H.lv.size(); l++) info->rounds[l] = H.rounds[l];
}

}  // namespace amg
}  // namespace cvrh

using namespace cvrh;

extern "C" {

int cvr_amg_mis2_aggregate_host(const cvr_csr_view *csr, double strength, int32_t *agg, int64_t *nc, int32_t *rounds)
{
    const char *entry = "cvr_amg_mis2_aggregate_host";
    if (!csr || !nc || !rounds) return fail(CVR_ERR_INVALID, "null argument");
    *nc = 0;
    *rounds = 0;
    if (!(strength >= 0 && strength < 1)) return fail(CVR_ERR_INVALID, "%s: strength = %g: must be 0 <= strength < 1", entry, strength);
    if (csr->arrays_on_device) return fail(CVR_ERR_INVALID, "%s: the arrays must be host arrays", entry);
    if (csr->nrows != csr->ncols) return fail(CVR_ERR_INVALID, "AMG needs a square matrix (%lld x %lld)", (long long)csr->nrows, (long long)csr->ncols);
    if (const int rc = check_csr(csr, true)) return rc;
    if (csr->nrows >= (int64_t)0x7fffffff) return fail(CVR_ERR_INVALID, "%s: nrows (%lld) must stay below 2^31 - 1", entry, (long long)csr->nrows);
    if (csr->nrows > 0 && !agg) return fail(CVR_ERR_INVALID, "null argument");
    if (const int rc = amg::check_structure(csr->nrows, csr->row_ptr, csr->col_idx, entry)) return rc;
    try {
        *nc = amg::mis2_aggregate(csr->nrows, csr->row_ptr, csr->col_idx, csr->vals, csr->is_f32, strength, agg, rounds);
    } catch (const std::bad_alloc &) {
        return fail(CVR_ERR_NOMEM, "%s: out of host memory (%lld rows)", entry, (long long)csr->nrows);
    }
    return CVR_OK;
}

int cvr_amg_mis2_setup_host(cvr_amg_hierarchy **out, const cvr_csr_view *csr, const cvr_amg_options *opt, double omega, int32_t *bad_level, int64_t *bad_row)
{
    const char *entry = "cvr_amg_mis2_setup_host";
    if (!out || !csr || !bad_level || !bad_row) return fail(CVR_ERR_INVALID, "null argument");
    *out = nullptr;
    *bad_level = -1;
    *bad_row = -1;
    cvr_amg_options o;
    cvr_amg_default_options(&o);
    if (opt) o = *opt;
    if (const int rc = amg::check_options(&o, entry)) return rc;
    double used = 0;
    if (const int rc = amg::check_omega(omega, &used, entry)) return rc;
    if (csr->arrays_on_device) return fail(CVR_ERR_INVALID, "%s: the arrays must be host arrays", entry);
    if (csr->nrows != csr->ncols) return fail(CVR_ERR_INVALID, "AMG needs a square matrix (%lld x %lld)", (long long)csr->nrows, (long long)csr->ncols);
    if (const int rc = check_csr(csr, true)) return rc;
    if (csr->nrows >= (int64_t)0x7fffffff) return fail(CVR_ERR_INVALID, "%s: nrows (%lld) must stay below 2^31 - 1", entry, (long long)csr->nrows);
    if (const int rc = amg::check_structure(csr->nrows, csr->row_ptr, csr->col_idx, entry)) return rc;
    cvr_amg_hierarchy *h = new (std::nothrow) cvr_amg_hierarchy;
    if (!h) return fail(CVR_ERR_NOMEM, "out of host memory");
    const int          is_f32 = csr->is_f32 ? 1 : 0;
    const amg::Coarsen coarsen = [&](amg::Level &f, amg::Level &c, int32_t) { return amg::smoothed_coarsen_host(f, c, is_f32, used); };
    if (const int rc = amg::setup(h->H, csr->nrows, csr->row_ptr, csr->col_idx, csr->vals, is_f32, &o, entry, bad_level, bad_row, &coarsen, amg::Aggregation::kMis2)) {
        delete h;
        return rc;
    }
    h->H.smoothed = 1;
    h->H.omega = used;
    *out = h;
    return CVR_OK;
}

int cvr_amg_hierarchy_mis2_info(const cvr_amg_hierarchy *h, cvr_amg_mis2_info *info)
{
    if (!h || !info) return fail(CVR_ERR_INVALID, "null argument");
    amg::fill_mis2_info(h->H, info);
    return CVR_OK;
}

}  // extern "C"
