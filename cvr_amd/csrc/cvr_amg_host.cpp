// cvr_amg_host.cpp -- the set-up of the aggregation AMG preconditioner (include/cvr_amd.h: cvr_amg_setup_host, which cvr_precond_amg calls as
// well: cvr_amg.hip), all of it on the host, O(nnz) per level: the smoother diagonal, the strength test, the three passes of the aggregation, the
// Galerkin coarse operator of the piecewise-constant prolongator (a sum of entries by (aggregate, aggregate): no sparse matrix-matrix product), the
// stopping rule and the dense inverse of a small coarsest level.  Every fp64 operation is rounded on its own (this file is compiled without
// contraction), every stored value rounded to T once.  No HIP: it links into a stand-alone host program.
#include "cvr_amg.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

namespace cvrh {
namespace amg {

int check_options(const cvr_amg_options *o, const char *entry)
{
    if (o->max_levels < 1 || o->max_levels > CVR_AMG_MAX_LEVELS) return fail(CVR_ERR_INVALID, "%s: max_levels = %d: must be 1 .. %d", entry, o->max_levels, CVR_AMG_MAX_LEVELS);
    if (o->coarse_size < 1 || o->coarse_size > CVR_AMG_MAX_COARSE) return fail(CVR_ERR_INVALID, "%s: coarse_size = %d: must be 1 .. %d", entry, o->coarse_size, CVR_AMG_MAX_COARSE);
    if (o->sweeps < 1 || o->sweeps > 4) return fail(CVR_ERR_INVALID, "%s: sweeps = %d: must be 1 .. 4", entry, o->sweeps);
    if (o->reserved0 != 0) return fail(CVR_ERR_INVALID, "%s: cvr_amg_options.reserved0 = %d: must be 0", entry, o->reserved0);
    if (!(o->strength >= 0 && o->strength < 1)) return fail(CVR_ERR_INVALID, "%s: strength = %g: must be 0 <= strength < 1", entry, o->strength);
    if (!(o->coarse_scale > 0 && o->coarse_scale <= kDblMax)) return fail(CVR_ERR_INVALID, "%s: coarse_scale = %g: must be finite and > 0", entry, o->coarse_scale);
    for (int i = 0; i < 8; i++)
        if (o->reserved[i] != 0) return fail(CVR_ERR_INVALID, "%s: cvr_amg_options.reserved[%d] = %d: must be 0", entry, i, o->reserved[i]);
    return CVR_OK;
}

int check_structure(int64_t n, const int64_t *rp, const int32_t *ci, const char *entry, int64_t row0)
{
    for (int64_t i = 0; i < n; i++) {
        int64_t d = -1, prev = -1;
        for (int64_t q = rp[i]; q < rp[i + 1]; q++) {
            const int64_t c = ci[q];
            if (c <= prev) return fail(CVR_ERR_INVALID, "%s: row %lld: the columns are not strictly increasing (%lld behind %lld)", entry, (long long)(row0 + i), (long long)c, (long long)prev);
            prev = c;
            if (c == row0 + i) d = q;
        }
        if (d < 0) return fail(CVR_ERR_INVALID, "%s: row %lld has no diagonal entry", entry, (long long)(row0 + i));
    }
    return CVR_OK;
}

namespace {

inline bool positive_finite(double d) { return d > 0 && d <= kDblMax; }

template <typename T>
inline const T *values(const Level &l) { return reinterpret_cast<const T *>(l.va.data()); }

// diag[n] as doubles; the lowest row whose diagonal entry is not finite or not > 0, or -1
template <typename T>
int64_t diagonal(const Level &l, std::vector<double> &diag)
{
    const T *va = values<T>(l);
    diag.assign((size_t)l.n, 0.0);
    int64_t bad = -1;
    for (int64_t i = 0; i < l.n; i++) {
        double d = 0;
        for (int64_t q = l.rp[(size_t)i]; q < l.rp[(size_t)i + 1]; q++)
            if (l.ci[(size_t)q] == i) d = (double)va[q];
        diag[(size_t)i] = d;
        if (bad < 0 && !positive_finite(d)) bad = i;
    }
    return bad;
}

// dinv_i = T(1 / (|a_i0| + |a_i1| + ..)), the sum from +0 in column order
template <typename T>
void smoother_diagonal(Level &l)
{
    const T *va = values<T>(l);
    l.dinv.assign(sizeof(T) * (size_t)l.n, 0);
    T *dinv = reinterpret_cast<T *>(l.dinv.data());
    for (int64_t i = 0; i < l.n; i++) {
        double s = 0;
        for (int64_t q = l.rp[(size_t)i]; q < l.rp[(size_t)i + 1]; q++) s = s + std::fabs((double)va[q]);
        dinv[i] = (T)(1.0 / s);
    }
}

// the three passes; agg[n], returns the number of aggregates
template <typename T>
int64_t aggregate(const Level &l, const std::vector<double> &diag, double strength, std::vector<int32_t> &agg)
{
    const T      *va = values<T>(l);
    const int64_t n = l.n;
    const double  s2 = strength * strength;
    auto strong = [&](int64_t i, int64_t q) {
        const int64_t j = l.ci[(size_t)q];
        const double  a = (double)va[q];
        return j != i && a != 0 && a * a >= (s2 * diag[(size_t)i]) * diag[(size_t)j];
    };
    agg.assign((size_t)n, -1);
    int64_t nc = 0;
    for (int64_t i = 0; i < n; i++) {          // pass 1: i and all its strong neighbours free
        if (agg[(size_t)i] >= 0) continue;
        bool all_free = true;
        for (int64_t q = l.rp[(size_t)i]; q < l.rp[(size_t)i + 1] && all_free; q++)
            if (strong(i, q) && agg[(size_t)l.ci[(size_t)q]] >= 0) all_free = false;
        if (!all_free) continue;
        agg[(size_t)i] = (int32_t)nc;
        for (int64_t q = l.rp[(size_t)i]; q < l.rp[(size_t)i + 1]; q++)
            if (strong(i, q)) agg[(size_t)l.ci[(size_t)q]] = (int32_t)nc;
        nc++;
    }
    std::vector<int32_t> join((size_t)n, -1);          // pass 2 reads pass-1 membership only: its own choices go in behind it
    for (int64_t i = 0; i < n; i++) {
        if (agg[(size_t)i] >= 0) continue;
        double best = -1;
        for (int64_t q = l.rp[(size_t)i]; q < l.rp[(size_t)i + 1]; q++) {
            if (!strong(i, q)) continue;
            const int32_t aj = agg[(size_t)l.ci[(size_t)q]];
            const double  m = std::fabs((double)va[q]);
            if (aj >= 0 && m > best) {          // (ties: the lowest j stays)
                best = m;
                join[(size_t)i] = aj;
            }
        }
    }
    for (int64_t i = 0; i < n; i++)
        if (agg[(size_t)i] < 0) agg[(size_t)i] = join[(size_t)i];
    for (int64_t i = 0; i < n; i++) {          // pass 3: i with its still-free strong neighbours
        if (agg[(size_t)i] >= 0) continue;
        agg[(size_t)i] = (int32_t)nc;
        for (int64_t q = l.rp[(size_t)i]; q < l.rp[(size_t)i + 1]; q++)
            if (strong(i, q) && agg[(size_t)l.ci[(size_t)q]] < 0) agg[(size_t)l.ci[(size_t)q]] = (int32_t)nc;
        nc++;
    }
    return nc;
}

void members(Level &l)
{
    l.mrp.assign((size_t)l.nc + 1, 0);
    l.mem.assign((size_t)l.n, 0);
    for (int64_t i = 0; i < l.n; i++) l.mrp[(size_t)l.agg[(size_t)i] + 1]++;
    for (int64_t I = 0; I < l.nc; I++) l.mrp[(size_t)I + 1] += l.mrp[(size_t)I];
    std::vector<int64_t> at(l.mrp.begin(), l.mrp.end() - 1);
    for (int64_t i = 0; i < l.n; i++) l.mem[(size_t)at[(size_t)l.agg[(size_t)i]]++] = (int32_t)i;
}

// A_c(I, J) = +0 + a_ij + .. over the rows of I ascending, each row's entries in column order; rounded to T once; rows sorted
template <typename T>
void coarse_operator(const Level &f, Level &c)
{
    const T      *va = values<T>(f);
    const int64_t nc = f.nc;
    c.n = nc;
    c.rp.assign((size_t)nc + 1, 0);
    c.ci.clear();
    std::vector<T>       cv;
    std::vector<double>  acc((size_t)nc, 0.0);
    std::vector<int64_t> mark((size_t)nc, -1);
    std::vector<int32_t> touched;
    for (int64_t I = 0; I < nc; I++) {
        touched.clear();
        for (int64_t m = f.mrp[(size_t)I]; m < f.mrp[(size_t)I + 1]; m++) {
            const int64_t i = f.mem[(size_t)m];
            for (int64_t q = f.rp[(size_t)i]; q < f.rp[(size_t)i + 1]; q++) {
                const int32_t J = f.agg[(size_t)f.ci[(size_t)q]];
                if (mark[(size_t)J] != I) {
                    mark[(size_t)J] = I;
                    acc[(size_t)J] = 0.0;
                    touched.push_back(J);
                }
                acc[(size_t)J] = acc[(size_t)J] + (double)va[q];
            }
        }
        std::sort(touched.begin(), touched.end());
        for (int32_t J : touched) {
            c.ci.push_back(J);
            cv.push_back((T)acc[(size_t)J]);
        }
        c.rp[(size_t)I + 1] = (int64_t)c.ci.size();
    }
    c.nnz = (int64_t)c.ci.size();
    c.va.resize(sizeof(T) * cv.size());
    if (!cv.empty()) memcpy(c.va.data(), cv.data(), c.va.size());
}

// The explicit inverse of the dense coarsest matrix, read from its lower triangle: right-looking LDL^T in FSAI's update order, Y = L^-1 by columns
// (y_a = y_a - l_ak * y_k in ascending k), then for j <= i: W_ij = W_ji = T(sum over k = i .. n-1 ascending, from +0, of (Y_ki / d_k) * Y_kj).
// Returns the pivot that is not finite or not > 0, or -1.
template <typename T>
int64_t dense_inverse(const Level &l, std::vector<uint8_t> &winv)
{
    const T     *va = values<T>(l);
    const size_t n = (size_t)l.n;
    std::vector<double> S(n * n, 0.0), Y(n * n, 0.0), d(n, 0.0), W(n * n, 0.0);
    for (size_t i = 0; i < n; i++)
        for (int64_t q = l.rp[i]; q < l.rp[i + 1]; q++) S[i * n + (size_t)l.ci[(size_t)q]] = (double)va[q];
    // l_ak goes to the mirrored position (k, a); s_a = S[a][k] stays where it is
    for (size_t k = 0; k < n; k++) {
        d[k] = S[k * n + k];
        if (!positive_finite(d[k])) return (int64_t)k;
        for (size_t a = k + 1; a < n; a++) S[k * n + a] = S[a * n + k] / d[k];
        for (size_t a = k + 1; a < n; a++) {
            const double lak = S[k * n + a];
            for (size_t b = k + 1; b <= a; b++) S[a * n + b] = S[a * n + b] - lak * S[b * n + k];
        }
    }
    for (size_t c = 0; c < n; c++) Y[c * n + c] = 1.0;
    for (size_t k = 0; k < n; k++)
        for (size_t a = k + 1; a < n; a++) {
            const double lak = S[k * n + a];
            for (size_t c = 0; c <= k; c++) Y[a * n + c] = Y[a * n + c] - lak * Y[k * n + c];
        }
    for (size_t k = 0; k < n; k++)
        for (size_t i = 0; i <= k; i++) {
            const double u = Y[k * n + i] / d[k];
            for (size_t j = 0; j <= i; j++) W[i * n + j] = W[i * n + j] + u * Y[k * n + j];
        }
    winv.assign(sizeof(T) * n * n, 0);
    T *w = reinterpret_cast<T *>(winv.data());
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j <= i; j++) w[i * n + j] = w[j * n + i] = (T)W[i * n + j];
    return -1;
}

template <typename T>
int setup_t(Hierarchy &H, const char *entry, int32_t *bad_level, int64_t *bad_row, const Coarsen *coarsen, Aggregation aggregation)
{
    H.mis2 = aggregation == Aggregation::kMis2;
    std::vector<double> diag;
    for (;;) {
        Level        &l = H.lv.back();
        const int32_t level = (int32_t)H.lv.size() - 1;
        const int64_t bad = diagonal<T>(l, diag);
        if (bad >= 0) {
            *bad_level = level;
            *bad_row = bad;
            return fail(CVR_ERR_STATE, "%s: level %d: the diagonal entry of row %lld is not finite or not > 0", entry, level, (long long)bad);
        }
        smoother_diagonal<T>(l);
        if (l.n <= H.opt.coarse_size || (int32_t)H.lv.size() == H.opt.max_levels) break;
        std::vector<int32_t> agg;
        int32_t              rounds = 0;
        int64_t              nc;
        if (aggregation == Aggregation::kMis2) {
            agg.assign((size_t)l.n, -1);
            nc = mis2_aggregate(l.n, l.rp.data(), l.ci.data(), l.va.data(), sizeof(T) == 4, H.opt.strength, agg.data(), &rounds);
        } else nc = aggregate<T>(l, diag, H.opt.strength, agg);
        if ((double)nc > 0.8 * (double)l.n) break;          // a stall: this level is the last
        H.rounds[level] = rounds;
        l.agg.swap(agg);
        l.nc = nc;
        Level c;
        if (coarsen) {
            if (const int rc = (*coarsen)(l, c, level)) return rc;
        } else {
            members(l);
            coarse_operator<T>(l, c);
        }
        H.lv.push_back(std::move(c));
    }
    const Level &last = H.lv.back();
    if (last.n <= CVR_AMG_MAX_COARSE) {
        H.coarse_direct = 1;
        const int64_t bad = dense_inverse<T>(last, H.winv);
        if (bad >= 0) {
            *bad_level = (int32_t)H.lv.size() - 1;
            *bad_row = bad;
            return fail(CVR_ERR_STATE, "%s: level %d: the pivot of row %lld of the coarsest matrix is not finite or not > 0", entry, *bad_level, (long long)bad);
        }
    }
    return CVR_OK;
}

}  // namespace

int setup(Hierarchy &H, int64_t n, const int64_t *rp, const int32_t *ci, const void *va, int is_f32, const cvr_amg_options *opt, const char *entry, int32_t *bad_level,
          int64_t *bad_row, const Coarsen *coarsen, Aggregation aggregation)
{
    *bad_level = -1;
    *bad_row = -1;
    try {
        H = Hierarchy();
        H.opt = *opt;
        H.is_f32 = is_f32 ? 1 : 0;
        const size_t vsz = is_f32 ? 4 : 8;
        H.lv.emplace_back();
        Level &l = H.lv.back();
        l.n = n;
        l.rp.assign((size_t)n + 1, 0);
        const int64_t base = n > 0 ? rp[0] : 0;
        for (int64_t i = 0; i <= n && n > 0; i++) l.rp[(size_t)i] = rp[i] - base;
        l.nnz = l.rp[(size_t)n];
        if (l.nnz > 0) {
            l.ci.assign(ci + base, ci + base + l.nnz);
            l.va.resize(vsz * (size_t)l.nnz);
            memcpy(l.va.data(), static_cast<const uint8_t *>(va) + vsz * (size_t)base, l.va.size());
        }
        return is_f32 ? setup_t<float>(H, entry, bad_level, bad_row, coarsen, aggregation) : setup_t<double>(H, entry, bad_level, bad_row, coarsen, aggregation);
    } catch (const std::bad_alloc &) {
        return fail(CVR_ERR_NOMEM, "%s: out of host memory (%lld rows)", entry, (long long)n);
    }
}

int64_t coarsest_inverse(const Level &l, int is_f32, std::vector<uint8_t> &winv) { return is_f32 ? dense_inverse<float>(l, winv) : dense_inverse<double>(l, winv); }

void fill_info(const Hierarchy &H, cvr_amg_info *info)
{
    memset(info, 0, sizeof(*info));
    info->levels = (int32_t)H.lv.size();
    info->coarse_direct = H.coarse_direct;
    info->sweeps = H.opt.sweeps;
    info->is_f32 = H.is_f32;
    info->max_levels = H.opt.max_levels;
    info->coarse_size = H.opt.coarse_size;
    info->strength = H.opt.strength;
    info->coarse_scale = H.opt.coarse_scale;
    int64_t total = 0;
    for (size_t l = 0; l < H.lv.size(); l++) {
        info->n[l] = H.lv[l].n;
        info->nnz[l] = H.lv[l].nnz;
        total += H.lv[l].nnz;
    }
    info->operator_complexity = !H.lv.empty() && H.lv[0].nnz > 0 ? (double)total / (double)H.lv[0].nnz : 0.0;
}

int export_level(const Hierarchy &H, int32_t level, int64_t *row_ptr, int32_t *col_idx, void *vals, void *dinv, int32_t *agg, void *winv, const char *entry)
{
    if (level < 0 || level >= (int32_t)H.lv.size()) return fail(CVR_ERR_INVALID, "%s: level = %d: the hierarchy has %d levels", entry, level, (int)H.lv.size());
    const Level &l = H.lv[(size_t)level];
    const bool   last = level + 1 == (int32_t)H.lv.size();
    if (!row_ptr || (l.nnz > 0 && (!col_idx || !vals)) || (l.n > 0 && !dinv) || (!last && !agg) || (last && H.coarse_direct && l.n > 0 && !winv)) return fail(CVR_ERR_INVALID, "null argument");
    std::copy(l.rp.begin(), l.rp.end(), row_ptr);
    if (l.nnz > 0) {
        std::copy(l.ci.begin(), l.ci.end(), col_idx);
        memcpy(vals, l.va.data(), l.va.size());
    }
    if (l.n > 0) memcpy(dinv, l.dinv.data(), l.dinv.size());
    if (!last) std::copy(l.agg.begin(), l.agg.end(), agg);
    if (last && H.coarse_direct && l.n > 0) memcpy(winv, H.winv.data(), H.winv.size());
    return CVR_OK;
}

}  // namespace amg
}  // namespace cvrh

using namespace cvrh;

extern "C" {

int cvr_amg_default_options(cvr_amg_options *opt)
{
    if (!opt) return fail(CVR_ERR_INVALID, "null argument");
    memset(opt, 0, sizeof(*opt));
    opt->max_levels = CVR_AMG_MAX_LEVELS;
    opt->coarse_size = 64;
    opt->sweeps = 1;
    opt->strength = 0.08;
    opt->coarse_scale = 1.0;
    return CVR_OK;
}

int cvr_amg_setup_host(cvr_amg_hierarchy **out, const cvr_csr_view *csr, const cvr_amg_options *opt, int32_t *bad_level, int64_t *bad_row)
{
    if (!out || !csr || !bad_level || !bad_row) return fail(CVR_ERR_INVALID, "null argument");
    *out = nullptr;
    *bad_level = -1;
    *bad_row = -1;
    cvr_amg_options o;
    cvr_amg_default_options(&o);
    if (opt) o = *opt;
    if (const int rc = amg::check_options(&o, "cvr_amg_setup_host")) return rc;
    if (csr->arrays_on_device) return fail(CVR_ERR_INVALID, "cvr_amg_setup_host: the arrays must be host arrays");
    if (csr->nrows != csr->ncols) return fail(CVR_ERR_INVALID, "AMG needs a square matrix (%lld x %lld)", (long long)csr->nrows, (long long)csr->ncols);
    if (const int rc = check_csr(csr, true)) return rc;
    if (csr->nrows >= (int64_t)0x7fffffff) return fail(CVR_ERR_INVALID, "cvr_amg_setup_host: nrows (%lld) must stay below 2^31 - 1", (long long)csr->nrows);
    if (const int rc = amg::check_structure(csr->nrows, csr->row_ptr, csr->col_idx, "cvr_amg_setup_host")) return rc;
    cvr_amg_hierarchy *h = new (std::nothrow) cvr_amg_hierarchy;
    if (!h) return fail(CVR_ERR_NOMEM, "out of host memory");
    if (const int rc = amg::setup(h->H, csr->nrows, csr->row_ptr, csr->col_idx, csr->vals, csr->is_f32, &o, "cvr_amg_setup_host", bad_level, bad_row)) {
        delete h;
        return rc;
    }
    *out = h;
    return CVR_OK;
}

int cvr_amg_hierarchy_info(const cvr_amg_hierarchy *h, cvr_amg_info *info)
{
    if (!h || !info) return fail(CVR_ERR_INVALID, "null argument");
    amg::fill_info(h->H, info);
    return CVR_OK;
}

int cvr_amg_hierarchy_export_level(const cvr_amg_hierarchy *h, int32_t level, int64_t *row_ptr, int32_t *col_idx, void *vals, void *dinv, int32_t *agg, void *winv)
{
    if (!h) return fail(CVR_ERR_INVALID, "null argument");
    return amg::export_level(h->H, level, row_ptr, col_idx, vals, dinv, agg, winv, "cvr_amg_hierarchy_export_level");
}

int cvr_amg_hierarchy_destroy(cvr_amg_hierarchy *h)
{
    delete h;
    return CVR_OK;
}

}  // extern "C"
