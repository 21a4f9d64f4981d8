// cvr_amg_smoothed_host.cpp -- the host half of smoothed-aggregation AMG (include/cvr_amd.h: cvr_amg_smoothed_setup_host and the calls that read a
// smoothed hierarchy): the check of omega, one coarsening step in host code -- the tentative prolongator, G = A T and A_c = R (A P) through
// cvr_spgemm_host, the prolongator smoother and the stable transpose in loops --, the info and the export of a prolongator.  Everything before and
// behind that step is cvr_amg_host.cpp's set-up, unchanged.  Every fp64 operation is rounded on its own (this file is compiled without
// contraction).  No HIP: with cvr_amg_host.cpp and cvr_spgemm_host.cpp it links into a stand-alone host program.
#include "cvr_amg.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

namespace cvrh {
namespace amg {

int check_omega(double omega, double *used, const char *entry)
{
    if (omega == 0.0) {
        *used = 4.0 / 3.0;
        return CVR_OK;
    }
    if (!(omega > 0 && omega < 2)) return fail(CVR_ERR_INVALID, "%s: omega = %g: must be 0 (the default 4/3) or finite with 0 < omega < 2", entry, omega);
    *used = omega;
    return CVR_OK;
}

namespace {

struct Csr {
    int64_t              nrows = 0, ncols = 0;
    std::vector<int64_t> rp;
    std::vector<int32_t> ci;
    std::vector<uint8_t> va;
    cvr_csr_view view(int is_f32) const
    {
        cvr_csr_view v{};
        v.nrows = nrows;
        v.ncols = ncols;
        v.row_ptr = rp.data();
        v.col_idx = ci.data();
        v.vals = va.data();
        v.is_f32 = is_f32;
        return v;
    }
};

// C = A B through the two calls of cvr_spgemm_host
int product(const cvr_csr_view &a, const cvr_csr_view &b, Csr &c)
{
    const size_t vsz = a.is_f32 ? 4 : 8;
    int64_t      bad = -1;
    c.nrows = a.nrows;
    c.ncols = b.ncols;
    c.rp.assign((size_t)a.nrows + 1, 0);
    if (const int rc = cvr_spgemm_host(&a, &b, c.rp.data(), nullptr, nullptr, &bad)) return rc;
    const size_t nnz = (size_t)c.rp.back();
    c.ci.assign(std::max<size_t>(nnz, 1), 0);          // (never a null array for an empty product)
    c.va.assign(vsz * std::max<size_t>(nnz, 1), 0);
    if (const int rc = cvr_spgemm_host(&a, &b, c.rp.data(), c.ci.data(), c.va.data(), &bad)) return rc;
    c.ci.resize(nnz);
    c.va.resize(vsz * nnz);
    return CVR_OK;
}

template <typename T>
int coarsen_t(Level &f, Level &c, double omega)
{
    const int    is_f32 = sizeof(T) == 4;
    const size_t n = (size_t)f.n;
    cvr_csr_view a{};
    a.nrows = a.ncols = f.n;
    a.row_ptr = f.rp.data();
    a.col_idx = f.ci.data();
    a.vals = f.va.data();
    a.is_f32 = is_f32;
    // 1. T: one 1.0 per row in column agg[i]
    Csr t;
    t.nrows = f.n;
    t.ncols = f.nc;
    t.rp.resize(n + 1);
    for (size_t i = 0; i <= n; i++) t.rp[i] = (int64_t)i;
    t.ci.assign(f.agg.begin(), f.agg.end());
    t.va.resize(sizeof(T) * n);
    for (size_t i = 0; i < n; i++) reinterpret_cast<T *>(t.va.data())[i] = T(1);
    // 2. G = A T;  3. P on G's pattern, in G's arrays
    Csr p;
    if (const int rc = product(a, t.view(is_f32), p)) return rc;
    const T *dinv = reinterpret_cast<const T *>(f.dinv.data());
    T       *pv = reinterpret_cast<T *>(p.va.data());
    for (size_t i = 0; i < n; i++) {
        const double w = omega * (double)dinv[i];
        for (int64_t q = p.rp[i]; q < p.rp[i + 1]; q++) {
            const double wg = w * (double)pv[q];
            pv[q] = (T)((p.ci[(size_t)q] == f.agg[i] ? 1.0 : 0.0) - wg);
        }
    }
    // 4. R = P^T, stable: row J takes column J's entries in ascending row of P
    Csr          r;
    const size_t pnnz = p.ci.size();
    r.nrows = f.nc;
    r.ncols = f.n;
    r.rp.assign((size_t)f.nc + 1, 0);
    r.ci.resize(pnnz);
    r.va.resize(sizeof(T) * pnnz);
    for (size_t q = 0; q < pnnz; q++) r.rp[(size_t)p.ci[q] + 1]++;
    for (size_t J = 0; J < (size_t)f.nc; J++) r.rp[J + 1] += r.rp[J];
    {
        std::vector<int64_t> at(r.rp.begin(), r.rp.end() - 1);
        T                   *rv = reinterpret_cast<T *>(r.va.data());
        for (size_t i = 0; i < n; i++)
            for (int64_t q = p.rp[i]; q < p.rp[i + 1]; q++) {
                const int64_t d = at[(size_t)p.ci[(size_t)q]]++;
                r.ci[(size_t)d] = (int32_t)i;
                rv[d] = pv[q];
            }
    }
    // 5. A_c = R (A P)
    Csr ap, ac;
    if (const int rc = product(a, p.view(is_f32), ap)) return rc;
    if (const int rc = product(r.view(is_f32), ap.view(is_f32), ac)) return rc;
    c.n = f.nc;
    c.nnz = (int64_t)ac.ci.size();
    c.rp.swap(ac.rp);
    c.ci.swap(ac.ci);
    c.va.swap(ac.va);
    f.prp.swap(p.rp);
    f.pci.swap(p.ci);
    f.pva.swap(p.va);
    f.pnnz = (int64_t)pnnz;
    return CVR_OK;
}

}  // namespace

int smoothed_coarsen_host(Level &fine, Level &coarse, int is_f32, double omega)
{
    return is_f32 ? coarsen_t<float>(fine, coarse, omega) : coarsen_t<double>(fine, coarse, omega);
}

int products_per_apply(const Hierarchy &H)
{
    const int s = H.opt.sweeps, L = (int)H.lv.size();
    return (H.smoothed ? 2 * s + 2 : 2 * s) * (L - 1) + (H.coarse_direct ? 0 : 2 * s - 1);
}

void fill_smoothed_info(const Hierarchy &H, cvr_amg_smoothed_info *info)
{
    memset(info, 0, sizeof(*info));
    if (!H.smoothed) return;
    info->smoothed = 1;
    info->products_per_apply = products_per_apply(H);
    info->omega = H.omega;
    for (size_t l = 0; l + 1 < H.lv.size(); l++) info->p_nnz[l] = H.lv[l].pnnz;
}

int export_prolongator(const Hierarchy &H, int32_t level, int64_t *row_ptr, int32_t *col_idx, void *vals, const char *entry)
{
    if (!H.smoothed) return fail(CVR_ERR_INVALID, "%s: the hierarchy is a plain one: it has no stored prolongator (agg is its prolongator)", entry);
    if (level < 0 || level + 1 >= (int32_t)H.lv.size())
        return fail(CVR_ERR_INVALID, "%s: level = %d: the hierarchy has %d levels, prolongators on levels 0 .. %d", entry, level, (int)H.lv.size(), (int)H.lv.size() - 2);
    if (!row_ptr || !col_idx || !vals) return fail(CVR_ERR_INVALID, "null argument");          // (a prolongator has an entry in every row)
    const Level &l = H.lv[(size_t)level];
    std::copy(l.prp.begin(), l.prp.end(), row_ptr);
    std::copy(l.pci.begin(), l.pci.end(), col_idx);
    memcpy(vals, l.pva.data(), l.pva.size());
    return CVR_OK;
}

}  // namespace amg
}  // namespace cvrh

using namespace cvrh;

extern "C" {

int cvr_amg_smoothed_setup_host(cvr_amg_hierarchy **out, const cvr_csr_view *csr, const cvr_amg_options *opt, double omega, int32_t *bad_level, int64_t *bad_row)
{
    const char *entry = "cvr_amg_smoothed_setup_host";
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
    if (const int rc = amg::setup(h->H, csr->nrows, csr->row_ptr, csr->col_idx, csr->vals, is_f32, &o, entry, bad_level, bad_row, &coarsen)) {
        delete h;
        return rc;
    }
    h->H.smoothed = 1;
    h->H.omega = used;
    *out = h;
    return CVR_OK;
}

int cvr_amg_hierarchy_smoothed_info(const cvr_amg_hierarchy *h, cvr_amg_smoothed_info *info)
{
    if (!h || !info) return fail(CVR_ERR_INVALID, "null argument");
    amg::fill_smoothed_info(h->H, info);
    return CVR_OK;
}

int cvr_amg_hierarchy_export_prolongator(const cvr_amg_hierarchy *h, int32_t level, int64_t *row_ptr, int32_t *col_idx, void *vals)
{
    if (!h) return fail(CVR_ERR_INVALID, "null argument");
    return amg::export_prolongator(h->H, level, row_ptr, col_idx, vals, "cvr_amg_hierarchy_export_prolongator");
}

}  // extern "C"
