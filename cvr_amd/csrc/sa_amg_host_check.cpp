// sa_amg_host_check.cpp -- a stand-alone driver of the smoothed-aggregation set-up (cvr_amg_smoothed_host.cpp on cvr_amg_host.cpp and
// cvr_spgemm_host.cpp) for `make sa-amg-asan-check`: the host code under AddressSanitizer and UBSan on n = 0, singletons among coupled rows, a
// stall, max_levels = 2, several levels in fp32 and a non-default omega, with every level and every prolongator exported into exactly sized arrays,
// and on every error return.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "cvr_amg.h"

namespace cvrh {
static char g_msg[512];
int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    return code;
}
int check_csr(const cvr_csr_view *c, bool)
{
    if (c->nrows < 0 || (c->nrows > 0 && !c->row_ptr)) return fail(CVR_ERR_INVALID, "null or negative-size CSR view");
    for (int64_t i = 0; i < c->nrows; i++)
        if (c->row_ptr[i + 1] < c->row_ptr[i]) return fail(CVR_ERR_INVALID, "row_ptr decreases at row %lld", (long long)i);
    for (int64_t q = c->nrows > 0 ? c->row_ptr[0] : 0; c->nrows > 0 && q < c->row_ptr[c->nrows]; q++)
        if (c->col_idx[q] < 0 || c->col_idx[q] >= c->ncols) return fail(CVR_ERR_INVALID, "col_idx[%lld] outside the matrix", (long long)q);
    return CVR_OK;
}
}  // namespace cvrh

namespace {

struct Csr {
    std::vector<int64_t> rp{0};
    std::vector<int32_t> ci;
    std::vector<double>  va;
    void row(std::initializer_list<std::pair<int, double>> e)
    {
        for (auto &p : e) {
            ci.push_back(p.first);
            va.push_back(p.second);
        }
        rp.push_back((int64_t)ci.size());
    }
};

int failures = 0;

void expect(bool ok, const char *what)
{
    if (!ok) {
        fprintf(stderr, "FAILED: %s (%s)\n", what, cvrh::g_msg);
        failures++;
    }
}

// set-up, both infos, every level and prolongator into arrays of exactly their sizes; returns the code of the set-up
template <typename T>
int run(const Csr &m, const cvr_amg_options *opt, double omega, cvr_amg_info *info, cvr_amg_smoothed_info *sinfo, int32_t *bad_level, int64_t *bad_row)
{
    std::vector<T> va(m.va.begin(), m.va.end());
    cvr_csr_view   v{};
    v.nrows = v.ncols = (int64_t)m.rp.size() - 1;
    v.row_ptr = m.rp.data();
    v.col_idx = m.ci.data();
    v.vals = va.data();
    v.is_f32 = sizeof(T) == 4;
    cvr_amg_hierarchy *h = nullptr;
    const int          rc = cvr_amg_smoothed_setup_host(&h, &v, opt, omega, bad_level, bad_row);
    if (rc) {
        expect(h == nullptr, "no hierarchy behind an error");
        return rc;
    }
    expect(cvr_amg_hierarchy_info(h, info) == CVR_OK && cvr_amg_hierarchy_smoothed_info(h, sinfo) == CVR_OK && sinfo->smoothed == 1, "the infos");
    for (int32_t l = 0; l < info->levels; l++) {
        const size_t         n = (size_t)info->n[l], nnz = (size_t)info->nnz[l], pnnz = (size_t)sinfo->p_nnz[l];
        const bool           last = l + 1 == info->levels;
        std::vector<int64_t> rp(n + 1), prp(n + 1);
        std::vector<int32_t> ci(nnz), agg(last ? 0 : n), pci(pnnz);
        std::vector<T>       vals(nnz), dinv(n), w(last && info->coarse_direct ? n * n : 0), pva(pnnz);
        expect(cvr_amg_hierarchy_export_level(h, l, rp.data(), nnz ? ci.data() : nullptr, nnz ? vals.data() : nullptr, n ? dinv.data() : nullptr, last ? nullptr : agg.data(),
                                              w.empty() ? nullptr : w.data()) == CVR_OK, "export_level");
        expect(rp[n] == (int64_t)nnz, "row_ptr[n] == nnz");
        if (last) {
            expect(pnnz == 0 && cvr_amg_hierarchy_export_prolongator(h, l, prp.data(), reinterpret_cast<int32_t *>(prp.data()), prp.data()) == CVR_ERR_INVALID, "no prolongator on the coarsest level");
            continue;
        }
        expect(pnnz >= n && cvr_amg_hierarchy_export_prolongator(h, l, prp.data(), pci.data(), pva.data()) == CVR_OK && prp[n] == (int64_t)pnnz, "export_prolongator");
        for (size_t i = 0; i < n; i++) {
            bool own = false;
            for (int64_t q = prp[i]; q < prp[i + 1]; q++) own = own || pci[(size_t)q] == agg[i];
            expect(own, "row i of P holds column agg[i]");
        }
        expect(cvr_amg_hierarchy_export_prolongator(h, l, nullptr, pci.data(), pva.data()) == CVR_ERR_INVALID, "a null row_ptr");
        expect(cvr_amg_hierarchy_export_prolongator(h, l, prp.data(), nullptr, pva.data()) == CVR_ERR_INVALID, "a null col_idx");
        expect(cvr_amg_hierarchy_export_prolongator(h, l, prp.data(), pci.data(), nullptr) == CVR_ERR_INVALID, "a null vals");
    }
    int64_t one = 0;
    expect(cvr_amg_hierarchy_export_prolongator(h, -1, &one, reinterpret_cast<int32_t *>(&one), &one) == CVR_ERR_INVALID, "level -1");
    expect(cvr_amg_hierarchy_export_prolongator(h, info->levels, &one, reinterpret_cast<int32_t *>(&one), &one) == CVR_ERR_INVALID, "level = levels");
    expect(cvr_amg_hierarchy_smoothed_info(h, nullptr) == CVR_ERR_INVALID, "a null info");
    cvr_amg_hierarchy_destroy(h);
    return CVR_OK;
}

Csr chain(int n, bool lonely_thirds, double diag)
{
    Csr m;
    for (int i = 0; i < n; i++) {
        const bool left = i > 0 && !(lonely_thirds && (i % 3 == 2 || (i - 1) % 3 == 2)), right = i + 1 < n && !(lonely_thirds && (i % 3 == 2 || (i + 1) % 3 == 2));
        if (left && right) m.row({{i - 1, -1.0}, {i, diag}, {i + 1, -1.0}});
        else if (left) m.row({{i - 1, -1.0}, {i, diag}});
        else if (right) m.row({{i, diag}, {i + 1, -1.0}});
        else m.row({{i, diag}});
    }
    return m;
}

Csr laplacian(int m)
{
    Csr a;
    for (int y = 0; y < m; y++)
        for (int x = 0; x < m; x++) {
            const int i = y * m + x;
            if (y > 0) { a.ci.push_back(i - m); a.va.push_back(-1.0); }
            if (x > 0) { a.ci.push_back(i - 1); a.va.push_back(-1.0); }
            a.ci.push_back(i); a.va.push_back(4.0);
            if (x + 1 < m) { a.ci.push_back(i + 1); a.va.push_back(-1.0); }
            if (y + 1 < m) { a.ci.push_back(i + m); a.va.push_back(-1.0); }
            a.rp.push_back((int64_t)a.ci.size());
        }
    return a;
}

}  // namespace

int main()
{
    cvr_amg_info          info;
    cvr_amg_smoothed_info si;
    int32_t               bl;
    int64_t               br;
    const double          nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // singletons among coupled rows, fp64 and fp32; a grid: several levels, the default omega reported as 4/3
    expect(run<double>(chain(90, true, 2.5), nullptr, 0.0, &info, &si, &bl, &br) == CVR_OK && info.levels == 2 && info.n[1] == 60 && si.p_nnz[0] == 90, "singletons");
    expect(run<float>(chain(90, true, 2.5), nullptr, 0.0, &info, &si, &bl, &br) == CVR_OK && info.levels == 2, "singletons, fp32");
    expect(run<double>(laplacian(40), nullptr, 0.0, &info, &si, &bl, &br) == CVR_OK && info.levels == 3 && info.coarse_direct == 1 && si.omega == 4.0 / 3.0 && si.products_per_apply == 8,
           "the 40 x 40 Laplacian");
    expect(run<float>(laplacian(23), nullptr, 0.7, &info, &si, &bl, &br) == CVR_OK && info.levels == 3 && si.omega == 0.7, "the 23 x 23 Laplacian, fp32, omega = 0.7");
    expect(run<float>(chain(5000, false, 2.0), nullptr, 0.0, &info, &si, &bl, &br) == CVR_OK && info.levels >= 4 && info.coarse_direct == 1, "a chain of 5000 rows, fp32");
    cvr_amg_options o;
    cvr_amg_default_options(&o);
    // max_levels = 2: a coarsest level of 280 rows, smoothed and not inverted
    o.max_levels = 2;
    expect(run<double>(laplacian(40), &o, 0.0, &info, &si, &bl, &br) == CVR_OK && info.levels == 2 && info.n[1] == 280 && info.coarse_direct == 0 && si.products_per_apply == 5, "max_levels = 2");
    cvr_amg_default_options(&o);
    o.coarse_size = 1;
    o.sweeps = 4;
    expect(run<double>(chain(700, false, 2.5), &o, 1.9, &info, &si, &bl, &br) == CVR_OK && info.levels >= 3, "coarse_size = 1, sweeps = 4");
    // a stall: 300 rows with the diagonal alone -- one level, no prolongator
    Csr d;
    for (int i = 0; i < 300; i++) d.row({{i, 1.0 + i % 5}});
    expect(run<double>(d, nullptr, 0.0, &info, &si, &bl, &br) == CVR_OK && info.levels == 1 && info.coarse_direct == 0 && si.p_nnz[0] == 0 && si.products_per_apply == 1, "stall");
    // n = 0
    expect(run<double>(Csr(), nullptr, 0.0, &info, &si, &bl, &br) == CVR_OK && info.levels == 1 && info.n[0] == 0 && info.coarse_direct == 1 && si.products_per_apply == 0, "n = 0");
    // a stored 0.0 off the diagonal keeps its entry
    Csr z = chain(120, false, 3.0);
    z.va[(size_t)z.rp[10]] = 0.0;
    expect(run<double>(z, nullptr, 0.0, &info, &si, &bl, &br) == CVR_OK, "a stored zero");
    // the errors: omega, the options in front of it, a bad diagonal on level 0, a bad pivot, the structure, the nulls
    for (double w : {nan, -0.5, 2.0, inf, -inf})
        expect(run<double>(chain(10, false, 2.5), nullptr, w, &info, &si, &bl, &br) == CVR_ERR_INVALID, "a bad omega");
    cvr_amg_default_options(&o);
    o.sweeps = 5;
    expect(run<double>(chain(10, false, 2.5), &o, nan, &info, &si, &bl, &br) == CVR_ERR_INVALID, "a bad option");
    cvr_amg_default_options(&o);
    o.reserved[3] = 1;
    expect(run<double>(chain(10, false, 2.5), &o, 0.0, &info, &si, &bl, &br) == CVR_ERR_INVALID, "a reserved word");
    Csr b = chain(300, false, 2.5);
    b.va[(size_t)b.rp[123] + 1] = -1.0;
    expect(run<double>(b, nullptr, 0.0, &info, &si, &bl, &br) == CVR_ERR_STATE && bl == 0 && br == 123, "a bad diagonal");
    Csr p;
    p.row({{0, 1.0}, {1, 2.0}});
    p.row({{0, 2.0}, {1, 1.0}});
    expect(run<double>(p, nullptr, 0.0, &info, &si, &bl, &br) == CVR_ERR_STATE && bl == 0 && br == 1, "a bad pivot");
    Csr u;
    u.row({{1, 1.0}, {0, 1.0}});
    u.row({{1, 1.0}});
    expect(run<double>(u, nullptr, 0.0, &info, &si, &bl, &br) == CVR_ERR_INVALID, "unsorted columns");
    {
        Csr            c = chain(10, false, 2.5);
        cvr_csr_view   v{};
        cvr_amg_hierarchy *h = nullptr;
        v.nrows = v.ncols = 10;
        v.row_ptr = c.rp.data();
        v.col_idx = c.ci.data();
        v.vals = c.va.data();
        expect(cvr_amg_smoothed_setup_host(nullptr, &v, nullptr, 0.0, &bl, &br) == CVR_ERR_INVALID && cvr_amg_smoothed_setup_host(&h, nullptr, nullptr, 0.0, &bl, &br) == CVR_ERR_INVALID &&
                   cvr_amg_smoothed_setup_host(&h, &v, nullptr, 0.0, nullptr, &br) == CVR_ERR_INVALID && cvr_amg_smoothed_setup_host(&h, &v, nullptr, 0.0, &bl, nullptr) == CVR_ERR_INVALID, "null arguments");
        v.ncols = 11;
        expect(cvr_amg_smoothed_setup_host(&h, &v, nullptr, 0.0, &bl, &br) == CVR_ERR_INVALID, "not square");
        v.ncols = 10;
        v.arrays_on_device = 1;
        expect(cvr_amg_smoothed_setup_host(&h, &v, nullptr, 0.0, &bl, &br) == CVR_ERR_INVALID, "device arrays");
        v.arrays_on_device = 0;
        // a plain hierarchy: the smoothed info all zero, no prolongator
        expect(cvr_amg_setup_host(&h, &v, nullptr, &bl, &br) == CVR_OK, "the plain set-up");
        int64_t one = 0;
        expect(cvr_amg_hierarchy_smoothed_info(h, &si) == CVR_OK && si.smoothed == 0 && si.omega == 0 && si.products_per_apply == 0 && si.p_nnz[0] == 0, "the info of a plain hierarchy");
        expect(cvr_amg_hierarchy_export_prolongator(h, 0, &one, reinterpret_cast<int32_t *>(&one), &one) == CVR_ERR_INVALID, "no prolongator of a plain hierarchy");
        expect(cvr_amg_hierarchy_export_prolongator(nullptr, 0, &one, reinterpret_cast<int32_t *>(&one), &one) == CVR_ERR_INVALID, "a null hierarchy");
        cvr_amg_hierarchy_destroy(h);
    }
    if (failures) return 1;
    printf("sa_amg_host_check: all cases ran clean\n");
    return 0;
}
