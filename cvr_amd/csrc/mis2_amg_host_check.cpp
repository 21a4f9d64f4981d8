// mis2_amg_host_check.cpp -- a stand-alone driver of the MIS(2) aggregation and the set-up with it (cvr_amg_mis2_host.cpp on cvr_amg_host.cpp,
// cvr_amg_smoothed_host.cpp and cvr_spgemm_host.cpp) for `make mis2-amg-asan-check`: the host code under AddressSanitizer and UBSan on n = 0 and
// 1, singletons among coupled rows, a stall, an unsymmetric pattern, a non-zero first row pointer, max_levels = 2, several levels in fp32, with
// agg, every level and every prolongator written into exactly sized arrays, and on every error return.
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

// the aggregation alone into an array of exactly n entries, from arrays of exactly their sizes that begin at row_ptr[0] = shift
template <typename T>
int64_t aggregate(const Csr &m, double strength, int64_t shift, std::vector<int32_t> &agg, int32_t *rounds)
{
    const size_t         n = m.rp.size() - 1;
    std::vector<int64_t> rp(m.rp);
    std::vector<int32_t> ci((size_t)shift, 0);
    std::vector<T>       va((size_t)shift, T(7));
    for (auto &r : rp) r += shift;
    ci.insert(ci.end(), m.ci.begin(), m.ci.end());
    for (double v : m.va) va.push_back((T)v);
    cvr_csr_view v{};
    v.nrows = v.ncols = (int64_t)n;
    v.row_ptr = rp.data();
    v.col_idx = ci.data();
    v.vals = va.data();
    v.is_f32 = sizeof(T) == 4;
    agg.assign(n, -1);
    int64_t nc = -1;
    expect(cvr_amg_mis2_aggregate_host(&v, strength, n ? agg.data() : nullptr, &nc, rounds) == CVR_OK, "aggregate_host");
    std::vector<int> seen((size_t)std::max<int64_t>(nc, 0), 0);
    for (size_t i = 0; i < n; i++) {
        expect(agg[i] >= 0 && agg[i] < nc, "every row is assigned");
        if (agg[i] >= 0 && agg[i] < nc) seen[(size_t)agg[i]] = 1;
    }
    for (int s : seen) expect(s == 1, "no aggregate is empty");
    return nc;
}

// set-up, the three infos, every level and prolongator into arrays of exactly their sizes; returns the code of the set-up
template <typename T>
int run(const Csr &m, const cvr_amg_options *opt, double omega, cvr_amg_info *info, cvr_amg_mis2_info *minfo, int32_t *bad_level, int64_t *bad_row)
{
    std::vector<T> va(m.va.begin(), m.va.end());
    cvr_csr_view   v{};
    v.nrows = v.ncols = (int64_t)m.rp.size() - 1;
    v.row_ptr = m.rp.data();
    v.col_idx = m.ci.data();
    v.vals = va.data();
    v.is_f32 = sizeof(T) == 4;
    cvr_amg_hierarchy *h = nullptr;
    const int          rc = cvr_amg_mis2_setup_host(&h, &v, opt, omega, bad_level, bad_row);
    if (rc) {
        expect(h == nullptr, "no hierarchy behind an error");
        return rc;
    }
    cvr_amg_smoothed_info sinfo;
    expect(cvr_amg_hierarchy_info(h, info) == CVR_OK && cvr_amg_hierarchy_smoothed_info(h, &sinfo) == CVR_OK && sinfo.smoothed == 1, "the infos");
    expect(cvr_amg_hierarchy_mis2_info(h, minfo) == CVR_OK && minfo->mis2 == 1 && minfo->reserved0 == 0, "the MIS(2) info");
    for (int32_t l = 0; l < CVR_AMG_MAX_LEVELS; l++) expect((minfo->rounds[l] > 0) == (l + 1 < info->levels), "rounds above the coarsest level only");
    for (int32_t l = 0; l < info->levels; l++) {
        const size_t         n = (size_t)info->n[l], nnz = (size_t)info->nnz[l], pnnz = (size_t)sinfo.p_nnz[l];
        const bool           last = l + 1 == info->levels;
        std::vector<int64_t> rp(n + 1), prp(n + 1);
        std::vector<int32_t> ci(nnz), agg(last ? 0 : n), pci(pnnz);
        std::vector<T>       vals(nnz), dinv(n), w(last && info->coarse_direct ? n * n : 0), pva(pnnz);
        expect(cvr_amg_hierarchy_export_level(h, l, rp.data(), nnz ? ci.data() : nullptr, nnz ? vals.data() : nullptr, n ? dinv.data() : nullptr, last ? nullptr : agg.data(),
                                              w.empty() ? nullptr : w.data()) == CVR_OK, "export_level");
        expect(rp[n] == (int64_t)nnz, "row_ptr[n] == nnz");
        if (last) continue;
        expect(pnnz >= n && cvr_amg_hierarchy_export_prolongator(h, l, prp.data(), pci.data(), pva.data()) == CVR_OK && prp[n] == (int64_t)pnnz, "export_prolongator");
        for (size_t i = 0; i < n; i++) {
            bool own = false;
            for (int64_t q = prp[i]; q < prp[i + 1]; q++) own = own || pci[(size_t)q] == agg[i];
            expect(own, "row i of P holds column agg[i]");
        }
    }
    expect(cvr_amg_hierarchy_mis2_info(h, nullptr) == CVR_ERR_INVALID && cvr_amg_hierarchy_mis2_info(nullptr, minfo) == CVR_ERR_INVALID, "a null argument of the info");
    cvr_amg_hierarchy_destroy(h);
    return CVR_OK;
}

Csr chain(int n, bool lonely_thirds, double diag)
{
    Csr m;
    for (int i = 0; i < n; i++) {
        auto coupled = [&](int a, int b) { return a >= 0 && b < n && !(lonely_thirds && (a % 3 == 2 || b % 3 == 2)); };
        if (coupled(i - 1, i) && coupled(i, i + 1)) m.row({{i - 1, -1.0}, {i, diag}, {i + 1, -1.0}});
        else if (coupled(i - 1, i)) m.row({{i - 1, -1.0}, {i, diag}});
        else if (coupled(i, i + 1)) m.row({{i, diag}, {i + 1, -1.0}});
        else m.row({{i, diag}});
    }
    return m;
}

Csr laplacian(int g)
{
    Csr m;
    for (int y = 0; y < g; y++)
        for (int x = 0; x < g; x++) {
            const int i = y * g + x;
            if (y > 0) m.ci.push_back(i - g), m.va.push_back(-1.0);
            if (x > 0) m.ci.push_back(i - 1), m.va.push_back(-1.0);
            m.ci.push_back(i), m.va.push_back(4.0);
            if (x + 1 < g) m.ci.push_back(i + 1), m.va.push_back(-1.0);
            if (y + 1 < g) m.ci.push_back(i + g), m.va.push_back(-1.0);
            m.rp.push_back((int64_t)m.ci.size());
        }
    return m;
}

// one-way entries and pairs whose directions differ in strength
Csr lopsided(int n)
{
    Csr m;
    for (int i = 0; i < n; i++) {
        if (i >= 5 && i % 4 == 1) m.ci.push_back(i - 5), m.va.push_back(i % 8 == 1 ? -0.125 : -0.75);
        if (i > 0) m.ci.push_back(i - 1), m.va.push_back(i % 3 == 1 ? -0.25 : -1.0);
        m.ci.push_back(i), m.va.push_back(4.0);
        if (i + 1 < n) m.ci.push_back(i + 1), m.va.push_back(-1.0 - 0.125 * (i % 4));
        if (i + 7 < n && i % 2 == 0) m.ci.push_back(i + 7), m.va.push_back(-0.5);
        m.rp.push_back((int64_t)m.ci.size());
    }
    return m;
}

}  // namespace

int main()
{
    cvr_amg_options o;
    cvr_amg_default_options(&o);
    cvr_amg_info      info;
    cvr_amg_mis2_info minfo;
    int32_t           bl = 0, rounds = -1;
    int64_t           br = 0;
    std::vector<int32_t> agg;
    // the aggregation alone
    Csr empty;
    expect(aggregate<double>(empty, 0.08, 0, agg, &rounds) == 0 && rounds == 0, "n = 0: no aggregate, no round");
    Csr one;
    one.row({{0, 3.0}});
    expect(aggregate<double>(one, 0.08, 0, agg, &rounds) == 1 && rounds == 1 && agg[0] == 0, "n = 1: a singleton in one round");
    const Csr lonely = chain(90, true, 2.5), lap = laplacian(24), lop = lopsided(61);
    for (int64_t shift : {0, 5}) {
        std::vector<int32_t> a64, a32;
        int32_t              r64 = 0, r32 = 0;
        expect(aggregate<double>(lonely, 0.08, shift, a64, &r64) == 60, "singletons: 30 pairs and 30 singletons");
        expect(aggregate<double>(lap, 0.08, shift, a64, &r64) == aggregate<float>(lap, 0.08, shift, a32, &r32) && a64 == a32 && r64 == r32 && r64 > 1, "the Laplacian in both types");
        expect(aggregate<double>(lop, 0.08, shift, a64, &r64) > 0 && aggregate<double>(lop, 0.5, shift, a64, &r64) > 0 && aggregate<double>(lop, 0.0, shift, a64, &r64) > 0, "the unsymmetric pattern");
    }
    {
        cvr_csr_view v{};
        v.nrows = v.ncols = 1;
        v.row_ptr = one.rp.data();
        v.col_idx = one.ci.data();
        v.vals = one.va.data();
        int64_t nc = 0;
        int32_t a0 = 0;
        expect(cvr_amg_mis2_aggregate_host(nullptr, 0.08, &a0, &nc, &rounds) == CVR_ERR_INVALID && cvr_amg_mis2_aggregate_host(&v, 0.08, nullptr, &nc, &rounds) == CVR_ERR_INVALID &&
                   cvr_amg_mis2_aggregate_host(&v, 0.08, &a0, nullptr, &rounds) == CVR_ERR_INVALID && cvr_amg_mis2_aggregate_host(&v, 0.08, &a0, &nc, nullptr) == CVR_ERR_INVALID, "null arguments");
        for (double s : {-0.1, 1.0, std::numeric_limits<double>::quiet_NaN()}) expect(cvr_amg_mis2_aggregate_host(&v, s, &a0, &nc, &rounds) == CVR_ERR_INVALID, "a strength outside [0, 1)");
        v.arrays_on_device = 1;
        expect(cvr_amg_mis2_aggregate_host(&v, 0.08, &a0, &nc, &rounds) == CVR_ERR_INVALID, "device arrays");
        v.arrays_on_device = 0;
        v.ncols = 2;
        expect(cvr_amg_mis2_aggregate_host(&v, 0.08, &a0, &nc, &rounds) == CVR_ERR_INVALID, "not square");
        Csr nodiag;
        nodiag.row({{1, 1.0}});
        nodiag.row({{1, 1.0}});
        v.nrows = v.ncols = 2;
        v.row_ptr = nodiag.rp.data();
        v.col_idx = nodiag.ci.data();
        v.vals = nodiag.va.data();
        int32_t a2[2];
        expect(cvr_amg_mis2_aggregate_host(&v, 0.08, a2, &nc, &rounds) == CVR_ERR_INVALID, "a row without its diagonal entry");
    }
    // the set-up
    expect(run<double>(empty, nullptr, 0.0, &info, &minfo, &bl, &br) == CVR_OK && info.levels == 1 && info.n[0] == 0 && info.coarse_direct == 1, "n = 0");
    expect(run<double>(one, nullptr, 0.0, &info, &minfo, &bl, &br) == CVR_OK && info.levels == 1 && info.coarse_direct == 1, "n = 1");
    expect(run<double>(lonely, nullptr, 0.0, &info, &minfo, &bl, &br) == CVR_OK && info.levels == 2 && info.n[1] == 60, "singletons");
    Csr diag;
    for (int i = 0; i < 300; i++) diag.row({{i, 1.0 + i % 5}});
    expect(run<double>(diag, nullptr, 0.0, &info, &minfo, &bl, &br) == CVR_OK && info.levels == 1 && info.coarse_direct == 0, "a stall: one level");
    expect(run<double>(lap, nullptr, 0.0, &info, &minfo, &bl, &br) == CVR_OK && info.levels == 3 && minfo.rounds[0] > 1 && minfo.rounds[1] > 0, "the Laplacian, fp64");
    expect(run<float>(lap, nullptr, 0.9, &info, &minfo, &bl, &br) == CVR_OK && info.levels == 3 && info.is_f32 == 1, "the Laplacian, fp32, omega = 0.9");
    o.max_levels = 2;
    expect(run<double>(laplacian(40), &o, 0.0, &info, &minfo, &bl, &br) == CVR_OK && info.levels == 2 && minfo.rounds[1] == 0, "max_levels = 2");
    cvr_amg_default_options(&o);
    // every error return
    expect(run<double>(lap, nullptr, 2.0, &info, &minfo, &bl, &br) == CVR_ERR_INVALID, "omega = 2");
    expect(run<double>(lap, nullptr, std::numeric_limits<double>::quiet_NaN(), &info, &minfo, &bl, &br) == CVR_ERR_INVALID, "omega = NaN");
    o.sweeps = 5;
    expect(run<double>(lap, &o, 0.0, &info, &minfo, &bl, &br) == CVR_ERR_INVALID, "sweeps = 5");
    cvr_amg_default_options(&o);
    Csr bad = chain(100, false, 2.5);
    bad.va[(size_t)bad.rp[40] + 1] = -2.5;
    expect(run<double>(bad, nullptr, 0.0, &info, &minfo, &bl, &br) == CVR_ERR_STATE && bl == 0 && br == 40, "a bad diagonal names level 0, row 40");
    Csr indefinite;
    indefinite.row({{0, 1.0}, {1, 2.0}});
    indefinite.row({{0, 2.0}, {1, 1.0}});
    indefinite.row({{2, 1.0}});
    expect(run<double>(indefinite, nullptr, 0.0, &info, &minfo, &bl, &br) == CVR_ERR_STATE && bl == 0 && br == 1, "a non-positive pivot names level 0, row 1");
    Csr unsorted;
    unsorted.row({{1, -1.0}, {0, 2.0}});
    unsorted.row({{0, -1.0}, {1, 2.0}});
    expect(run<double>(unsorted, nullptr, 0.0, &info, &minfo, &bl, &br) == CVR_ERR_INVALID, "columns out of order");
    {
        cvr_csr_view v{};
        v.nrows = v.ncols = 1;
        v.row_ptr = one.rp.data();
        v.col_idx = one.ci.data();
        v.vals = one.va.data();
        cvr_amg_hierarchy *h = nullptr;
        expect(cvr_amg_mis2_setup_host(nullptr, &v, nullptr, 0.0, &bl, &br) == CVR_ERR_INVALID && cvr_amg_mis2_setup_host(&h, nullptr, nullptr, 0.0, &bl, &br) == CVR_ERR_INVALID &&
                   cvr_amg_mis2_setup_host(&h, &v, nullptr, 0.0, nullptr, &br) == CVR_ERR_INVALID && cvr_amg_mis2_setup_host(&h, &v, nullptr, 0.0, &bl, nullptr) == CVR_ERR_INVALID, "null arguments of the set-up");
        v.arrays_on_device = 1;
        expect(cvr_amg_mis2_setup_host(&h, &v, nullptr, 0.0, &bl, &br) == CVR_ERR_INVALID && h == nullptr, "device arrays");
    }
    if (failures) {
        fprintf(stderr, "mis2_amg_host_check: %d failure(s)\n", failures);
        return 1;
    }
    printf("mis2_amg_host_check: ok\n");
    return 0;
}
