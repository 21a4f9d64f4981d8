// amg_host_check.cpp -- a stand-alone driver of the AMG set-up (cvr_amg_host.cpp) for `make amg-asan-check`: the host code under AddressSanitizer
// and UBSan on the cases whose index arithmetic differs -- singletons among coupled rows, a stall (one level, no direct solve), n = 0, a bad
// diagonal, a singular coarsest matrix, a hierarchy of several levels in fp32 -- with every level exported into exactly sized arrays.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
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

// set-up, info, every level exported into arrays of exactly the level's sizes; returns the code of the set-up
template <typename T>
int run(const Csr &m, const cvr_amg_options *opt, cvr_amg_info *info, int32_t *bad_level, int64_t *bad_row)
{
    std::vector<T> va(m.va.begin(), m.va.end());
    cvr_csr_view   v{};
    v.nrows = v.ncols = (int64_t)m.rp.size() - 1;
    v.row_ptr = m.rp.data();
    v.col_idx = m.ci.data();
    v.vals = va.data();
    v.is_f32 = sizeof(T) == 4;
    cvr_amg_hierarchy *h = nullptr;
    const int          rc = cvr_amg_setup_host(&h, &v, opt, bad_level, bad_row);
    if (rc) return rc;
    expect(cvr_amg_hierarchy_info(h, info) == CVR_OK, "info");
    for (int32_t l = 0; l < info->levels; l++) {
        const size_t         n = (size_t)info->n[l], nnz = (size_t)info->nnz[l];
        const bool           last = l + 1 == info->levels;
        std::vector<int64_t> rp(n + 1);
        std::vector<int32_t> ci(nnz), agg(last ? 0 : n);
        std::vector<T>       vals(nnz), dinv(n), w(last && info->coarse_direct ? n * n : 0);
        expect(cvr_amg_hierarchy_export_level(h, l, rp.data(), nnz ? ci.data() : nullptr, nnz ? vals.data() : nullptr, n ? dinv.data() : nullptr, last ? nullptr : agg.data(),
                                              w.empty() ? nullptr : w.data()) == CVR_OK, "export");
        expect(rp[n] == (int64_t)nnz, "row_ptr[n] == nnz");
    }
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

}  // namespace

int main()
{
    cvr_amg_info info;
    int32_t      bl;
    int64_t      br;
    // singletons among coupled rows, fp64 and fp32; a long chain: several levels
    expect(run<double>(chain(90, true, 2.5), nullptr, &info, &bl, &br) == CVR_OK && info.levels == 2 && info.n[1] == 60, "singletons");
    expect(run<float>(chain(90, true, 2.5), nullptr, &info, &bl, &br) == CVR_OK && info.levels == 2, "singletons, fp32");
    expect(run<float>(chain(5000, false, 2.5), nullptr, &info, &bl, &br) == CVR_OK && info.levels >= 4 && info.coarse_direct == 1, "a chain of 5000 rows");
    cvr_amg_options o;
    cvr_amg_default_options(&o);
    o.coarse_size = 1;
    o.sweeps = 4;
    expect(run<double>(chain(700, false, 2.5), &o, &info, &bl, &br) == CVR_OK && info.levels >= 3, "coarse_size = 1, sweeps = 4");
    // a stall: 300 rows with the diagonal alone
    Csr d;
    for (int i = 0; i < 300; i++) d.row({{i, 1.0 + i % 5}});
    expect(run<double>(d, nullptr, &info, &bl, &br) == CVR_OK && info.levels == 1 && info.coarse_direct == 0, "stall");
    // n = 0
    expect(run<double>(Csr(), nullptr, &info, &bl, &br) == CVR_OK && info.levels == 1 && info.n[0] == 0 && info.coarse_direct == 1, "n = 0");
    // a bad diagonal on level 0; a bad pivot of the coarsest matrix on level 0 and, for the Neumann chain (row sums 0), on a coarse level
    Csr b = chain(300, false, 2.5);
    b.va[(size_t)b.rp[123] + 1] = -1.0;
    expect(run<double>(b, nullptr, &info, &bl, &br) == CVR_ERR_STATE && bl == 0 && br == 123, "a bad diagonal");
    Csr p;
    p.row({{0, 1.0}, {1, 2.0}});
    p.row({{0, 2.0}, {1, 1.0}});
    expect(run<double>(p, nullptr, &info, &bl, &br) == CVR_ERR_STATE && bl == 0 && br == 1, "a bad pivot");
    Csr s = chain(100, false, 2.0);
    s.va[0] = 1.0;
    s.va.back() = 1.0;
    expect(run<double>(s, nullptr, &info, &bl, &br) == CVR_ERR_STATE && bl >= 1 && br >= 0, "a singular coarse matrix");
    // a view that fails the structure check
    Csr u;
    u.row({{1, 1.0}, {0, 1.0}});
    u.row({{1, 1.0}});
    expect(run<double>(u, nullptr, &info, &bl, &br) == CVR_ERR_INVALID, "unsorted columns");
    if (failures) return 1;
    printf("amg_host_check: all cases ran clean\n");
    return 0;
}
