// color_host_check.cpp -- a stand-alone driver of the graph colouring's host twin (cvr_color_host.cpp) for `make color-asan-check`: the host code
// under AddressSanitizer and UBSan on n = 0 and 1, a path, a star, a clique of 70 rows inside a band (the first-fit mask leaves its first window
// of 64), a grid, a non-zero first row pointer, with color, perm and color_ptr written into exactly sized arrays, and on every error return.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "cvr_color.h"

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

int failures = 0;

void expect(bool ok, const char *what)
{
    if (!ok) {
        fprintf(stderr, "FAILED: %s (%s)\n", what, cvrh::g_msg);
        failures++;
    }
}

// a pattern from its pairs (the symmetric closure, a diagonal in every row), the arrays beginning at row_ptr[0] = shift
struct Pattern {
    std::vector<int64_t> rp;
    std::vector<int32_t> ci;
    Pattern(int n, const std::vector<std::pair<int, int>> &pairs, int64_t shift = 0)
    {
        std::vector<std::set<int>> rows((size_t)n);
        for (int i = 0; i < n; i++) rows[(size_t)i].insert(i);
        for (auto &p : pairs) {
            rows[(size_t)p.first].insert(p.second);
            rows[(size_t)p.second].insert(p.first);
        }
        ci.assign((size_t)shift, 0);
        rp.push_back(shift);
        for (auto &r : rows) {
            ci.insert(ci.end(), r.begin(), r.end());
            rp.push_back((int64_t)ci.size());
        }
    }
    cvr_csr_view view() const
    {
        cvr_csr_view v{};
        v.nrows = v.ncols = (int64_t)rp.size() - 1;
        v.row_ptr = rp.data();
        v.col_idx = ci.data();
        return v;          // vals stays null: the colouring does not read it
    }
};

// the colouring into exactly sized arrays, held to its properties; returns ncolors
int colour(const Pattern &m, int32_t *rounds_out = nullptr)
{
    const cvr_csr_view   v = m.view();
    const size_t         n = (size_t)v.nrows;
    std::vector<int32_t> color(n, -7), perm(n, -7), ptr(n + 1, -7);
    int32_t              nc = -1, rounds = -1;
    expect(cvr_color_host(&v, n ? color.data() : nullptr, n ? perm.data() : nullptr, ptr.data(), &nc, &rounds) == CVR_OK, "cvr_color_host");
    std::vector<int> used((size_t)std::max(nc, 0), 0);
    for (size_t i = 0; i < n; i++) {
        expect(color[i] >= 0 && color[i] < nc, "every row has a colour below ncolors");
        if (color[i] >= 0 && color[i] < nc) used[(size_t)color[i]] = 1;
        for (int64_t q = m.rp[i]; q < m.rp[i + 1]; q++) expect(m.ci[(size_t)q] == (int32_t)i || color[(size_t)m.ci[(size_t)q]] != color[i], "no two neighbours share a colour");
        expect(color[i] <= (int32_t)(m.rp[i + 1] - m.rp[i] - 1), "a row's colour is at most its degree");
    }
    for (int u : used) expect(u == 1, "every colour is used");
    expect(ptr[0] == 0 && ptr[(size_t)nc] == (int32_t)n, "color_ptr spans the rows");
    for (int32_t c = 0; c < nc; c++)
        for (int32_t k = ptr[(size_t)c]; k < ptr[(size_t)c + 1]; k++)
            expect(color[(size_t)perm[(size_t)k]] == c && (k == ptr[(size_t)c] || perm[(size_t)k - 1] < perm[(size_t)k]), "perm is ordered by (colour, row)");
    expect(rounds >= (n ? 1 : 0) && rounds <= (int32_t)n, "rounds");
    if (rounds_out) *rounds_out = rounds;
    return nc;
}

}  // namespace

int main()
{
    expect(colour(Pattern(0, {})) == 0, "n = 0: no colour");
    expect(colour(Pattern(1, {})) == 1, "n = 1: one colour");
    std::vector<std::pair<int, int>> path, star, clique, grid;
    for (int i = 0; i + 1 < 1000; i++) path.push_back({i, i + 1});
    const int np = colour(Pattern(1000, path));
    expect(np >= 2 && np <= 3, "a path takes 2 or 3 colours");
    expect(colour(Pattern(1000, path, 17)) == np, "a non-zero first row pointer changes nothing");
    for (int j = 1; j < 500; j++) star.push_back({0, j});
    expect(colour(Pattern(500, star)) == 2, "a star takes 2 colours");
    for (int i = 0; i + 1 < 300; i++) clique.push_back({i, i + 1});
    for (int a = 0; a < 70; a++)
        for (int b = a + 1; b < 70; b++) clique.push_back({40 + 3 * a, 40 + 3 * b});
    int32_t rounds = 0;
    expect(colour(Pattern(300, clique), &rounds) >= 70 && rounds >= 70, "a clique of 70 takes 70 colours in 70 rounds");
    for (int i = 0; i < 40; i++)
        for (int j = 0; j < 40; j++) {
            if (j + 1 < 40) grid.push_back({i * 40 + j, i * 40 + j + 1});
            if (i + 1 < 40) grid.push_back({i * 40 + j, (i + 1) * 40 + j});
        }
    expect(colour(Pattern(1600, grid)) <= 5, "a 5-point grid takes at most 5 colours");

    // every error return
    const Pattern        ok(4, {{0, 1}, {1, 2}, {2, 3}});
    cvr_csr_view         v = ok.view();
    std::vector<int32_t> color(4), perm(4), ptr(5);
    int32_t              nc = 0, rounds2 = 0;
    expect(cvr_color_host(nullptr, color.data(), perm.data(), ptr.data(), &nc, &rounds2) == CVR_ERR_INVALID, "null view");
    expect(cvr_color_host(&v, nullptr, perm.data(), ptr.data(), &nc, &rounds2) == CVR_ERR_INVALID, "null color");
    expect(cvr_color_host(&v, color.data(), nullptr, ptr.data(), &nc, &rounds2) == CVR_ERR_INVALID, "null perm");
    expect(cvr_color_host(&v, color.data(), perm.data(), nullptr, &nc, &rounds2) == CVR_ERR_INVALID, "null color_ptr");
    expect(cvr_color_host(&v, color.data(), perm.data(), ptr.data(), nullptr, &rounds2) == CVR_ERR_INVALID, "null ncolors");
    expect(cvr_color_host(&v, color.data(), perm.data(), ptr.data(), &nc, nullptr) == CVR_ERR_INVALID, "null rounds");
    v.ncols = 5;
    expect(cvr_color_host(&v, color.data(), perm.data(), ptr.data(), &nc, &rounds2) == CVR_ERR_INVALID, "not square");
    v = ok.view();
    v.arrays_on_device = 1;
    expect(cvr_color_host(&v, color.data(), perm.data(), ptr.data(), &nc, &rounds2) == CVR_ERR_INVALID, "device arrays");
    const std::vector<int64_t> rp{0, 2, 5, 7};
    std::vector<int32_t>       unsorted{0, 1, 1, 0, 2, 1, 2}, nodiag{0, 1, 0, 2, 2, 1, 2}, asym{0, 2, 0, 1, 2, 1, 2};
    cvr_csr_view               w{};
    w.nrows = w.ncols = 3;
    w.row_ptr = rp.data();
    w.col_idx = unsorted.data();
    expect(cvr_color_host(&w, color.data(), perm.data(), ptr.data(), &nc, &rounds2) == CVR_ERR_INVALID, "an unsorted row");
    w.col_idx = nodiag.data();
    expect(cvr_color_host(&w, color.data(), perm.data(), ptr.data(), &nc, &rounds2) == CVR_ERR_INVALID, "a missing diagonal");
    w.col_idx = asym.data();          // (0, 2) without (2, 0)
    expect(cvr_color_host(&w, color.data(), perm.data(), ptr.data(), &nc, &rounds2) == CVR_ERR_INVALID && nc == 0 && rounds2 == 0, "an asymmetric pattern");
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("color_host_check: ok\n");
    return 0;
}
