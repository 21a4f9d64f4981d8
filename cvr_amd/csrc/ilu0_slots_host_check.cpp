// ilu0_slots_host_check.cpp -- a stand-alone driver of the Jacobi-swept ILU(0) apply's row-ordered slot builder (cvr_ilu0_slots.h) for
// `make ilu0-slots-asan-check`: the host code under AddressSanitizer and UBSan on n = 0 and 1, a diagonal matrix, a 5-point grid, a matrix with a row
// of 200 lower entries and a non-zero first row pointer, rp and dpos in exactly sized arrays, every slot held to the row it names.
#include <cstdio>
#include <utility>
#include <vector>

#include "cvr_ilu0_slots.h"

using cvrh::krylov::Ilu0Slot;
using cvrh::krylov::ilu0_row_slots;

namespace {

int failures = 0;

void expect(bool ok, const char *what)
{
    if (!ok) {
        fprintf(stderr, "FAILED: %s\n", what);
        failures++;
    }
}

// rows[i]: the ascending off-diagonal columns of row i; the arrays begin at row_ptr[0] = shift
struct Pattern {
    std::vector<int64_t> rp, dpos;
    std::vector<int32_t> ci;
    Pattern(const std::vector<std::vector<int>> &rows, int64_t shift = 0)
    {
        ci.assign((size_t)shift, -1);
        rp.push_back(shift);
        for (size_t i = 0; i < rows.size(); i++) {
            bool placed = false;
            for (int c : rows[i]) {
                if (!placed && c > (int)i) {
                    dpos.push_back((int64_t)ci.size());
                    ci.push_back((int32_t)i);
                    placed = true;
                }
                ci.push_back(c);
            }
            if (!placed) {
                dpos.push_back((int64_t)ci.size());
                ci.push_back((int32_t)i);
            }
            rp.push_back((int64_t)ci.size());
        }
    }
};

// both triangles' slots: slot i names row i, its entries are exactly the row's columns on that side of the diagonal, and the diagonal lies where
// the kernels look for it (L: at beg + cnt, U: at beg - 1)
void check(const Pattern &m, const char *what)
{
    const int64_t         n = (int64_t)m.rp.size() - 1;
    std::vector<Ilu0Slot> lo(3), up;          // (lo: resized down or up)
    ilu0_row_slots(n, m.rp.data(), m.dpos.data(), false, lo);
    ilu0_row_slots(n, m.rp.data(), m.dpos.data(), true, up);
    expect((int64_t)lo.size() == n && (int64_t)up.size() == n, what);
    long long entries = 0;
    for (int64_t i = 0; i < n; i++) {
        const Ilu0Slot &a = lo[(size_t)i], &b = up[(size_t)i];
        expect(a.row == i && b.row == i, what);
        expect(a.beg == m.rp[(size_t)i] && a.beg + a.cnt == m.dpos[(size_t)i] && m.ci[(size_t)(a.beg + a.cnt)] == i, what);
        expect(b.beg - 1 == m.dpos[(size_t)i] && b.beg + b.cnt == m.rp[(size_t)i + 1] && m.ci[(size_t)(b.beg - 1)] == i, what);
        for (int e = 0; e < a.cnt; e++) expect(m.ci[(size_t)(a.beg + e)] < i, what);
        for (int e = 0; e < b.cnt; e++) expect(m.ci[(size_t)(b.beg + e)] > i, what);
        entries += a.cnt + b.cnt + 1;
    }
    expect(entries == (long long)(m.rp.back() - m.rp.front()), what);
}

}  // namespace

int main()
{
    check(Pattern(std::vector<std::vector<int>>(0)), "n = 0");
    check(Pattern(std::vector<std::vector<int>>(1)), "n = 1");
    check(Pattern(std::vector<std::vector<int>>(7)), "a diagonal matrix");
    std::vector<std::vector<int>> grid(40 * 40), wide(300);
    for (int i = 0; i < 40; i++)
        for (int j = 0; j < 40; j++) {
            std::vector<int> &r = grid[(size_t)(i * 40 + j)];
            if (i > 0) r.push_back((i - 1) * 40 + j);
            if (j > 0) r.push_back(i * 40 + j - 1);
            if (j + 1 < 40) r.push_back(i * 40 + j + 1);
            if (i + 1 < 40) r.push_back((i + 1) * 40 + j);
        }
    check(Pattern(grid), "a 5-point grid");
    check(Pattern(grid, 17), "a non-zero first row pointer");
    for (int c = 0; c < 200; c++) wide[250].push_back(c);          // a row of 200 lower entries ...
    for (int c = 1; c < 300; c += 2) wide[0].push_back(c);         // ... and a row of 150 upper ones
    check(Pattern(wide), "long rows");
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("ilu0_slots_host_check: ok\n");
    return 0;
}
