// cvr_ilu0_slots.h -- what a sweep kernel of the ILU(0) kind reads per row (cvr_ilu0.hip), and the slot array in natural row order that the
// Jacobi-swept apply (cvr_precond_ilu0_jacobi) walks.  Pure host code, no HIP: `make ilu0-slots-asan-check` runs it under the host sanitizers.
#pragma once
#include <cstdint>
#include <vector>

namespace cvrh {
namespace krylov {

// a row in a sweep's order: its entries of the sweep's triangle are beg .. beg + cnt - 1 (U: the diagonal lies at beg - 1, L: at beg + cnt)
struct Ilu0Slot {
    long long beg;
    int32_t   cnt, row;
};
static_assert(sizeof(Ilu0Slot) == 16, "one 16-byte load per row");

// slots[i] = row i's part of the triangle, i = 0 .. n - 1: left of the diagonal (upper = false) or right of it.  rp: n + 1 row pointers, dpos: where
// each row's diagonal lies, rp[i] <= dpos[i] < rp[i + 1].
inline void ilu0_row_slots(int64_t n, const int64_t *rp, const int64_t *dpos, bool upper, std::vector<Ilu0Slot> &slots)
{
    slots.resize((size_t)(n > 0 ? n : 0));
    for (int64_t i = 0; i < n; i++) {
        if (upper) slots[(size_t)i] = {dpos[i] + 1, (int32_t)(rp[i + 1] - dpos[i] - 1), (int32_t)i};
        else slots[(size_t)i] = {rp[i], (int32_t)(dpos[i] - rp[i]), (int32_t)i};
    }
}

}  // namespace krylov
}  // namespace cvrh
