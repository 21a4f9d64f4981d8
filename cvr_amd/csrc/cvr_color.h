// cvr_color.h -- what the two halves of the graph colouring share (cvr_color_host.cpp: the pattern rules and the rounds as host loops;
// cvr_color.hip: the same with a thread per row) and what the multicolour SGS preconditioner (cvr_mcsgs.hip) calls.  Plain C++ but for the
// device half's declarations: cvr_color_host.cpp includes nothing of HIP, so that it links into a stand-alone host program that supplies fail()
// and check_csr() itself.  The definition: include/cvr_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/cvr_amd.h"
#include "cvr_amg.h"          // fail, check_csr and amg::mis2_hash: murmur3's finaliser, the one function both keys use

namespace cvrh {
namespace color {

constexpr int32_t kUncoloured = -1;          // a row's word until a round colours it; else its colour

// key(i) = (h(i) >> 1) << 31 | i: no seed, no level
CVR_AMG_BOTH inline uint64_t key(uint32_t i) { return ((uint64_t)(amg::mis2_hash(i) >> 1) << 31) | (uint64_t)i; }

// what both entry points check of the view before they read an array: square, 0 <= n < 2^31
int check_view(const cvr_csr_view *csr, const char *entry);
// cvr_precond_ilu0's structure rules on host arrays (the columns of every row strictly increasing, a diagonal entry in every row), with its texts;
// row0: the number of the first of the n rows (a caller that found the offending row elsewhere passes that row alone for the message)
int check_structure(int64_t n, const int64_t *rp, const int32_t *ci, const char *entry, int64_t row0 = 0);
// the symmetry rule on host arrays that passed check_structure: every stored (i, j), j != i, has a stored (j, i)
int check_symmetric(int64_t n, const int64_t *rp, const int32_t *ci, const char *entry);
// the message of the rule, for both halves
int fail_asymmetric(const char *entry, int64_t row, int64_t col);
// The rounds on host arrays that passed the rules.  color[n]; perm[n] and color_ptr[n + 1 at least] may be null together.  rp indexes ci as it
// stands (rp[0] need not be 0).
void color_host(int64_t n, const int64_t *rp, const int32_t *ci, int32_t *color, int32_t *perm, int32_t *color_ptr, int32_t *ncolors, int32_t *rounds);

}  // namespace color
}  // namespace cvrh

#if defined(__HIPCC__)
#include "cvr_precond.h"

namespace cvrh {
namespace krylov {

// A view of host or device arrays as a view of device arrays, checked as cvr_create checks one: device arrays stay where they are (dv = *c), host
// arrays are copied into `s` (col_idx and, with_values, vals in the places row_ptr names).  *rp_host: the row pointers on the host (the caller's, or
// the copy in rp_own).  vals may be null without with_values.
CVR_HIDDEN int stage_device(const char *entry, const cvr_csr_view *c, bool with_values, Scratch &s, cvr_csr_view *dv, std::vector<int64_t> &rp_own, const int64_t **rp_host,
                            hipStream_t st);
// The colouring of a view that stage_device made, n > 0: the pattern rules (one read-back of the two bad-row words), the rounds (the counters every
// color_check rounds), the order.  d_color and d_perm: n words each on the device; color_ptr: ncolors + 1 offsets on the host.
CVR_HIDDEN int color_device(const char *entry, const cvr_csr_view &dv, const int64_t *rp_host, int32_t *d_color, int32_t *d_perm, std::vector<int32_t> &color_ptr, int32_t *ncolors,
                            int32_t *rounds, hipStream_t st);

}  // namespace krylov
}  // namespace cvrh
#endif
