// cvr_spgemm.h -- what the two halves of the sparse matrix-matrix product C = A B share (cvr_spgemm.hip: the object and its kernels on the device;
// cvr_spgemm_host.cpp: the pure-host twin with the same checks and the same bits).  Plain C++: cvr_spgemm_host.cpp includes nothing of HIP, so that
// it links into a stand-alone host program that supplies fail() itself.  The contract: include/cvr_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/cvr_amd.h"

namespace cvrh {

int fail(int code, const char *fmt, ...);                              // cvr_capi.hip: formats cvr_last_error, returns code

namespace spgemm {

// The row classes by products[i] = the sum over A's row i of nnz(B row col_A[p]):
//   0                                    empty: nothing is launched for the row
//   1 .. kGroupLimit - 1                 group: kLanes lanes of a wavefront, a table of kGroupSlots slots in LDS
//   kGroupLimit .. kBlockLimit - 1       block: a workgroup, a table of up to kBlockSlots slots in LDS
//   kBlockLimit ..                       spill: a workgroup, a table in the global arena
// A table has at least twice as many slots as the row has products, so it is never more than half full.
constexpr int64_t kGroupLimit = 32, kBlockLimit = 4096;
constexpr int32_t kLanes = 8, kGroupSlots = 64, kBlockSlots = 8192;

// what both entry points ask of the two views before they look at an array; `entry` names the caller in the message
int check_pair(const cvr_csr_view *a, const cvr_csr_view *b, const char *entry);
// A view of host arrays checked as cvr_create checks a CSR -- sizes, row_ptr[0] >= 0 and no decrease, col_idx and vals present, every column in
// [0, ncols), ncols < 2^31 - 1 -- without cvr_create's limit that a vector x of ncols values fit a buffer descriptor: the product has no x.  This is the
// check of both entry points, so the sanitizer run of the host twin exercises the very code the library runs.
int check_view(const cvr_csr_view *c);
// B's rows strictly ascending in column (host arrays): the first offending row, or -1
int64_t first_unsorted_row(int64_t nrows, const int64_t *rp, const int32_t *ci);
int fail_unsorted(const char *entry, int64_t row);

}  // namespace spgemm
}  // namespace cvrh
