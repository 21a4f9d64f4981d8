// cvr_amg_mis2.h -- what cvr_precond_amg_mis2's level loop (cvr_amg.hip) calls per level, defined in cvr_amg_mis2.hip.  Every call enqueues on `st`
// and returns with it idle, having waited for a scalar.  `entry`: the name the messages begin with.
#pragma once
#include "cvr_precond.h"

namespace cvrh {
namespace krylov {

// the structure rules on a view of device arrays behind check_device_view (rp_host: its copy of the row pointers): amg::check_structure's error,
// naming the lowest offending row
CVR_HIDDEN int mis2_check_structure_device(const char *entry, const cvr_csr_view &device_view, const std::vector<int64_t> &rp_host, hipStream_t st);
// d_diag[n] = the diagonal as doubles, d_dinv[n] (values of the view's type; may be null) = the smoother diagonal's inverse; *bad_row = the lowest
// row whose diagonal entry is not finite or not > 0, or -1
CVR_HIDDEN int mis2_diagonal_device(const char *entry, const cvr_csr_view &device_view, void *d_dinv, double *d_diag, int64_t *bad_row, hipStream_t st);
// d_agg[n], *nc and *rounds of the MIS(2) aggregation; [j0, j1) = row_ptr[0], row_ptr[nrows]
CVR_HIDDEN int mis2_aggregate_device(const char *entry, const cvr_csr_view &device_view, int64_t j0, int64_t j1, const double *d_diag, double strength, int32_t *d_agg, int64_t *nc,
                                     int32_t *rounds, hipStream_t st);

}  // namespace krylov
}  // namespace cvrh
