// cvr_amg.h -- what the two halves of the aggregation AMG preconditioner share (cvr_amg.hip: the object and its apply on the device;
// cvr_amg_host.cpp: the whole set-up -- option and structure checks, strength, aggregation, the Galerkin coarse operators, the smoother diagonals
// and the dense inverse of the coarsest level).  Plain C++: cvr_amg_host.cpp includes nothing of HIP, so that it links into a stand-alone host
// program that supplies fail() and check_csr() itself.  The arithmetic: include/cvr_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/cvr_amd.h"

namespace cvrh {

int fail(int code, const char *fmt, ...);                              // cvr_capi.hip: formats cvr_last_error, returns code
int check_csr(const cvr_csr_view *c, bool columns_on_host);            // cvr_capi.hip: cvr_create's checks of a view

namespace amg {

constexpr double kDblMax = 1.7976931348623157e308;

struct Level {
    int64_t              n = 0, nnz = 0, nc = 0;          // nc: the aggregates (the next level's n); 0 on the coarsest level
    std::vector<int64_t> rp;                              // n + 1
    std::vector<int32_t> ci;                              // nnz
    std::vector<uint8_t> va, dinv;                        // nnz and n values of T
    std::vector<int32_t> agg;                             // n, empty on the coarsest level
    std::vector<int64_t> mrp;                             // nc + 1: the aggregates' members ...
    std::vector<int32_t> mem;                             // ... n rows, ascending within an aggregate (the plain kind only)
    std::vector<int64_t> prp;                             // the smoothed kind above the coarsest level: P_l as a CSR of n x nc ...
    std::vector<int32_t> pci;
    std::vector<uint8_t> pva;                             // ... values of T
};

struct Hierarchy {
    cvr_amg_options      opt{};
    int32_t              is_f32 = 0, coarse_direct = 0, smoothed = 0;
    double               omega = 0;          // smoothed: as used
    std::vector<Level>   lv;
    std::vector<uint8_t> winv;          // coarse_direct: the n x n inverse of the coarsest matrix, row-major, values of T (symmetric bit for bit)
};

// cvr_amg_options as the header wants them; `entry` names the caller in the message
int check_options(const cvr_amg_options *opt, const char *entry);
// the structure rules of cvr_precond_fsai: the columns of every row strictly increasing, a diagonal entry in every row
int check_structure(int64_t n, const int64_t *rp, const int32_t *ci, const char *entry);
// The set-up from host arrays that passed both checks.  CVR_OK, CVR_ERR_NOMEM, or CVR_ERR_STATE with *bad_level / *bad_row = the level and its lowest
// row whose diagonal entry (or, on the coarsest level, pivot) is not finite or not > 0.
// coarsen: null for the plain kind (the sum of entries by aggregate pair); else the step from a level whose dinv, agg and nc are set to the next
// level's n and CSR -- the smoothed kind's, which also leaves the level's prolongator in prp, pci, pva.  Its error ends the set-up.
using Coarsen = std::function<int(Level &fine, Level &coarse, int32_t level)>;
int setup(Hierarchy &H, int64_t n, const int64_t *rp, const int32_t *ci, const void *va, int is_f32, const cvr_amg_options *opt, const char *entry, int32_t *bad_level,
          int64_t *bad_row, const Coarsen *coarsen = nullptr);
void fill_info(const Hierarchy &H, cvr_amg_info *info);
// cvr_precond_amg_export_level's copies, out of the hierarchy
int export_level(const Hierarchy &H, int32_t level, int64_t *row_ptr, int32_t *col_idx, void *vals, void *dinv, int32_t *agg, void *winv, const char *entry);


// ---- the smoothed kind (cvr_amg_smoothed_host.cpp; needs cvr_spgemm_host.cpp)
// omega as the header wants it: 0.0 -> 4/3 in *used
int check_omega(double omega, double *used, const char *entry);
// steps 1 - 5 of the header's set-up in host code, the products through cvr_spgemm_host
int smoothed_coarsen_host(Level &fine, Level &coarse, int is_f32, double omega);
int  products_per_apply(const Hierarchy &H);
void fill_smoothed_info(const Hierarchy &H, cvr_amg_smoothed_info *info);
int  export_prolongator(const Hierarchy &H, int32_t level, int64_t *row_ptr, int32_t *col_idx, void *vals, const char *entry);

}  // namespace amg
}  // namespace cvrh

struct cvr_amg_hierarchy {
    cvrh::amg::Hierarchy H;
};
