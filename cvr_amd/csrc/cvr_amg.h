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
    int64_t              pnnz = 0;                        // ... its entries (set where the arrays above stay on the device until an export asks)
};

struct Hierarchy {
    cvr_amg_options      opt{};
    int32_t              is_f32 = 0, coarse_direct = 0, smoothed = 0;
    double               omega = 0;          // smoothed: as used
    int32_t              mis2 = 0;           // the aggregation was MIS(2) ...
    int32_t              rounds[CVR_AMG_MAX_LEVELS] = {};          // ... in this many rounds on every level that was coarsened
    std::vector<Level>   lv;
    std::vector<uint8_t> winv;          // coarse_direct: the n x n inverse of the coarsest matrix, row-major, values of T (symmetric bit for bit)
};

// cvr_amg_options as the header wants them; `entry` names the caller in the message
int check_options(const cvr_amg_options *opt, const char *entry);
// the structure rules of cvr_precond_fsai: the columns of every row strictly increasing, a diagonal entry in every row.  row0: the number of the
// first of the n rows (a caller that found the offending row elsewhere passes that row alone for the message)
int check_structure(int64_t n, const int64_t *rp, const int32_t *ci, const char *entry, int64_t row0 = 0);
// The set-up from host arrays that passed both checks.  CVR_OK, CVR_ERR_NOMEM, or CVR_ERR_STATE with *bad_level / *bad_row = the level and its lowest
// row whose diagonal entry (or, on the coarsest level, pivot) is not finite or not > 0.
// coarsen: null for the plain kind (the sum of entries by aggregate pair); else the step from a level whose dinv, agg and nc are set to the next
// level's n and CSR -- the smoothed kind's, which also leaves the level's prolongator in prp, pci, pva.  Its error ends the set-up.
// aggregation: the three serial passes, or MIS(2) in parallel rounds (cvr_amg_mis2_host.cpp), which also sets H.mis2 and H.rounds.
using Coarsen = std::function<int(Level &fine, Level &coarse, int32_t level)>;
enum class Aggregation { kSerial, kMis2 };
int setup(Hierarchy &H, int64_t n, const int64_t *rp, const int32_t *ci, const void *va, int is_f32, const cvr_amg_options *opt, const char *entry, int32_t *bad_level,
          int64_t *bad_row, const Coarsen *coarsen = nullptr, Aggregation aggregation = Aggregation::kSerial);
// the explicit inverse of a coarsest level of at most CVR_AMG_MAX_COARSE rows (rp, ci, va set) into winv; the pivot that is not finite or not > 0, or -1
int64_t coarsest_inverse(const Level &l, int is_f32, std::vector<uint8_t> &winv);
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

// ---- the MIS(2) aggregation (cvr_amg_mis2_host.cpp)
// murmur3's 32-bit finaliser and the key of a row in a state (1 undecided, 2 root, 0 out): what the host loops and the device kernels share
constexpr uint64_t kMis2Undecided = 1, kMis2Root = 2, kMis2Out = 0;
#if defined(__HIPCC__)
#define CVR_AMG_BOTH __host__ __device__
#else
#define CVR_AMG_BOTH
#endif
CVR_AMG_BOTH inline uint32_t mis2_hash(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}
CVR_AMG_BOTH inline uint64_t mis2_key(uint64_t state, uint32_t i) { return (state << 62) | ((uint64_t)(mis2_hash(i) >> 1) << 31) | (uint64_t)i; }
// agg[n] of a CSR that passed check_structure (rp indexes ci and va as it stands: rp[0] need not be 0); returns the number of aggregates
int64_t mis2_aggregate(int64_t n, const int64_t *rp, const int32_t *ci, const void *va, int is_f32, double strength, int32_t *agg, int32_t *rounds);
void    fill_mis2_info(const Hierarchy &H, cvr_amg_mis2_info *info);

}  // namespace amg
}  // namespace cvrh

struct cvr_amg_hierarchy {
    cvrh::amg::Hierarchy H;
};
