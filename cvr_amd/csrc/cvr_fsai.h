// cvr_fsai.h -- what the two halves of the FSAI preconditioner share (cvr_fsai.hip: the device set-up, the object and its apply; cvr_fsai_host.cpp: the
// structure checks, the row patterns and the host twin of the factorisation).  Plain C++: cvr_fsai_host.cpp includes nothing of HIP, so that it links
// into a stand-alone host program that supplies fail() and check_csr() itself.  The arithmetic both halves implement: include/cvr_amd.h.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/cvr_amd.h"

namespace cvrh {

int fail(int code, const char *fmt, ...);                              // cvr_capi.hip: formats cvr_last_error, returns code
int check_csr(const cvr_csr_view *c, bool columns_on_host);            // cvr_capi.hip: cvr_create's checks of a view

namespace fsai {

constexpr int    kMaxRow = CVR_FSAI_MAX_ROW;          // entries of a row of W at most
constexpr int    kLd = kMaxRow + 1;                   // the pitch of a row of the small matrix S, in doubles: rows fall on different LDS banks
constexpr double kDblMax = 1.7976931348623157e308;

struct Pattern {
    int32_t max_row = 0;                     // the largest m
    int64_t truncated = 0, nnz = 0;          // rows with more than kMaxRow columns <= i; nnz of W
};

// The structure checks of cvr_precond_ilu0 (columns strictly increasing, a diagonal in every row; `entry` names the caller in the message) and the
// pattern of W: wrp[n + 1] = W's row_ptr from 0, src[n] = where in A's arrays the first kept entry of row i lies (its m = wrp[i + 1] - wrp[i] kept
// entries are src[i] .. src[i] + m - 1, the last of them the diagonal).  O(nnz).
int pattern(int64_t n, const int64_t *rp, const int32_t *ci, const char *entry, int64_t *wrp, int64_t *src, Pattern *out);

// G: the power of two from the largest m up, 4 .. 64
inline int32_t lanes_of(int32_t max_row)
{
    int32_t G = 4;
    while (G < max_row && G < 64) G <<= 1;
    return G;
}

// A pivot the factorisation accepts: finite and > 0
inline bool pivot_ok(double d) { return d > 0 && d <= kDblMax; }

}  // namespace fsai
}  // namespace cvrh
