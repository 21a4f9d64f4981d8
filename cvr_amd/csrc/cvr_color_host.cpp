// cvr_color_host.cpp -- the host half of the graph colouring (include/cvr_amd.h: cvr_color_host): the pattern rules and the rounds on hashed
// keys as loops over the rows, every round reading the state before it only (two arrays in turn) -- what the kernels of cvr_color.hip do with a
// thread per row -- and the rows ordered by (colour, row).  No HIP: it links into a stand-alone host program that supplies fail() and check_csr().
#include "cvr_color.h"

#include <algorithm>
#include <new>

namespace cvrh {
namespace color {

int check_view(const cvr_csr_view *csr, const char *entry)
{
    if (csr->nrows != csr->ncols) return fail(CVR_ERR_INVALID, "%s: the colouring needs a square matrix (%lld x %lld)", entry, (long long)csr->nrows, (long long)csr->ncols);
    if (csr->nrows < 0) return fail(CVR_ERR_INVALID, "null or negative-size CSR view");
    if (csr->nrows > (int64_t)0x7fffffff) return fail(CVR_ERR_INVALID, "%s: nrows (%lld) must stay below 2^31", entry, (long long)csr->nrows);
    return CVR_OK;
}

int check_structure(int64_t n, const int64_t *rp, const int32_t *ci, const char *entry, int64_t row0)
{
    for (int64_t i = 0; i < n; i++) {
        int64_t d = -1, prev = -1;
        for (int64_t q = rp[i]; q < rp[i + 1]; q++) {
            const int64_t c = ci[q];
            if (c <= prev) return fail(CVR_ERR_INVALID, "%s: row %lld: the columns are not strictly increasing (%lld behind %lld)", entry, (long long)(row0 + i), (long long)c, (long long)prev);
            prev = c;
            if (c == row0 + i) d = q;
        }
        if (d < 0) return fail(CVR_ERR_INVALID, "%s: row %lld has no diagonal entry", entry, (long long)(row0 + i));
    }
    return CVR_OK;
}

int fail_asymmetric(const char *entry, int64_t row, int64_t col)
{
    return fail(CVR_ERR_INVALID, "%s: row %lld has an entry in column %lld, row %lld none in column %lld: the off-diagonal pattern must be structurally symmetric", entry,
                (long long)row, (long long)col, (long long)col, (long long)row);
}

int check_symmetric(int64_t n, const int64_t *rp, const int32_t *ci, const char *entry)
{
    for (int64_t i = 0; i < n; i++)
        for (int64_t q = rp[i]; q < rp[i + 1]; q++) {
            const int64_t j = ci[q];
            if (j != i && !std::binary_search(ci + rp[j], ci + rp[j + 1], (int32_t)i)) return fail_asymmetric(entry, i, j);
        }
    return CVR_OK;
}

void color_host(int64_t n, const int64_t *rp, const int32_t *ci, int32_t *color, int32_t *perm, int32_t *color_ptr, int32_t *ncolors, int32_t *rounds)
{
    *ncolors = 0;
    *rounds = 0;
    if (n == 0) {
        if (color_ptr) color_ptr[0] = 0;
        return;
    }
    std::vector<int32_t> a((size_t)n, kUncoloured), b((size_t)n, kUncoloured);
    int32_t             *in = a.data(), *out = b.data();
    int32_t              top = -1;
    for (int64_t uncoloured = n; uncoloured > 0;) {
        ++*rounds;
        uncoloured = 0;
        for (int64_t i = 0; i < n; i++) {
            if (in[i] != kUncoloured) {
                out[i] = in[i];
                continue;
            }
            const uint64_t k = key((uint32_t)i);
            bool           first = true;
            for (int64_t q = rp[i]; q < rp[i + 1] && first; q++) {
                const int32_t j = ci[q];
                first = j == i || in[j] != kUncoloured || key((uint32_t)j) < k;
            }
            if (!first) {
                out[i] = kUncoloured;
                uncoloured++;
                continue;
            }
            // first fit: the neighbours' colours in the window [base, base + 64) as a mask; a full window moves on by 64
            int32_t c = -1;
            for (int32_t base = 0; c < 0; base += 64) {
                uint64_t mask = 0;
                for (int64_t q = rp[i]; q < rp[i + 1]; q++) {
                    const int32_t j = ci[q], cj = in[j];
                    if (j != i && cj >= base && cj < base + 64) mask |= 1ull << (cj - base);
                }
                if (~mask) c = base + __builtin_ctzll(~mask);
            }
            out[i] = c;
            top = std::max(top, c);
        }
        std::swap(in, out);
    }
    *ncolors = top + 1;
    for (int64_t i = 0; i < n; i++) color[i] = in[i];
    if (!perm || !color_ptr) return;
    std::fill(color_ptr, color_ptr + *ncolors + 1, 0);
    for (int64_t i = 0; i < n; i++) color_ptr[in[i] + 1]++;
    for (int32_t c = 0; c < *ncolors; c++) color_ptr[c + 1] += color_ptr[c];
    std::vector<int32_t> at(color_ptr, color_ptr + *ncolors);
    for (int64_t i = 0; i < n; i++) perm[at[(size_t)in[i]]++] = (int32_t)i;          // ascending rows within a colour
}

}  // namespace color
}  // namespace cvrh

using namespace cvrh;

extern "C" {

int cvr_color_host(const cvr_csr_view *csr, int32_t *color, int32_t *perm, int32_t *color_ptr, int32_t *ncolors, int32_t *rounds)
{
    const char *entry = "cvr_color_host";
    if (!csr || !ncolors || !rounds || !color_ptr) return fail(CVR_ERR_INVALID, "null argument");
    *ncolors = 0;
    *rounds = 0;
    if (csr->arrays_on_device) return fail(CVR_ERR_INVALID, "%s: the arrays must be host arrays", entry);
    if (const int rc = color::check_view(csr, entry)) return rc;
    if (csr->nrows > 0 && (!color || !perm)) return fail(CVR_ERR_INVALID, "null argument");
    cvr_csr_view v = *csr;
    if (!v.vals) v.vals = v.col_idx;          // (not read here)
    if (const int rc = check_csr(&v, true)) return rc;
    if (const int rc = color::check_structure(csr->nrows, csr->row_ptr, csr->col_idx, entry)) return rc;
    if (const int rc = color::check_symmetric(csr->nrows, csr->row_ptr, csr->col_idx, entry)) return rc;
    try {
        color::color_host(csr->nrows, csr->row_ptr, csr->col_idx, color, perm, color_ptr, ncolors, rounds);
    } catch (const std::bad_alloc &) {
        return fail(CVR_ERR_NOMEM, "%s: out of host memory (%lld rows)", entry, (long long)csr->nrows);
    }
    return CVR_OK;
}

}  // extern "C"
