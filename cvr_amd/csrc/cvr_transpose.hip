// cvr_transpose.hip -- the CSR of A^T on the device, for cvr_options.transpose (include/cvr_amd.h).
//
// T = the CSR of A^T: row j holds A's elements of column j in ascending CSR position (ascending row of A, duplicates in their order),
// its column index is A's row.  That is a STABLE sort of A's positions by column: one hipCUB radix sort of (column, position) pairs --
// LSD radix sort keeps the input order of equal keys, so T is the same bit for bit on every run, no order depends on atomics --, then
//   transpose_rows_kernel    T's row pointers: rp_t[c] = the number of sorted keys below c (lower bound, one thread per column of A);
//   transpose_gather_kernel  per element of T: A's row of the position (binary search in A's row_ptr, as cvr_split.hip does) and its
//                            value -- or, for mutable handles, the position itself (its bits + 1 stand in for the value, cvr_update.hip),
//                            so that the handle's map points into A's CSR positions.
// The result is an ordinary device CSR with row_ptr[0] = 0: cvr_create goes on with it as with any arrays_on_device input.
#include "cvr_internal.h"

#include <hipcub/hipcub.hpp>

using namespace cvrh;

namespace cvr {
namespace {

__global__ __launch_bounds__(256) void transpose_iota_kernel(uint32_t *__restrict__ pos, long long j0, long long n)
{
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) pos[t] = (uint32_t)(j0 + t);
}

// rp_t[c] = first t with key[t] >= c, c = 0 .. ncols (keys sorted ascending, all < ncols: rp_t[ncols] = n)
__global__ __launch_bounds__(256) void transpose_rows_kernel(const uint32_t *__restrict__ key, long long n, long long ncols, long long *__restrict__ rp_t)
{
    for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c <= ncols; c += (long long)gridDim.x * 256) {
        long long lo = 0, hi = n;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if ((long long)key[mid] < c) lo = mid + 1; else hi = mid;
        }
        rp_t[c] = lo;
    }
}

// B: the bits of the value type (values are moved, never interpreted); POS: write position + 1 instead of the value
template <typename B, bool POS>
__global__ __launch_bounds__(256) void transpose_gather_kernel(const long long *__restrict__ rp, long long nrows, const uint32_t *__restrict__ pos,
                                                               const B *__restrict__ va, long long va_shift, long long n, int32_t *__restrict__ ci_t,
                                                               B *__restrict__ va_t)
{
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
        const long long j = (long long)pos[t];
        long long lo = 0, hi = nrows;                       // last r with rp[r] <= j (then rp[r+1] > j: rp[0] <= j < rp[nrows])
        while (lo < hi) {
            const long long mid = (lo + hi + 1) >> 1;
            if (rp[mid] <= j) lo = mid; else hi = mid - 1;
        }
        ci_t[t] = (int32_t)lo;
        va_t[t] = POS ? (B)(j + 1) : va[j - va_shift];
    }
}

uint32_t grid_of(long long n) { return (uint32_t)std::min<long long>(8192, std::max<long long>(1, (n + 255) / 256)); }

template <typename B>
void launch_gather(bool positions, const long long *rp, long long nrows, const uint32_t *pos, const void *va, long long va_shift, long long n, int32_t *ci_t, void *va_t,
                   hipStream_t st)
{
    if (positions)
        hipLaunchKernelGGL((transpose_gather_kernel<B, true>), dim3(grid_of(n)), dim3(256), 0, st, rp, nrows, pos, static_cast<const B *>(va), va_shift, n, ci_t,
                           static_cast<B *>(va_t));
    else
        hipLaunchKernelGGL((transpose_gather_kernel<B, false>), dim3(grid_of(n)), dim3(256), 0, st, rp, nrows, pos, static_cast<const B *>(va), va_shift, n, ci_t,
                           static_cast<B *>(va_t));
}

}  // namespace
}  // namespace cvr

namespace cvrh {

void TransposedCsr::release()
{
    if (arena) (void)hipFree(arena);
    *this = TransposedCsr();
}

int transpose_csr(const cvr_csr_view &a, int64_t j0, int64_t j1, bool positions, hipStream_t st, TransposedCsr *out)
{
    out->release();
    const long long n = j1 - j0, nr = a.nrows, nc = a.ncols;
    if (n < 0 || j1 >= (1ll << 32) || nr >= 0x7fffffffll) return fail(CVR_ERR_INVALID, "transpose: the CSR is beyond 32-bit positions or row indices");
    const bool   f32 = a.is_f32 != 0, host = a.arrays_on_device == 0;
    const size_t vsz = f32 ? 4 : 8, nn = (size_t)std::max<long long>(n, 1);
    int          bits = 1;
    while (bits < 32 && (1ll << bits) < nc) bits++;
    size_t sort_bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                               (unsigned int)nn, 0, bits, st));
    // one allocation: T (row pointers, columns -- the sorted keys until the gather overwrites them --, values), the positions before and after
    // the sort, the sort's work space and, for host arrays, A's upload (row pointers, columns, values of [j0, j1))
    auto         up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_rp = 0, o_ci = o_rp + up(8 * ((size_t)nc + 1)), o_va = o_ci + up(4 * nn), o_pin = o_va + up(vsz * nn), o_pos = o_pin + up(4 * nn),
                 o_work = o_pos + up(4 * nn), o_arp = o_work + up(std::max<size_t>(sort_bytes, 16)), o_aci = o_arp + (host ? up(8 * ((size_t)nr + 1)) : 0),
                 o_ava = o_aci + (host ? up(4 * nn) : 0), total = o_ava + (host && !positions ? up(vsz * nn) : 0);
    void *arena = nullptr;
    HIP_TRY(hipMalloc(&arena, total));
    uint8_t *m = static_cast<uint8_t *>(arena);
    out->arena = arena;
    out->rp = reinterpret_cast<int64_t *>(m + o_rp);
    out->ci = reinterpret_cast<int32_t *>(m + o_ci);
    out->va = m + o_va;
    out->nrows = nc; out->ncols = nr; out->nnz = n;
    const int64_t *rp_a = a.row_ptr;
    const int32_t *ci_a = a.col_idx ? a.col_idx + j0 : nullptr;      // (the keys: A's columns of [j0, j1))
    const void    *va_a = a.vals;
    long long      va_shift = 0;
#define TR_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { out->release(); return fail(CVR_ERR_HIP, "transpose: %s: %s", #expr, hipGetErrorString(e_)); } } while (0)
    if (host && nr > 0) {
        TR_TRY(hipMemcpyAsync(m + o_arp, a.row_ptr, 8 * ((size_t)nr + 1), hipMemcpyHostToDevice, st));
        if (n > 0) TR_TRY(hipMemcpyAsync(m + o_aci, a.col_idx + j0, 4 * (size_t)n, hipMemcpyHostToDevice, st));
        if (n > 0 && !positions) TR_TRY(hipMemcpyAsync(m + o_ava, static_cast<const uint8_t *>(a.vals) + vsz * (size_t)j0, vsz * (size_t)n, hipMemcpyHostToDevice, st));
        rp_a = reinterpret_cast<const int64_t *>(m + o_arp);
        ci_a = reinterpret_cast<const int32_t *>(m + o_aci);
        va_a = m + o_ava;
        va_shift = j0;
    }
    uint32_t *key = reinterpret_cast<uint32_t *>(out->ci), *pin = reinterpret_cast<uint32_t *>(m + o_pin), *pos = reinterpret_cast<uint32_t *>(m + o_pos);
    if (n > 0) {
        hipLaunchKernelGGL(cvr::transpose_iota_kernel, dim3(cvr::grid_of(n)), dim3(256), 0, st, pin, (long long)j0, n);
        TR_TRY(hipGetLastError());
        // (the column range of A was checked before: every key is in [0, ncols), below 2^bits)
        TR_TRY(hipcub::DeviceRadixSort::SortPairs(m + o_work, sort_bytes, reinterpret_cast<const uint32_t *>(ci_a), key, pin, pos, (unsigned int)n, 0, bits, st));
    }
    hipLaunchKernelGGL(cvr::transpose_rows_kernel, dim3(cvr::grid_of(nc + 1)), dim3(256), 0, st, key, n, nc, reinterpret_cast<long long *>(out->rp));
    TR_TRY(hipGetLastError());
    if (n > 0) {
        if (f32) cvr::launch_gather<uint32_t>(positions, reinterpret_cast<const long long *>(rp_a), nr, pos, va_a, va_shift, n, out->ci, out->va, st);
        else cvr::launch_gather<unsigned long long>(positions, reinterpret_cast<const long long *>(rp_a), nr, pos, va_a, va_shift, n, out->ci, out->va, st);
        TR_TRY(hipGetLastError());
    }
    TR_TRY(hipStreamSynchronize(st));
#undef TR_TRY
    return CVR_OK;
}

}  // namespace cvrh
