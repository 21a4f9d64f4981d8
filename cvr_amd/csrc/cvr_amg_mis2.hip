// cvr_amg_mis2.hip -- the device half of the MIS(2) aggregation (include/cvr_amd.h: cvr_amg_mis2_aggregate_device, and what cvr_precond_amg_mis2's
// level loop in cvr_amg.hip calls per level): the structure check of device arrays, the diagonal with dinv and the lowest bad row, the flags of
// the strong entries (taken once per level, not re-derived in a round), the two kernels of a round, the numbering of the roots (rocprim's scan)
// and the two join passes.  The definition and its host loops: cvr_amg_mis2_host.cpp -- every kernel here is one of those loops with a thread per
// row on a grid-stride loop.
//   Why a thread per row: level 0's rows are short (5 to 30 entries) and hold nearly all the rows; the coarse levels, whose rows reach a few
//     hundred entries, have a few thousand rows at most and take microseconds either way.  A round reads 8 bytes per strong entry through a
//     gather (m1, or the state byte of the neighbour) that lanes per row would not coalesce any better.
//   A round is two launches: m1 from the states, then m2 from m1 with the state update in place (thread i alone reads and writes state[i], and m1
//     is read-only there) and the count of the rows still undecided: a sum per wavefront by shuffles, then one integer atomic add per wavefront
//     into the round's own counter.  The host reads the counters back every `check` rounds (CVR_DEBUG=mis2_check=<k>, default 4); a round with
//     nothing undecided changes nothing, so the states and the count of rounds do not depend on k.
//   No kernel waits on another workgroup, no floating-point atomic; the only atomics are atomicMin on the bad-row word and atomicAdd on a counter,
//     both integer and order-free.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "cvr_krylov.h"
#include "cvr_precond.h"
#include "cvr_amg.h"
#include "cvr_amg_mis2.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

constexpr int kNoRow = 0x7fffffff;          // the bad-row word while no row is bad (n < 2^31 - 1)

#define CVR_MIS2_ROWS(i, n) for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < (n); i += (long long)gridDim.x * kThreads)

// the structure rules: bad = the lowest row whose columns are not strictly increasing or that has no diagonal entry
__global__ __launch_bounds__(kThreads) void mis2_structure_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, long long n, int *__restrict__ bad)
{
    CVR_MIS2_ROWS(i, n) {
        long long prev = -1;
        bool      ok = true, diag = false;
        for (long long q = rp[i]; q < rp[i + 1]; q++) {
            const long long c = ci[q];
            ok = ok && c > prev;
            prev = c;
            diag = diag || c == i;
        }
        if (!ok || !diag) atomicMin(bad, (int)i);
    }
}

// diag_i = double(a_ii); dinv_i = T(1 / (+0 + |a_i0| + ..)) in column order (dinv may be null); bad = the lowest row whose diagonal entry is not
// finite or not > 0
template <typename T>
__global__ __launch_bounds__(kThreads) void mis2_diagonal_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ va, long long n,
                                                                 double *__restrict__ diag, T *__restrict__ dinv, int *__restrict__ bad)
{
    CVR_MIS2_ROWS(i, n) {
        double d = 0, s = 0;
        for (long long q = rp[i]; q < rp[i + 1]; q++) {
            const double a = (double)va[q];
            if (ci[q] == i) d = a;
            s = s + fabs(a);
        }
        diag[i] = d;
        if (dinv) dinv[i] = (T)(1.0 / s);
        if (!(d > 0 && d <= amg::kDblMax)) atomicMin(bad, (int)i);
    }
}

// strong[q - j0] = the entry at q passes the strength test
template <typename T>
__global__ __launch_bounds__(kThreads) void mis2_strong_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ va, long long n, long long j0,
                                                               const double *__restrict__ diag, double s2, uint8_t *__restrict__ strong)
{
    CVR_MIS2_ROWS(i, n) {
        const double di = s2 * diag[i];
        for (long long q = rp[i]; q < rp[i + 1]; q++) {
            const int    j = ci[q];
            const double a = (double)va[q];
            strong[q - j0] = j != i && a != 0 && a * a >= di * diag[j];
        }
    }
}

// m1_i = max(key(i), key(j) for j in N(i))
__global__ __launch_bounds__(kThreads) void mis2_m1_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const uint8_t *__restrict__ strong, long long n, long long j0,
                                                           const uint8_t *__restrict__ state, uint64_t *__restrict__ m1)
{
    CVR_MIS2_ROWS(i, n) {
        uint64_t m = amg::mis2_key(state[i], (uint32_t)i);
        for (long long q = rp[i]; q < rp[i + 1]; q++)
            if (strong[q - j0]) {
                const int      j = ci[q];
                const uint64_t k = amg::mis2_key(state[j], (uint32_t)j);
                m = k > m ? k : m;
            }
        m1[i] = m;
    }
}

// m2_i = max(m1_i, m1_j for j in N(i)) of an undecided row and its new state; *undecided += the rows that stay undecided
__global__ __launch_bounds__(kThreads) void mis2_m2_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const uint8_t *__restrict__ strong, long long n, long long j0,
                                                           const uint64_t *__restrict__ m1, uint8_t *__restrict__ state, int *__restrict__ undecided)
{
    int still = 0;
    CVR_MIS2_ROWS(i, n) {
        if (state[i] != amg::kMis2Undecided) continue;
        uint64_t m = m1[i];
        for (long long q = rp[i]; q < rp[i + 1]; q++)
            if (strong[q - j0]) {
                const uint64_t k = m1[ci[q]];
                m = k > m ? k : m;
            }
        if (m == amg::mis2_key(amg::kMis2Undecided, (uint32_t)i)) state[i] = (uint8_t)amg::kMis2Root;
        else if ((m >> 62) == amg::kMis2Root) state[i] = (uint8_t)amg::kMis2Out;
        else still++;
    }
    for (int off = 32; off > 0; off >>= 1) still += __shfl_down(still, off, 64);          // (every lane is here: the loop above has ended)
    if ((threadIdx.x & 63) == 0 && still > 0) atomicAdd(undecided, still);
}

struct IsRoot {
    __host__ __device__ int32_t operator()(uint8_t s) const { return s == amg::kMis2Root ? 1 : 0; }
};

// the strong neighbour j of row i with the largest |a_ij| among those with from[j] >= 0 (ROOTS: that are roots); ties: the lowest j stays
template <typename T, bool ROOTS>
__device__ __forceinline__ int32_t mis2_join(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ va, const uint8_t *__restrict__ strong, long long j0,
                                             long long i, const uint8_t *__restrict__ state, const int32_t *__restrict__ from)
{
    double  best = -1;
    int32_t to = -1;
    for (long long q = rp[i]; q < rp[i + 1]; q++) {
        if (!strong[q - j0]) continue;
        const int j = ci[q];
        int32_t   aj;
        if constexpr (ROOTS) aj = state[j] == amg::kMis2Root ? from[j] - 1 : -1;          // (from: the inclusive scan of the root flags)
        else aj = from[j];
        const double m = fabs((double)va[q]);
        if (aj >= 0 && m > best) {
            best = m;
            to = aj;
        }
    }
    return to;
}

// pass 1: a root takes its number, another row the aggregate of its strongest root
template <typename T>
__global__ __launch_bounds__(kThreads) void mis2_join1_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ va, const uint8_t *__restrict__ strong,
                                                              long long n, long long j0, const uint8_t *__restrict__ state, const int32_t *__restrict__ scan, int32_t *__restrict__ one)
{
    CVR_MIS2_ROWS(i, n) one[i] = state[i] == amg::kMis2Root ? scan[i] - 1 : mis2_join<T, true>(rp, ci, va, strong, j0, i, state, scan);
}

// pass 2: a row that pass 1 left free takes the aggregate of its strongest neighbour that pass 1 did not leave free
template <typename T>
__global__ __launch_bounds__(kThreads) void mis2_join2_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ va, const uint8_t *__restrict__ strong,
                                                              long long n, long long j0, const int32_t *__restrict__ one, int32_t *__restrict__ agg)
{
    CVR_MIS2_ROWS(i, n) agg[i] = one[i] >= 0 ? one[i] : mis2_join<T, false>(rp, ci, va, strong, j0, i, nullptr, one);
}

template <typename... P, typename... A>
void launch_rows(void (*kernel)(P...), long long n, hipStream_t st, A... args)
{
    const long long blocks = std::min<long long>((n + kThreads - 1) / kThreads, kBlocks);
    hipLaunchKernelGGL(kernel, dim3((unsigned)std::max<long long>(blocks, 1)), dim3(kThreads), 0, st, args...);
}

int check_interval()
{
    int k = 4;
    if (const char *e = cvr::debug_env("mis2_check")) {
        const long long v = atoll(e);
        if (v >= 1) k = (int)std::min<long long>(v, 1 << 16);
    }
    return k;
}

template <typename T>
int aggregate_t(const char *entry, const cvr_csr_view &v, int64_t j0, int64_t j1, const double *d_diag, double strength, int32_t *d_agg, int64_t *nc, int32_t *rounds, hipStream_t st)
{
    const long long n = v.nrows;
    const T        *va = static_cast<const T *>(v.vals);
    const int       check = check_interval();
    Scratch         s;
    void           *d_strong = nullptr, *d_state = nullptr, *d_m1 = nullptr, *d_scan = nullptr, *d_one = nullptr, *d_cnt = nullptr, *d_tmp = nullptr;
    if (const int rc = scratch_alloc(entry, s, &d_strong, (size_t)(j1 - j0), "the strong entries' flags")) return rc;
    if (const int rc = scratch_alloc(entry, s, &d_state, (size_t)n, "the rows' states")) return rc;
    if (const int rc = scratch_alloc(entry, s, &d_m1, sizeof(uint64_t) * (size_t)n, "the rows' keys")) return rc;
    if (const int rc = scratch_alloc(entry, s, &d_scan, sizeof(int32_t) * (size_t)n, "the roots' numbers")) return rc;
    if (const int rc = scratch_alloc(entry, s, &d_one, sizeof(int32_t) * (size_t)n, "the first join pass")) return rc;
    if (const int rc = scratch_alloc(entry, s, &d_cnt, sizeof(int) * (size_t)check, "the undecided counts")) return rc;
    uint8_t       *strong = static_cast<uint8_t *>(d_strong), *state = static_cast<uint8_t *>(d_state);
    uint64_t      *m1 = static_cast<uint64_t *>(d_m1);
    int32_t       *scan = static_cast<int32_t *>(d_scan), *one = static_cast<int32_t *>(d_one);
    std::vector<int> cnt((size_t)check, 0);
    HIP_TRY(hipMemsetAsync(state, (int)amg::kMis2Undecided, (size_t)n, st));
    launch_rows(mis2_strong_kernel<T>, n, st, v.row_ptr, v.col_idx, va, n, (long long)j0, d_diag, strength * strength, strong);
    HIP_TRY(hipGetLastError());
    *rounds = 0;
    for (bool done = false; !done;) {
        if ((long long)*rounds > n) return fail(CVR_ERR_STATE, "%s: the MIS(2) rounds did not end within %lld rounds", entry, n);          // (a round decides a row: this is never reached)
        HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(int) * (size_t)check, st));
        for (int r = 0; r < check; r++) {
            launch_rows(mis2_m1_kernel, n, st, v.row_ptr, v.col_idx, (const uint8_t *)strong, n, (long long)j0, (const uint8_t *)state, m1);
            launch_rows(mis2_m2_kernel, n, st, v.row_ptr, v.col_idx, (const uint8_t *)strong, n, (long long)j0, (const uint64_t *)m1, state, static_cast<int *>(d_cnt) + r);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int) * (size_t)check, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int r = 0; r < check && !done; r++) {          // the rounds behind the first count of 0 began with nothing undecided
            ++*rounds;
            done = cnt[(size_t)r] == 0;
        }
    }
    // the roots' numbers: the inclusive scan of their flags, less one; nc is its last element
    const auto flags = rocprim::make_transform_iterator(static_cast<const uint8_t *>(state), IsRoot());
    size_t     bytes = 0;
    HIP_TRY(rocprim::inclusive_scan(nullptr, bytes, flags, scan, (size_t)n, rocprim::plus<int32_t>(), st));
    if (const int rc = scratch_alloc(entry, s, &d_tmp, bytes, "the scan's workspace")) return rc;
    HIP_TRY(rocprim::inclusive_scan(d_tmp, bytes, flags, scan, (size_t)n, rocprim::plus<int32_t>(), st));
    int32_t last = 0;
    HIP_TRY(hipMemcpyAsync(&last, scan + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    launch_rows(mis2_join1_kernel<T>, n, st, v.row_ptr, v.col_idx, va, (const uint8_t *)strong, n, (long long)j0, (const uint8_t *)state, (const int32_t *)scan, one);
    launch_rows(mis2_join2_kernel<T>, n, st, v.row_ptr, v.col_idx, va, (const uint8_t *)strong, n, (long long)j0, (const int32_t *)one, d_agg);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));          // (nc has arrived; the scratch goes)
    *nc = last;
    return CVR_OK;
}

}  // namespace

namespace cvrh {
namespace krylov {

int mis2_check_structure_device(const char *entry, const cvr_csr_view &v, const std::vector<int64_t> &rp_host, hipStream_t st)
{
    const int64_t n = v.nrows;
    if (n == 0) return CVR_OK;
    Scratch s;
    void   *d_bad = nullptr;
    int     bad = kNoRow;
    if (const int rc = scratch_alloc(entry, s, &d_bad, sizeof(int), "the bad-row word")) return rc;
    HIP_TRY(hipMemcpyAsync(d_bad, &bad, sizeof(int), hipMemcpyHostToDevice, st));
    launch_rows(mis2_structure_kernel, n, st, v.row_ptr, v.col_idx, (long long)n, static_cast<int *>(d_bad));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad == kNoRow) return CVR_OK;
    // the offending row alone comes to the host, for the message
    const int64_t        q0 = rp_host[(size_t)bad], q1 = rp_host[(size_t)bad + 1];
    std::vector<int32_t> cols((size_t)(q1 - q0), 0);
    if (q1 > q0) HIP_TRY(hipMemcpy(cols.data(), v.col_idx + q0, sizeof(int32_t) * cols.size(), hipMemcpyDeviceToHost));
    const int64_t rp1[2] = {0, q1 - q0};
    if (const int rc = amg::check_structure(1, rp1, cols.data(), entry, bad)) return rc;
    return fail(CVR_ERR_INVALID, "%s: row %d breaks the structure rules", entry, bad);          // (never: the kernel and the host loop test the same thing)
}

int mis2_diagonal_device(const char *entry, const cvr_csr_view &v, void *d_dinv, double *d_diag, int64_t *bad_row, hipStream_t st)
{
    const long long n = v.nrows;
    *bad_row = -1;
    if (n == 0) return CVR_OK;
    Scratch s;
    void   *d_bad = nullptr;
    int     bad = kNoRow;
    if (const int rc = scratch_alloc(entry, s, &d_bad, sizeof(int), "the bad-row word")) return rc;
    HIP_TRY(hipMemcpyAsync(d_bad, &bad, sizeof(int), hipMemcpyHostToDevice, st));
    if (v.is_f32) launch_rows(mis2_diagonal_kernel<float>, n, st, v.row_ptr, v.col_idx, static_cast<const float *>(v.vals), n, d_diag, static_cast<float *>(d_dinv), static_cast<int *>(d_bad));
    else launch_rows(mis2_diagonal_kernel<double>, n, st, v.row_ptr, v.col_idx, static_cast<const double *>(v.vals), n, d_diag, static_cast<double *>(d_dinv), static_cast<int *>(d_bad));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad != kNoRow) *bad_row = bad;
    return CVR_OK;
}

int mis2_aggregate_device(const char *entry, const cvr_csr_view &v, int64_t j0, int64_t j1, const double *d_diag, double strength, int32_t *d_agg, int64_t *nc, int32_t *rounds,
                          hipStream_t st)
{
    *nc = 0;
    *rounds = 0;
    if (v.nrows == 0) return CVR_OK;
    return v.is_f32 ? aggregate_t<float>(entry, v, j0, j1, d_diag, strength, d_agg, nc, rounds, st) : aggregate_t<double>(entry, v, j0, j1, d_diag, strength, d_agg, nc, rounds, st);
}

}  // namespace krylov
}  // namespace cvrh

extern "C" {

int cvr_amg_mis2_aggregate_device(const cvr_csr_view *csr, double strength, int32_t *agg_dev, int64_t *nc, int32_t *rounds, int device, void *stream)
{
    const char *entry = "cvr_amg_mis2_aggregate_device";
    if (!csr || !nc || !rounds) return fail(CVR_ERR_INVALID, "null argument");
    *nc = 0;
    *rounds = 0;
    if (!(strength >= 0 && strength < 1)) return fail(CVR_ERR_INVALID, "%s: strength = %g: must be 0 <= strength < 1", entry, strength);
    if (!csr->arrays_on_device) return fail(CVR_ERR_INVALID, "%s: the arrays must be device arrays", entry);
    if (csr->nrows != csr->ncols) return fail(CVR_ERR_INVALID, "AMG needs a square matrix (%lld x %lld)", (long long)csr->nrows, (long long)csr->ncols);
    if (csr->nrows < 0) return fail(CVR_ERR_INVALID, "null or negative-size CSR view");
    if (csr->nrows >= (int64_t)0x7fffffff) return fail(CVR_ERR_INVALID, "%s: nrows (%lld) must stay below 2^31 - 1", entry, (long long)csr->nrows);
    if (csr->nrows > 0 && !agg_dev) return fail(CVR_ERR_INVALID, "null argument");
    if (device < 0 || device >= cvr_device_count()) return fail(CVR_ERR_NO_DEVICE, "device %d of %d", device, cvr_device_count());
    cvr::debug_refresh();
    Range range(entry);
    HIP_TRY(hipSetDevice(device));
    hipStream_t          st = (hipStream_t)stream;
    std::vector<int64_t> rp_host;
    if (const int rc = check_device_view(entry, csr, rp_host, st)) return rc;
    if (csr->nrows == 0) return CVR_OK;
    if (rp_host.back() > rp_host.front() && !csr->vals) return fail(CVR_ERR_INVALID, "vals is null");
    if (const int rc = mis2_check_structure_device(entry, *csr, rp_host, st)) return rc;
    Scratch s;
    void   *d_diag = nullptr;
    int64_t bad = -1;
    if (const int rc = scratch_alloc(entry, s, &d_diag, sizeof(double) * (size_t)csr->nrows, "the diagonal")) return rc;
    if (const int rc = mis2_diagonal_device(entry, *csr, nullptr, static_cast<double *>(d_diag), &bad, st)) return rc;          // (the diagonal's sign is not this call's business)
    return mis2_aggregate_device(entry, *csr, rp_host.front(), rp_host.back(), static_cast<const double *>(d_diag), strength, agg_dev, nc, rounds, st);
}

}  // extern "C"
