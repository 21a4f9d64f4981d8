// cvr_color.hip -- the device half of the graph colouring (include/cvr_amd.h: cvr_color_device, and what cvr_precond_mcsgs builds on): the pattern
// rules of device arrays, the rounds on hashed keys and the rows ordered by (colour, row).  The definition and its host loops:
// cvr_color_host.cpp -- every kernel here is one of those loops with a thread per row.
//   The rules: one kernel, a thread per row on a grid-stride loop; the lowest row that breaks ILU(0)'s structure rules and the lowest row with an
//     entry (i, j) whose (j, i) a binary search of row j does not find come back in two words (integer atomicMin), read together.
//   A round: one kernel, a thread per row on a grid-stride loop, one int32 word per row (-1 or the colour) read from one array and written to the
//     other, so a round sees the state before it and nothing else.  First fit by a 64-bit mask of the neighbours' colours in [base, base + 64); a
//     full window moves on by 64.  The rows still uncoloured: a sum per wavefront by shuffles, then one integer atomicAdd per wavefront into the
//     round's own counter; the largest colour the same way by atomicMax.  The host reads the counters back every `check` rounds
//     (CVR_DEBUG=color_check=<k>, default 4); a round with nothing uncoloured copies its input, so no bit and no count depends on k.
//   The order: a counting sort without an order-dependent atomic.  A workgroup takes 256 consecutive rows; a thread's rank is the number of rows
//     before it in the workgroup with its colour (a loop over the colours in LDS), the last row of a colour stores the workgroup's count of it;
//     rocprim's exclusive scan of the counts in (colour, workgroup) order gives every pair its place, the rank the row's place behind it.
//   No kernel waits on another workgroup, no floating-point atomic, plain C++ stores.
#include <rocprim/device/device_scan.hpp>

#include "cvr_krylov.h"
#include "cvr_color.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

constexpr int kNoRow = 0x7fffffff;          // a bad-row word while no row is bad (rows are below 2^31 - 1)

#define CVR_COLOR_ROWS(i, n) for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < (n); i += (long long)gridDim.x * kThreads)

// bad[0]: the lowest row whose columns are not strictly increasing or that has no diagonal entry; bad[1]: the lowest row with an off-diagonal
// entry (i, j) that row j does not answer (meaningful where bad[0] stays free: the search needs sorted rows; it stays inside row j either way)
__global__ __launch_bounds__(kThreads) void color_rules_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, long long n, int *__restrict__ bad)
{
    CVR_COLOR_ROWS(i, n) {
        long long prev = -1;
        bool      ok = true, diag = false, sym = true;
        for (long long q = rp[i]; q < rp[i + 1]; q++) {
            const long long c = ci[q];
            ok = ok && c > prev;
            prev = c;
            diag = diag || c == i;
            if (c == i) continue;
            long long lo = rp[c], hi = rp[c + 1];          // the first position of row c whose column is >= i
            while (lo < hi) {
                const long long mid = lo + ((hi - lo) >> 1);
                if (ci[mid] < i) lo = mid + 1;
                else hi = mid;
            }
            sym = sym && lo < rp[c + 1] && ci[lo] == i;
        }
        if (!ok || !diag) atomicMin(bad, (int)i);
        if (!sym) atomicMin(bad + 1, (int)i);
    }
}

// One round: out = the state behind it, from in = the state before it.  *uncoloured += the rows it leaves uncoloured; *top = max(*top, the
// colours it gives).
__global__ __launch_bounds__(kThreads) void color_round_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, long long n, const int32_t *__restrict__ in,
                                                               int32_t *__restrict__ out, int *__restrict__ uncoloured, int *__restrict__ top)
{
    int still = 0, mx = -1;
    CVR_COLOR_ROWS(i, n) {
        int32_t s = in[i];
        if (s == color::kUncoloured) {
            const long long b = rp[i], e = rp[i + 1];
            const uint64_t  k = color::key((uint32_t)i);
            bool            first = true;
            for (long long q = b; q < e && first; q++) {
                const int j = ci[q];
                first = j == i || in[j] != color::kUncoloured || color::key((uint32_t)j) < k;
            }
            if (first) {
                for (int base = 0; s < 0; base += 64) {
                    unsigned long long mask = 0;
                    for (long long q = b; q < e; q++) {
                        const int j = ci[q], cj = in[j];
                        if (j != i && cj >= base && cj < base + 64) mask |= 1ull << (cj - base);
                    }
                    if (~mask) s = base + __builtin_ctzll(~mask);
                }
                mx = s > mx ? s : mx;
            } else still++;
        }
        out[i] = s;
    }
    for (int off = 32; off > 0; off >>= 1) {          // (every lane is here: the loop above has ended)
        still += __shfl_down(still, off, 64);
        const int o = __shfl_down(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        if (still > 0) atomicAdd(uncoloured, still);
        if (mx >= 0) atomicMax(top, mx);
    }
}

// rank[i] = the rows before i among the workgroup's 256 with i's colour; count[c * nb + workgroup] = the workgroup's rows of colour c (stored by
// the last of them; the others stay at the 0 they were set to)
__global__ __launch_bounds__(kThreads) void color_rank_kernel(const int32_t *__restrict__ color, long long n, long long nb, int32_t *__restrict__ rank, int32_t *__restrict__ count)
{
    __shared__ int32_t sh[kThreads];
    const long long    i = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int32_t      c = i < n ? color[i] : -1;
    sh[threadIdx.x] = c;
    __syncthreads();
    if (i >= n || c < 0) return;          // (c < 0: never, the rounds have ended)
    int before = 0, behind = 0;
    for (int t = 0; t < (int)threadIdx.x; t++) before += sh[t] == c;
    for (int t = threadIdx.x + 1; t < kThreads; t++) behind += sh[t] == c;
    rank[i] = before;
    if (behind == 0) count[(long long)c * nb + blockIdx.x] = before + 1;
}

// perm: row i to the place of its (colour, workgroup) pair plus its rank
__global__ __launch_bounds__(kThreads) void color_place_kernel(const int32_t *__restrict__ color, const int32_t *__restrict__ rank, const int32_t *__restrict__ place, long long n,
                                                               long long nb, int32_t *__restrict__ perm)
{
    CVR_COLOR_ROWS(i, n) perm[place[(long long)color[i] * nb + i / kThreads] + rank[i]] = (int32_t)i;
}

// color_ptr[c] = the place of colour c's first pair; color_ptr[ncolors] = n (the scan's last element)
__global__ __launch_bounds__(kThreads) void color_ptr_kernel(const int32_t *__restrict__ place, int ncolors, long long nb, int32_t *__restrict__ color_ptr)
{
    CVR_COLOR_ROWS(c, (long long)ncolors + 1) color_ptr[c] = place[c * nb];
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
    if (const char *e = cvr::debug_env("color_check")) {
        const long long v = atoll(e);
        if (v >= 1) k = (int)std::min<long long>(v, 1 << 16);
    }
    return k;
}

// the message of a broken rule: the offending row alone comes to the host, and for the symmetry rule the rows its columns name, one at a time
int explain(const char *entry, const cvr_csr_view &dv, const int64_t *rp, int bad_structure, int bad_symmetry)
{
    auto fetch = [&](int64_t i, std::vector<int32_t> &cols) {
        cols.assign((size_t)(rp[i + 1] - rp[i]), 0);
        if (!cols.empty()) HIP_TRY(hipMemcpy(cols.data(), dv.col_idx + rp[i], sizeof(int32_t) * cols.size(), hipMemcpyDeviceToHost));
        return (int)CVR_OK;
    };
    std::vector<int32_t> row, other;
    if (bad_structure != kNoRow) {
        if (const int rc = fetch(bad_structure, row)) return rc;
        const int64_t rp1[2] = {0, (int64_t)row.size()};
        if (const int rc = color::check_structure(1, rp1, row.data(), entry, bad_structure)) return rc;
        return fail(CVR_ERR_INVALID, "%s: row %d breaks the structure rules", entry, bad_structure);          // (never: the kernel and the host loop test the same thing)
    }
    if (const int rc = fetch(bad_symmetry, row)) return rc;
    for (const int32_t j : row) {
        if (j == bad_symmetry) continue;
        if (const int rc = fetch(j, other)) return rc;
        if (!std::binary_search(other.begin(), other.end(), (int32_t)bad_symmetry)) return color::fail_asymmetric(entry, bad_symmetry, j);
    }
    return fail(CVR_ERR_INVALID, "%s: row %d breaks the symmetry rule", entry, bad_symmetry);          // (never)
}

}  // namespace

namespace cvrh {
namespace krylov {

int stage_device(const char *entry, const cvr_csr_view *c, bool with_values, Scratch &s, cvr_csr_view *dv, std::vector<int64_t> &rp_own, const int64_t **rp_host, hipStream_t st)
{
    cvr_csr_view v = *c;
    if (!with_values && !v.vals) v.vals = v.col_idx;          // (not read)
    *dv = v;
    if (c->arrays_on_device) {
        if (const int rc = check_device_view(entry, &v, rp_own, st)) return rc;
        *rp_host = rp_own.data();
        return CVR_OK;
    }
    if (const int rc = check_csr(&v, true)) return rc;
    *rp_host = c->row_ptr;
    const int64_t n = c->nrows;
    if (n == 0) return CVR_OK;
    const int64_t j0 = c->row_ptr[0], j1 = c->row_ptr[n];
    const size_t  vsz = c->is_f32 ? 4 : 8;
    void         *d_rp = nullptr, *d_ci = nullptr, *d_va = nullptr;
    if (const int rc = scratch_alloc(entry, s, &d_rp, sizeof(int64_t) * (size_t)(n + 1), "row_ptr")) return rc;
    if (const int rc = scratch_alloc(entry, s, &d_ci, sizeof(int32_t) * (size_t)j1, "col_idx")) return rc;
    HIP_TRY(hipMemcpyAsync(d_rp, c->row_ptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, st));
    if (j1 > j0) HIP_TRY(hipMemcpyAsync(static_cast<int32_t *>(d_ci) + j0, c->col_idx + j0, sizeof(int32_t) * (size_t)(j1 - j0), hipMemcpyHostToDevice, st));
    if (with_values) {
        if (const int rc = scratch_alloc(entry, s, &d_va, vsz * (size_t)j1, "vals")) return rc;
        if (j1 > j0)
            HIP_TRY(hipMemcpyAsync(static_cast<uint8_t *>(d_va) + vsz * (size_t)j0, static_cast<const uint8_t *>(c->vals) + vsz * (size_t)j0, vsz * (size_t)(j1 - j0), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));          // (the caller's arrays may go once this returns)
    dv->row_ptr = static_cast<const int64_t *>(d_rp);
    dv->col_idx = static_cast<const int32_t *>(d_ci);
    dv->vals = with_values ? d_va : d_ci;
    dv->arrays_on_device = 1;
    return CVR_OK;
}

int color_device(const char *entry, const cvr_csr_view &dv, const int64_t *rp_host, int32_t *d_color, int32_t *d_perm, std::vector<int32_t> &color_ptr, int32_t *ncolors, int32_t *rounds,
                 hipStream_t st)
{
    const long long n = dv.nrows;
    const int       check = check_interval();
    Scratch         s;
    void           *d_words = nullptr, *d_other = nullptr;
    // the words the host reads: [0], [1] the bad rows, [2] the largest colour, [3 ..] the rounds' counters
    if (const int rc = scratch_alloc(entry, s, &d_words, sizeof(int) * (size_t)(3 + check), "the words the host reads")) return rc;
    if (const int rc = scratch_alloc(entry, s, &d_other, sizeof(int32_t) * (size_t)n, "the rows' second state")) return rc;
    int             *words = static_cast<int *>(d_words);
    std::vector<int> host((size_t)(3 + check), 0);
    host[0] = host[1] = kNoRow;
    host[2] = -1;
    HIP_TRY(hipMemcpyAsync(words, host.data(), sizeof(int) * 3, hipMemcpyHostToDevice, st));
    launch_rows(color_rules_kernel, n, st, dv.row_ptr, dv.col_idx, n, words);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host.data(), words, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (host[0] != kNoRow || host[1] != kNoRow) return explain(entry, dv, rp_host, host[0], host[1]);

    int32_t *in = d_color, *out = static_cast<int32_t *>(d_other);
    HIP_TRY(hipMemsetAsync(in, 0xff, sizeof(int32_t) * (size_t)n, st));          // kUncoloured
    *rounds = 0;
    for (bool done = false; !done;) {
        if ((long long)*rounds > n) return fail(CVR_ERR_STATE, "%s: the colouring did not end within %lld rounds", entry, n);          // (a round colours a row: this is never reached)
        HIP_TRY(hipMemsetAsync(words + 3, 0, sizeof(int) * (size_t)check, st));
        for (int r = 0; r < check; r++) {
            launch_rows(color_round_kernel, n, st, dv.row_ptr, dv.col_idx, n, (const int32_t *)in, out, words + 3 + r, words + 2);
            std::swap(in, out);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host.data() + 2, words + 2, sizeof(int) * (size_t)(1 + check), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int r = 0; r < check && !done; r++) {          // the rounds behind the first count of 0 began with nothing uncoloured
            ++*rounds;
            done = host[(size_t)(3 + r)] == 0;
        }
    }
    if (in != d_color) HIP_TRY(hipMemcpyAsync(d_color, in, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    *ncolors = host[2] + 1;

    // the order
    const long long nb = (n + kThreads - 1) / kThreads;
    const size_t    pairs = (size_t)*ncolors * (size_t)nb + 1;
    if (pairs > (size_t)0x7fffffff) return fail(CVR_ERR_NOMEM, "%s: %d colours of %lld rows need %zu counters for the order", entry, *ncolors, n, pairs);
    void  *d_rank = nullptr, *d_count = nullptr, *d_place = nullptr, *d_cptr = nullptr, *d_tmp = nullptr;
    size_t bytes = 0;
    if (const int rc = scratch_alloc(entry, s, &d_rank, sizeof(int32_t) * (size_t)n, "the rows' ranks")) return rc;
    if (const int rc = scratch_alloc(entry, s, &d_count, sizeof(int32_t) * pairs, "the workgroups' counts")) return rc;
    if (const int rc = scratch_alloc(entry, s, &d_place, sizeof(int32_t) * pairs, "the pairs' places")) return rc;
    if (const int rc = scratch_alloc(entry, s, &d_cptr, sizeof(int32_t) * (size_t)(*ncolors + 1), "color_ptr")) return rc;
    int32_t *count = static_cast<int32_t *>(d_count), *place = static_cast<int32_t *>(d_place);
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(int32_t) * pairs, st));
    hipLaunchKernelGGL(color_rank_kernel, dim3((unsigned)nb), dim3(kThreads), 0, st, (const int32_t *)d_color, n, nb, static_cast<int32_t *>(d_rank), count);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::exclusive_scan(nullptr, bytes, count, place, (int32_t)0, pairs, rocprim::plus<int32_t>(), st));
    if (const int rc = scratch_alloc(entry, s, &d_tmp, bytes, "the scan's workspace")) return rc;
    HIP_TRY(rocprim::exclusive_scan(d_tmp, bytes, count, place, (int32_t)0, pairs, rocprim::plus<int32_t>(), st));
    launch_rows(color_place_kernel, n, st, (const int32_t *)d_color, (const int32_t *)d_rank, (const int32_t *)place, n, nb, d_perm);
    launch_rows(color_ptr_kernel, (long long)*ncolors + 1, st, (const int32_t *)place, (int)*ncolors, nb, static_cast<int32_t *>(d_cptr));
    HIP_TRY(hipGetLastError());
    try {
        color_ptr.assign((size_t)*ncolors + 1, 0);
    } catch (const std::bad_alloc &) {
        (void)hipStreamSynchronize(st);
        return fail(CVR_ERR_NOMEM, "%s: out of host memory for color_ptr (%d colours)", entry, *ncolors);
    }
    HIP_TRY(hipMemcpyAsync(color_ptr.data(), d_cptr, sizeof(int32_t) * color_ptr.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));          // (the scratch goes)
    return CVR_OK;
}

}  // namespace krylov
}  // namespace cvrh

extern "C" {

int cvr_color_device(const cvr_csr_view *csr, int32_t device, void *stream, int32_t *color, int32_t *perm, int32_t *color_ptr, int32_t *ncolors, int32_t *rounds)
{
    const char *entry = "cvr_color_device";
    if (!csr || !ncolors || !rounds || !color_ptr) return fail(CVR_ERR_INVALID, "null argument");
    *ncolors = 0;
    *rounds = 0;
    if (const int rc = color::check_view(csr, entry)) return rc;
    if (csr->nrows > 0 && (!color || !perm)) return fail(CVR_ERR_INVALID, "null argument");
    if (device < 0 || device >= cvr_device_count()) return fail(CVR_ERR_NO_DEVICE, "device %d of %d", device, cvr_device_count());
    cvr::debug_refresh();
    Range range(entry);
    HIP_TRY(hipSetDevice(device));
    hipStream_t          st = (hipStream_t)stream;
    Scratch              s;
    cvr_csr_view         dv;
    std::vector<int64_t> rp_own;
    const int64_t       *rp = nullptr;
    if (const int rc = stage_device(entry, csr, false, s, &dv, rp_own, &rp, st)) return rc;
    color_ptr[0] = 0;
    const int64_t n = csr->nrows;
    if (n == 0) return CVR_OK;
    void *d_color = nullptr, *d_perm = nullptr;
    if (const int rc = scratch_alloc(entry, s, &d_color, sizeof(int32_t) * (size_t)n, "the colours")) return rc;
    if (const int rc = scratch_alloc(entry, s, &d_perm, sizeof(int32_t) * (size_t)n, "perm")) return rc;
    std::vector<int32_t> cptr;
    if (const int rc = color_device(entry, dv, rp, static_cast<int32_t *>(d_color), static_cast<int32_t *>(d_perm), cptr, ncolors, rounds, st)) {
        *ncolors = 0;
        *rounds = 0;
        return rc;
    }
    HIP_TRY(hipMemcpy(color, d_color, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(perm, d_perm, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    std::copy(cptr.begin(), cptr.end(), color_ptr);
    return CVR_OK;
}

}  // extern "C"
