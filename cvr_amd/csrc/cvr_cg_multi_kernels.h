// cvr_cg_multi_kernels.h -- the vector kernels and the host pieces of batched conjugate gradients (cvr_cg_multi.hip:
// cvr_cg_multi_device, cvr_pcg_multi_device).  cvr_pcg_multi.hip includes it for the column walk of its k-wide apply.
// What the kernels do and how a row's columns are walked: cvr_cg_multi.hip's head.
#pragma once
#include "cvr_krylov.h"

namespace cvrh {
namespace krylov {
namespace {

constexpr int kCols = cvr::kSpmmBlock;          // columns per call
constexpr int kSets = 3;                        // partial-sum sets per column in `part`: column c's begin at part + c * kSets * kBlocks

// the sub-block's values at p + off for the columns of `mask` (bits 0 .. kPack - 1): one 16-byte store when all of them are live, else one by one
template <typename T, bool VEC>
__device__ __forceinline__ void store_cols(T *__restrict__ p, long long off, uint32_t mask, const T (&v)[kPack<T>])
{
    constexpr uint32_t kFull = (1u << kPack<T>) - 1;
    if (VEC && mask == kFull) {
        store_pack<T, true>(p, off, kPack<T>, v);
    } else {
#pragma unroll
        for (int i = 0; i < kPack<T>; i++) if (mask >> i & 1u) p[off + i] = v[i];
    }
}

// the sub-blocks of one row: cb = the first column, cc = how many of its kPack<T> columns exist (the loop is unrolled: cb is a constant in the body)
#define CVR_CG_MULTI_SUBBLOCKS(T, cb, cc)                 \
    _Pragma("unroll") for (int cb = 0; cb < kCols; cb += kPack<T>) \
        if (int cc = nvec - cb < kPack<T> ? nvec - cb : kPack<T>; cc > 0)

// P = [X0 | a zero row] with ld = nvec, from the caller's X of leading dimension ldx
template <typename T>
__global__ __launch_bounds__(kThreads) void cgm_start_kernel(const T *__restrict__ x, long long ldx, T *__restrict__ p, long long n, int nvec)
{
    const long long total = (n + 1) * nvec;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
        const long long row = i / nvec;
        p[i] = row < n ? x[row * ldx + (i - row * nvec)] : (T)0;
    }
}

// x = 0 in the columns of `mask` (b == 0 there)
template <typename T>
__global__ __launch_bounds__(kThreads) void cgm_zero_kernel(T *__restrict__ x, long long ldx, long long n, int nvec, uint32_t mask)
{
    for (long long row = (long long)blockIdx.x * kThreads + threadIdx.x; row < n; row += (long long)gridDim.x * kThreads)
        for (int c = 0; c < nvec; c++)
            if (mask >> c & 1u) x[row * ldx + c] = (T)0;
}

// The start: q holds A x0.  r = T(b - q) (the scaled product's alpha = -1, beta = 1 write-out), z = minv .* r (PRE), p = z (or r), and per column
// the partial sums of r . r, r . z (PRE) and b . b.  LV: the library's blocks take 16-byte packets (nvec is a multiple of kPack); AL: so do b
// (ldb a multiple of kPack, 16-byte aligned) and minv.
template <typename T, bool PRE, bool LV, bool AL>
__global__ __launch_bounds__(kThreads) void cgm_init_kernel(const T *__restrict__ b, long long ldb, const T *__restrict__ minv, const T *__restrict__ q,
                                                            T *__restrict__ r, T *__restrict__ z, T *__restrict__ p, long long n, int nvec,
                                                            double *__restrict__ out)
{
    __shared__ double sh[kCols][kSets][kWaves];
    double acc[kCols][kSets] = {};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T mv[kPack<T>];
        if constexpr (PRE) load_pack<T, AL>(minv, e, (int)cnt, mv);
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            const uint32_t all = (1u << cc) - 1;
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) {
                if (j < cnt) {
                    const long long row = e + j;
                    T bv[kPack<T>], qv[kPack<T>], rv[kPack<T>], zv[kPack<T>];
                    load_pack<T, AL>(b, row * ldb + cb, cc, bv);
                    load_pack<T, LV>(q, row * nvec + cb, cc, qv);
#pragma unroll
                    for (int i = 0; i < kPack<T>; i++) {
                        rv[i] = bv[i] - qv[i];
                        zv[i] = PRE ? (T)((double)mv[j] * (double)rv[i]) : rv[i];
                        acc[cb + i][0] += (double)rv[i] * (double)rv[i];
                        if constexpr (PRE) acc[cb + i][1] += (double)rv[i] * (double)zv[i];
                        acc[cb + i][2] += (double)bv[i] * (double)bv[i];
                    }
                    store_cols<T, LV>(r, row * nvec + cb, all, rv);
                    if constexpr (PRE) store_cols<T, LV>(z, row * nvec + cb, all, zv);
                    store_cols<T, LV>(p, row * nvec + cb, all, zv);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < kCols; c++)
        if (c < nvec) store_partials<kSets>(acc[c], out + (size_t)c * kSets * kBlocks, sh[c]);
}

// per column the partial sums of p . q
template <typename T, bool LV>
__global__ __launch_bounds__(kThreads) void cgm_pq_kernel(const T *__restrict__ p, const T *__restrict__ q, long long n, int nvec, double *__restrict__ out,
                                                          const CgCell *__restrict__ cells)
{
    __shared__ double sh[kCols][1][kWaves];
    int going = 0;          // (no workgroup of this kernel sets a stop)
    for (int c = 0; c < nvec; c++) going |= !cells[c].stop;
    if (!going) return;
    double acc[kCols][1] = {};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) {
                if (j < cnt) {
                    T pv[kPack<T>], qv[kPack<T>];
                    load_pack<T, LV>(p, (e + j) * nvec + cb, cc, pv);
                    load_pack<T, LV>(q, (e + j) * nvec + cb, cc, qv);
#pragma unroll
                    for (int i = 0; i < kPack<T>; i++) acc[cb + i][0] += (double)pv[i] * (double)qv[i];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < kCols; c++)
        if (c < nvec) store_partials<1>(acc[c], out + (size_t)c * kBlocks, sh[c]);
}

// Step k, per column that has not stopped: alpha = r.z / p.q; x += alpha p, r -= alpha q, z = minv .* r; the partial sums of r . r (set 0) and
// r . z (set 1, PRE).  p.q <= 0 or not finite: that column's breakdown, recorded, nothing of it written.  AL: x (ldx a multiple of kPack, 16-byte
// aligned) and minv take 16-byte packets.
template <typename T, bool PRE, bool LV, bool AL>
__global__ __launch_bounds__(kThreads) void cgm_update_kernel(T *__restrict__ x, long long ldx, T *__restrict__ r, T *__restrict__ z, const T *__restrict__ p,
                                                              const T *__restrict__ q, const T *__restrict__ minv, long long n, int nvec,
                                                              const double *__restrict__ part_pq, double *__restrict__ out, CgCell *__restrict__ cells, int k)
{
    constexpr int K = PRE ? 2 : 1;
    __shared__ double shp[kCols][1][kWaves];
    __shared__ double sh[kCols][K][kWaves];
    __shared__ int stopped[kCols];
    if ((int)threadIdx.x < nvec) stopped[threadIdx.x] = cells[threadIdx.x].stop;
    double   alpha[kCols] = {};
    uint32_t live = 0;
#pragma unroll
    for (int c = 0; c < kCols; c++) {
        if (c < nvec) {
            double pq[1];
            sum_partials<1>(part_pq + (size_t)c * kBlocks, pq, shp[c]);
            if (stopped[c]) continue;
            if (!(pq[0] > 0) || !(pq[0] <= kDblMax)) {
                if (blockIdx.x == 0 && threadIdx.x == 0) { cells[c].status = CVR_CG_BREAKDOWN; cells[c].stop = 1; }
                continue;
            }
            alpha[c] = cells[c].rz[k & 1] / pq[0];
            if (blockIdx.x == 0 && threadIdx.x == 0) cells[c].iters = k + 1;
            live |= 1u << c;
        }
    }
    if (!live) return;
    double acc[kCols][K] = {};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T mv[kPack<T>];
        if constexpr (PRE) load_pack<T, AL>(minv, e, (int)cnt, mv);
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            const uint32_t m = live >> cb & ((1u << cc) - 1);
            if (!m) continue;
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) {
                if (j < cnt) {
                    const long long row = e + j;
                    T xv[kPack<T>], rv[kPack<T>], pv[kPack<T>], qv[kPack<T>], zv[kPack<T>];
                    load_pack<T, AL>(x, row * ldx + cb, cc, xv);
                    load_pack<T, LV>(r, row * nvec + cb, cc, rv);
                    load_pack<T, LV>(p, row * nvec + cb, cc, pv);
                    load_pack<T, LV>(q, row * nvec + cb, cc, qv);
#pragma unroll
                    for (int i = 0; i < kPack<T>; i++) {
                        xv[i] = (T)((double)xv[i] + alpha[cb + i] * (double)pv[i]);
                        rv[i] = (T)((double)rv[i] - alpha[cb + i] * (double)qv[i]);
                        if constexpr (PRE) zv[i] = (T)((double)mv[j] * (double)rv[i]);
                        acc[cb + i][0] += (double)rv[i] * (double)rv[i];
                        if constexpr (PRE) acc[cb + i][1] += (double)rv[i] * (double)zv[i];
                    }
                    store_cols<T, AL>(x, row * ldx + cb, m, xv);
                    store_cols<T, LV>(r, row * nvec + cb, m, rv);
                    if constexpr (PRE) store_cols<T, LV>(z, row * nvec + cb, m, zv);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < kCols; c++)
        if (c < nvec) store_partials<K>(acc[c], out + (size_t)c * kSets * kBlocks, sh[c]);
}

// Step k, behind the update, per column that has not stopped: r.r and r.z from its partials into its cell; ||r|| <= rtol ||b||: converged, recorded,
// nothing of it written; else p = z + beta p with beta = r.z / r.z of the step before.  z is r without a preconditioner.
template <typename T, bool PRE, bool LV>
__global__ __launch_bounds__(kThreads) void cgm_direction_kernel(T *__restrict__ p, const T *__restrict__ z, long long n, int nvec, const double *__restrict__ part,
                                                                 CgCell *__restrict__ cells, int k, double rtol)
{
    constexpr int K = PRE ? 2 : 1;
    __shared__ double sh[kCols][K][kWaves];
    __shared__ int stopped[kCols];
    if ((int)threadIdx.x < nvec) stopped[threadIdx.x] = cells[threadIdx.x].stop;
    double   beta[kCols] = {};
    uint32_t live = 0;
#pragma unroll
    for (int c = 0; c < kCols; c++) {
        if (c < nvec) {
            double s[K];
            sum_partials<K>(part + (size_t)c * kSets * kBlocks, s, sh[c]);
            if (stopped[c]) continue;
            const double rr = s[0], rz = s[K - 1], rnorm = sqrt(rr);
            const bool   done = rnorm <= rtol * cells[c].bnorm;
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                cells[c].rr = rr; cells[c].rnorm = rnorm; cells[c].rz[(k + 1) & 1] = rz;
                if (done) { cells[c].status = CVR_CG_CONVERGED; cells[c].stop = 1; }
            }
            if (done) continue;
            beta[c] = rz / cells[c].rz[k & 1];
            live |= 1u << c;
        }
    }
    if (!live) return;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            const uint32_t m = live >> cb & ((1u << cc) - 1);
            if (!m) continue;
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) {
                if (j < cnt) {
                    T pv[kPack<T>], zv[kPack<T>];
                    load_pack<T, LV>(p, (e + j) * nvec + cb, cc, pv);
                    load_pack<T, LV>(z, (e + j) * nvec + cb, cc, zv);
#pragma unroll
                    for (int i = 0; i < kPack<T>; i++) pv[i] = (T)((double)zv[i] + beta[cb + i] * (double)pv[i]);
                    store_cols<T, LV>(p, (e + j) * nvec + cb, m, pv);
                }
            }
        }
    }
}

// the library's blocks of one call: P (x_ext rows, ld = nvec), Q and R (y_ext rows each), Z, the partial sums, the cells
template <typename T>
struct Workspace {
    T      *p, *q, *r, *z;
    double *part_pq, *part;
    CgCell *cells;
};

// what the vector launches of a call share.  lv: the library's blocks take 16-byte packets; al: so do the caller's
template <typename T>
struct Call {
    const T  *b; long long ldb;
    T        *x; long long ldx;
    const T  *minv;
    long long n;
    int       nvec;
    bool      lv, al;
    double    rtol;
};

// what both entry points check beside check_solver_args, before any device work and before the handle is looked at
inline int check_block_args(int32_t nvec, int64_t ldb, int64_t ldx)
{
    if (nvec < 1 || nvec > kCols) return fail(CVR_ERR_INVALID, "nvec = %d: 1 to %d right-hand sides per call", nvec, kCols);
    if (ldb < nvec || ldx < nvec) return fail(CVR_ERR_INVALID, "ldb = %lld, ldx = %lld: each must be >= nvec = %d", (long long)ldb, (long long)ldx, nvec);
    return CVR_OK;
}

// what is asked of the handle (`entry`: "cvr_cg_multi", "cvr_pcg_multi"); single: one vector of stride 1, which goes through run_spmv on any layout
inline int check_handle(const cvr_handle *h, int32_t nvec, bool single, const char *entry)
{
    if (const int rc = check_square_preprocessed(h, entry, "conjugate gradients need")) return rc;
    if (single) return CVR_OK;
    if (!cvr_spmm_supported(h)) return fail(CVR_ERR_STATE, "%s: this handle's image is not the plain layout; create it with cvr_options.nvec >= 2 for several right-hand sides", entry);
    if ((uint64_t)(h->info.ncols + 1) * (uint64_t)nvec * h->vsz > 0xffffffffull)
        return fail(CVR_ERR_INVALID, "P of %lld rows of %d values exceeds the 4 GiB a buffer descriptor addresses", (long long)(h->info.ncols + 1), nvec);
    return CVR_OK;
}

// Q = A P for all columns
template <typename T>
int product(cvr_handle *h, bool single, const Workspace<T> &w, int nvec, hipStream_t st)
{
    if (single) {
        HIP_TRY(run_spmv(h, w.p, w.q, st));
        return CVR_OK;
    }
    if (h->d_map) HIP_TRY(handle_enter(h, st));          // (a mutable handle's image: ordered with its updates, as cvr_spmm_device)
    HIP_TRY(cvr::launch_spmm(h->parts[0].img, w.p, nvec, w.q, nvec, nvec, st));
    if (h->d_map) HIP_TRY(handle_leave(h, st));
    return CVR_OK;
}

// A host entry point around its device form fn(B_dev, X_dev, stream): B and X (nrows x nvec each, ld = nvec) on the device for this call, X copied back
template <typename Fn>
int solve_block_from_host(cvr_handle *h, const void *B_host, void *X_host, int32_t nvec, Fn &&fn)
{
    HIP_TRY(hipSetDevice(h->device));
    const size_t bytes = h->vsz * (size_t)nvec * (size_t)h->info.nrows, slot = (bytes + 255) & ~(size_t)255;
    struct Mem { void *p = nullptr; ~Mem() { if (p) (void)hipFree(p); } } mem;
    HIP_TRY(hipMalloc(&mem.p, 2 * slot + 256));
    uint8_t *B = static_cast<uint8_t *>(mem.p), *X = B + slot;
    if (bytes) {
        HIP_TRY(hipMemcpyAsync(B, B_host, bytes, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(X, X_host, bytes, hipMemcpyHostToDevice, h->stream));
    }
    if (const int rc = fn(B, X, h->stream)) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(X_host, X, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return CVR_OK;
}

}  // namespace
}  // namespace krylov
}  // namespace cvrh
