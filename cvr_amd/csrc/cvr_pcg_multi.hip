// cvr_pcg_multi.hip -- the block-Jacobi object with several right-hand sides (include/cvr_amd.h: cvr_precond_apply_multi_device, the entry point of
// every kind whose table has apply_multi; cvr_pcg_multi_device and cvr_pcg_multi are cvr_cg_multi.hip's): Z = W R for row-major blocks of up to kSpmmBlock columns, on its own and in the form the batched solver enqueues.
//   precond_apply_multi_kernel   Z = W R
//   pcgm_apply_kernel            the same inside the solver, with per column the partial sums of r . z (set 1 of cgm_direction_kernel<T, true, LV>) and,
//                                at the start, P = Z
// The thread that owns rows e .. e + kPack - 1 of a single vector (CVR_KRYLOV_PACKETS) owns those rows of every column.  For a row i of block k it
// walks the block's columns j = 0 .. m - 1 once: W[i][j] is loaded once (the address the single apply reads, cvr_precond.h: apply_sums) and used for
// all columns, row k bs + j of R comes in sub-blocks of kPack<T> columns (CVR_CG_MULTI_SUBBLOCKS), and every column keeps its own fp64 sum in a
// register: s = t_0, then s += t_j, each product and addition rounded on its own -- per column the operations of apply_sums in its order, so column c
// of Z has the bits cvr_precond_apply_device gives for column c of R.
// The solver is cvr_cg_multi.hip's cg_multi_solve, which enqueues pcgm_apply_kernel through kBlockJacobiOps' cgm_apply (cvr_precond.h); this file launches
// no cgm_* kernel and holds no solve loop (cvr_cg_multi_kernels.h is included for the cells, the column walk and the constants).
#include "cvr_cg_multi_kernels.h"
#include "cvr_precond.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

// The fp64 sums of row il of block k for the columns of `live` (a sub-block without a live column is skipped, its sums stay 0; the other columns of
// a sub-block with one are computed and dropped by the caller).  RV: a whole sub-block of R is one 16-byte load.
template <typename T, bool RV>
__device__ __forceinline__ void apply_row_sums(const T *__restrict__ wt, int bs, const T *__restrict__ R, long long ldr, long long n, int nvec, uint32_t live,
                                               long long k, int il, double (&s)[kCols])
{
    const long long r0 = k * bs;
    const int       m = n - r0 < bs ? (int)(n - r0) : bs;
    const T        *w = wt + r0 * bs + il;
#pragma unroll
    for (int c = 0; c < kCols; c++) s[c] = 0;
    {
        const double wv = (double)w[0];
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            if (!(live >> cb & ((1u << cc) - 1))) continue;
            T rv[kPack<T>];
            load_pack<T, RV>(R, r0 * ldr + cb, cc, rv);
#pragma unroll
            for (int i = 0; i < kPack<T>; i++) s[cb + i] = wv * (double)rv[i];
        }
    }
    for (int j = 1; j < m; j++) {
        const double wv = (double)w[(long long)j * bs];
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            if (!(live >> cb & ((1u << cc) - 1))) continue;
            T rv[kPack<T>];
            load_pack<T, RV>(R, (r0 + j) * ldr + cb, cc, rv);
#pragma unroll
            for (int i = 0; i < kPack<T>; i++) s[cb + i] += wv * (double)rv[i];
        }
    }
}

// Z = W R.  RV, ZV: the sub-blocks of R / Z, the caller's blocks, take 16-byte packets (the leading dimension a multiple of kPack, 16-byte aligned)
template <typename T, bool RV, bool ZV>
__global__ __launch_bounds__(kThreads) void precond_apply_multi_kernel(const T *__restrict__ wt, int bs, const T *__restrict__ R, long long ldr, T *__restrict__ Z,
                                                                       long long ldz, long long n, int nvec)
{
    const uint32_t live = (1u << nvec) - 1;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        long long k = e / bs;
        int       il = (int)(e - k * bs);
#pragma unroll
        for (int jj = 0; jj < kPack<T>; jj++) {
            if (jj < cnt) {
                double s[kCols];
                apply_row_sums<T, RV>(wt, bs, R, ldr, n, nvec, live, k, il, s);
                CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
                    T zv[kPack<T>];
#pragma unroll
                    for (int i = 0; i < kPack<T>; i++) zv[i] = (T)s[cb + i];
                    store_cols<T, ZV>(Z, (e + jj) * ldz + cb, (1u << cc) - 1, zv);
                }
                if (++il == bs) { il = 0; k++; }
            }
        }
    }
}

// The solver's form on the library's blocks (ld = nvec; LV: nvec is a multiple of kPack): Z = W R and per column the partial sums of r . z, the terms
// double(r_i) * double(z_i) added in the thread that owns element i, in element order -- what cgm_update_kernel<T, true, ..> puts into set 1 of that
// column's partials.  START: before the cells exist; P = Z as well.  Otherwise a column whose cell holds a stop is not written, neither its Z nor its
// partials, and without a live column nothing is done (no workgroup of this kernel sets a stop).
template <typename T, bool START, bool LV>
__global__ __launch_bounds__(kThreads) void pcgm_apply_kernel(const T *__restrict__ wt, int bs, const T *__restrict__ R, T *__restrict__ Z, T *__restrict__ P,
                                                              long long n, int nvec, double *__restrict__ out, const CgCell *__restrict__ cells)
{
    __shared__ double sh[kCols][1][kWaves];
    uint32_t live = (1u << nvec) - 1;
    if constexpr (!START) {
        live = 0;
        for (int c = 0; c < nvec; c++) live |= (cells[c].stop ? 0u : 1u) << c;
        if (!live) return;
    }
    double acc[kCols][1] = {};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        long long k = e / bs;
        int       il = (int)(e - k * bs);
#pragma unroll
        for (int jj = 0; jj < kPack<T>; jj++) {
            if (jj < cnt) {
                double s[kCols];
                apply_row_sums<T, LV>(wt, bs, R, nvec, n, nvec, live, k, il, s);
                CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
                    const uint32_t m = live >> cb & ((1u << cc) - 1);
                    if (!m) continue;
                    T rv[kPack<T>], zv[kPack<T>];
                    load_pack<T, LV>(R, (e + jj) * nvec + cb, cc, rv);
#pragma unroll
                    for (int i = 0; i < kPack<T>; i++) {
                        zv[i] = (T)s[cb + i];
                        acc[cb + i][0] += (double)rv[i] * (double)zv[i];
                    }
                    store_cols<T, LV>(Z, (e + jj) * nvec + cb, m, zv);
                    if constexpr (START) store_cols<T, LV>(P, (e + jj) * nvec + cb, m, zv);
                }
                if (++il == bs) { il = 0; k++; }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < kCols; c++)
        if (c < nvec && (live >> c & 1u)) store_partials<1>(acc[c], out + (size_t)c * kSets * kBlocks + kBlocks, sh[c]);
}

template <typename T>
hipError_t launch_apply_multi(const cvr_precond *p, const void *R, int64_t ldr, void *Z, int64_t ldz, int32_t nvec, hipStream_t st)
{
    const bool rv = ((uintptr_t)R & 15u) == 0 && ldr % kPack<T> == 0, zv = ((uintptr_t)Z & 15u) == 0 && ldz % kPack<T> == 0;
    with_flags([&](auto RV, auto ZV) { launch(precond_apply_multi_kernel<T, RV, ZV>, st, static_cast<const T *>(p->d_w), (int)p->bs, static_cast<const T *>(R), (long long)ldr, static_cast<T *>(Z), (long long)ldz, (long long)p->n, (int)nvec); },
               rv, zv);
    return hipGetLastError();
}

}  // namespace

namespace cvrh {
namespace krylov {

template <typename T>
int block_jacobi_cgm_apply(const cvr_precond *pc, const T *R, T *Z, T *P, long long n, int nvec, bool lv, double *part, const void *cells, bool start, hipStream_t st, int *)
{
    with_flags([&](auto START, auto LV) { launch(pcgm_apply_kernel<T, START, LV>, st, static_cast<const T *>(pc->d_w), (int)pc->bs, R, Z, P, n, nvec, part, static_cast<const CgCell *>(cells)); },
               start, lv);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}
template int block_jacobi_cgm_apply<float>(const cvr_precond *, const float *, float *, float *, long long, int, bool, double *, const void *, bool, hipStream_t, int *);
template int block_jacobi_cgm_apply<double>(const cvr_precond *, const double *, double *, double *, long long, int, bool, double *, const void *, bool, hipStream_t, int *);

int block_jacobi_apply_multi(const cvr_precond *p, const void *R, int64_t ldr, void *Z, int64_t ldz, int32_t nvec, hipStream_t st)
{
    if (p->n == 0) return CVR_OK;
    HIP_TRY(p->is_f32 ? launch_apply_multi<float>(p, R, ldr, Z, ldz, nvec, st) : launch_apply_multi<double>(p, R, ldr, Z, ldz, nvec, st));
    return CVR_OK;
}

}  // namespace krylov
}  // namespace cvrh

extern "C" {

int cvr_precond_apply_multi_device(const cvr_precond *p, const void *R_dev, int64_t ldr, void *Z_dev, int64_t ldz, int32_t nvec, void *stream)
{
    if (!p || !R_dev || !Z_dev) return fail(CVR_ERR_INVALID, "null argument");
    if (R_dev == Z_dev) return fail(CVR_ERR_INVALID, "cvr_precond_apply_multi_device: R and Z are the same block");
    if (nvec < 1 || nvec > kCols) return fail(CVR_ERR_INVALID, "nvec = %d: 1 to %d columns per call", nvec, kCols);
    if (ldr < nvec || ldz < nvec) return fail(CVR_ERR_INVALID, "ldr = %lld, ldz = %lld: each must be >= nvec = %d", (long long)ldr, (long long)ldz, nvec);
    if (const int rc = check_multi(p, nvec, "cvr_precond_apply_multi_device")) return rc;
    if (p->n == 0) return CVR_OK;
    HIP_TRY(hipSetDevice(p->device));
    return p->ops->apply_multi(p, R_dev, ldr, Z_dev, ldz, nvec, (hipStream_t)stream);
}

}  // extern "C"
