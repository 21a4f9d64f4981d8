// cvr_pcg_multi.hip -- the block-Jacobi object with several right-hand sides (include/cvr_amd.h: cvr_precond_apply_multi_device, cvr_pcg_multi_device,
// cvr_pcg_multi): Z = W R for row-major blocks of up to kSpmmBlock columns, and cvr_cg_multi.hip's solver with that apply in place of the diagonal.
//   precond_apply_multi_kernel   Z = W R
//   pcgm_apply_kernel            the same inside the solver, with per column the partial sums of r . z (set 1 of cgm_direction_kernel<T, true, LV>) and,
//                                at the start, P = Z
// The thread that owns rows e .. e + kPack - 1 of a single vector (CVR_KRYLOV_PACKETS) owns those rows of every column.  For a row i of block k it
// walks the block's columns j = 0 .. m - 1 once: W[i][j] is loaded once (the address the single apply reads, cvr_precond.h: apply_sums) and used for
// all columns, row k bs + j of R comes in sub-blocks of kPack<T> columns (CVR_CG_MULTI_SUBBLOCKS), and every column keeps its own fp64 sum in a
// register: s = t_0, then s += t_j, each product and addition rounded on its own -- per column the operations of apply_sums in its order, so column c
// of Z has the bits cvr_precond_apply_device gives for column c of R.
// The solver is cvr_cg_multi.hip's with four vector launches per step beside the k-wide product: cgm_pq_kernel, cgm_update_kernel<T, false, LV, AL>,
// pcgm_apply_kernel<T, false, LV>, cgm_direction_kernel<T, true, LV> (cvr_cg_multi_kernels.h: the kernels cvr_cg_multi_device runs, unchanged), as
// cvr_precond.hip's pcg_solve is cvr_cg.hip's: column j gets bit for bit what cvr_pcg_device gives for b = B[:, j], x0 = X[:, j].
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
hipError_t launch_apply(const Workspace<T> &w, const Call<T> &c, const cvr_precond *pc, bool start, hipStream_t st)
{
    with_flags([&](auto START, auto LV) { launch(pcgm_apply_kernel<T, START, LV>, st, static_cast<const T *>(pc->d_w), (int)pc->bs, (const T *)w.r, w.z, w.p, c.n, c.nvec, w.part, (const CgCell *)w.cells); },
               start, c.lv);
    return hipGetLastError();
}

// the four vector launches of step k (the product Q = A P is enqueued in front of them)
template <typename T>
hipError_t launch_step(const Workspace<T> &w, const Call<T> &c, const cvr_precond *pc, int k, hipStream_t st)
{
    with_flags([&](auto LV) { launch(cgm_pq_kernel<T, LV>, st, w.p, w.q, c.n, c.nvec, w.part_pq, w.cells); }, c.lv);
    with_flags([&](auto LV, auto AL) { launch(cgm_update_kernel<T, false, LV, AL>, st, c.x, c.ldx, w.r, w.z, w.p, w.q, (const T *)nullptr, c.n, c.nvec, w.part_pq, w.part, w.cells, k); },
               c.lv, c.al);
    if (const hipError_t e = launch_apply(w, c, pc, false, st)) return e;
    with_flags([&](auto LV) { launch(cgm_direction_kernel<T, true, LV>, st, w.p, w.z, c.n, c.nvec, w.part, w.cells, k, c.rtol); }, c.lv);
    return hipGetLastError();
}

// cvr_cg_multi.hip's cg_multi_solve with W in place of minv
template <typename T>
int pcg_multi_solve(cvr_handle *h, const cvr_precond *pc, bool single, const T *B, int64_t ldb, T *X, int64_t ldx, int32_t nvec, const cvr_cg_options *opt,
                    cvr_cg_result *res, hipStream_t st)
{
    const long long n = h->info.nrows;
    Call<T>         c{B, ldb, X, ldx, nullptr, n, nvec, false, false, opt->rtol};
    c.lv = nvec % kPack<T> == 0;
    c.al = (((uintptr_t)B | (uintptr_t)X) & 15u) == 0 && ldb % kPack<T> == 0 && ldx % kPack<T> == 0;

    Arena        a;
    const size_t op = a.add(x_ext_bytes(h, nvec)), oq = a.add(y_ext_bytes(h, nvec)), orr = a.add(y_ext_bytes(h, nvec)), oz = a.add(vec_bytes(h, nvec));
    const size_t opq = a.add(sizeof(double) * kCols * kBlocks), opart = a.add(sizeof(double) * kCols * kSets * kBlocks), ocells = a.add(sizeof(CgCell) * kCols);
    HIP_TRY(a.alloc());
    const Workspace<T> w{a.at<T>(op), a.at<T>(oq), a.at<T>(orr), a.at<T>(oz), a.at<double>(opq), a.at<double>(opart), a.at<CgCell>(ocells)};
    if (const int rc = a.begin(st)) return rc;

    // P = X0 for the moment (with its zero row), Q = A X0; then R, P = R and the sums r . r and b . b; Z = W R, P = Z and r . z; the cells
    launch(cgm_start_kernel<T>, st, X, (long long)ldx, w.p, n, nvec);
    HIP_TRY(hipGetLastError());
    if (const int rc = product(h, single, w, nvec, st)) return rc;
    int spmms = 1;
    with_flags([&](auto LV, auto AL) { launch(cgm_init_kernel<T, false, LV, AL>, st, c.b, c.ldb, (const T *)nullptr, w.q, w.r, w.z, w.p, c.n, c.nvec, w.part); }, c.lv, c.al);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_apply(w, c, pc, true, st));
    hipLaunchKernelGGL(cgm_check_kernel, dim3(1), dim3(kThreads), 0, st, w.part, 1, opt->rtol, nvec, w.cells);
    HIP_TRY(hipGetLastError());

    CgCell    cells[kCols] = {};
    const int rc = run_batches(
        opt,
        [&](int k) -> int {
            if (const int rc = product(h, single, w, nvec, st)) return rc;
            spmms++;
            HIP_TRY(launch_step(w, c, pc, k, st));
            return CVR_OK;
        },
        [&](int, bool *stopped) -> int {          // stopped: every column has
            if (const int rc = read_cell(cells, w.cells, sizeof(CgCell) * (size_t)nvec, st)) return rc;
            *stopped = true;
            for (int j = 0; j < nvec; j++) *stopped = *stopped && cells[j].stop;
            return CVR_OK;
        });
    if (rc) return rc;
    uint32_t zero = 0;
    for (int j = 0; j < nvec; j++) if (cells[j].zero_x) zero |= 1u << j;
    if (zero && n) {
        launch(cgm_zero_kernel<T>, st, X, (long long)ldx, n, nvec, zero);
        HIP_TRY(hipGetLastError());
    }
    double seconds = 0;
    if (const int rc = a.seconds(st, &seconds)) return rc;
    for (int j = 0; j < nvec; j++) fill_result(&res[j], cells[j].iters, cells[j].status, spmms, cells[j].rnorm, cells[j].bnorm, seconds);
    return CVR_OK;
}

// what both entry points check before any device work and before the handle is looked at
int check_pcg_multi_args(const void *h, const cvr_precond *p, const void *B, const void *X, int32_t nvec, int64_t ldb, int64_t ldx, const cvr_cg_options *opt,
                         const cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, B, X, opt, res)) return rc;
    if (const int rc = check_precond_args(p, opt, "cvr_pcg_multi")) return rc;
    return check_block_args(nvec, ldb, ldx);
}

// ... and what they ask of the handle and of the pair
int check_pcg_multi_handle(const cvr_handle *h, const cvr_precond *p, int32_t nvec, bool single)
{
    if (const int rc = check_handle(h, nvec, single, "cvr_pcg_multi")) return rc;
    if (const int rc = check_precond_pair(h, p, "cvr_pcg_multi")) return rc;
    return check_block_jacobi(p, "cvr_pcg_multi");
}

// behind the checks
int pcg_multi_device(cvr_handle *h, const cvr_precond *p, bool single, const void *B, int64_t ldb, void *X, int64_t ldx, int32_t nvec, const cvr_cg_options *opt,
                     cvr_cg_result *res, hipStream_t st)
{
    Range range("cvr_pcg_multi_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) {
        return pcg_multi_solve(h, p, single, static_cast<const decltype(t) *>(B), ldb, static_cast<decltype(t) *>(X), ldx, nvec, opt, res, st);
    });
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

extern "C" {

int cvr_precond_apply_multi_device(const cvr_precond *p, const void *R_dev, int64_t ldr, void *Z_dev, int64_t ldz, int32_t nvec, void *stream)
{
    if (!p || !R_dev || !Z_dev) return fail(CVR_ERR_INVALID, "null argument");
    if (R_dev == Z_dev) return fail(CVR_ERR_INVALID, "cvr_precond_apply_multi_device: R and Z are the same block");
    if (nvec < 1 || nvec > kCols) return fail(CVR_ERR_INVALID, "nvec = %d: 1 to %d columns per call", nvec, kCols);
    if (ldr < nvec || ldz < nvec) return fail(CVR_ERR_INVALID, "ldr = %lld, ldz = %lld: each must be >= nvec = %d", (long long)ldr, (long long)ldz, nvec);
    if (const int rc = check_block_jacobi(p, "cvr_precond_apply_multi_device")) return rc;
    if (p->n == 0) return CVR_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(p->is_f32 ? launch_apply_multi<float>(p, R_dev, ldr, Z_dev, ldz, nvec, (hipStream_t)stream)
                      : launch_apply_multi<double>(p, R_dev, ldr, Z_dev, ldz, nvec, (hipStream_t)stream));
    return CVR_OK;
}

int cvr_pcg_multi_device(cvr_handle *h, const cvr_precond *p, const void *B_dev, int64_t ldb, void *X_dev, int64_t ldx, int32_t nvec, const cvr_cg_options *opt,
                         cvr_cg_result *res, void *stream)
{
    if (const int rc = check_pcg_multi_args(h, p, B_dev, X_dev, nvec, ldb, ldx, opt, res)) return rc;
    const bool single = nvec == 1 && ldb == 1 && ldx == 1;
    if (const int rc = check_pcg_multi_handle(h, p, nvec, single)) return rc;
    return pcg_multi_device(h, p, single, B_dev, ldb, X_dev, ldx, nvec, opt, res, (hipStream_t)stream);
}

int cvr_pcg_multi(cvr_handle *h, const cvr_precond *p, const void *B_host, void *X_host, int32_t nvec, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_pcg_multi_args(h, p, B_host, X_host, nvec, nvec, nvec, opt, res)) return rc;
    if (const int rc = check_pcg_multi_handle(h, p, nvec, nvec == 1)) return rc;
    return solve_block_from_host(h, B_host, X_host, nvec, [&](const void *B, void *X, hipStream_t st) { return pcg_multi_device(h, p, nvec == 1, B, nvec, X, nvec, nvec, opt, res, st); });
}

}  // extern "C"
