// cvr_amg_block.hip -- the AMG object for blocks of right-hand sides (include/cvr_amd.h: cvr_precond_amg_block, cvr_precond_amg_block_info): one
// V-cycle that carries up to K vectors through every level.  The object is cvr_amg.hip's, built by its constructor with Amg::width = K (cvr_amg_dev.h):
// the same hierarchy, handles of the plain layout (cvr_options.nvec = K), every buffer a row-major block of K columns with ld = K whose pad row n is
// never written.  A k-wide cycle issues the launches of a single-vector one and reads every level's image, dinv, agg and winv once for all columns.
//   amgb_copy_kernel       rows of one leading dimension into rows of another: R (ldr) -> r_0 (K), z_0 (K) -> Z (ldz)
//   amgb_first_kernel      z = dinv .* r                           amgb_smooth_kernel     z += dinv .* (r - q)
//   amgb_restrict_kernel   a lane per aggregate, a sum per column  amgb_prolong_kernel    z += scale * zc[agg]
//   amgb_residual_kernel   t = r - q                               amgb_correct_kernel    z += scale * e
//   amgb_dense_kernel      the coarsest level's z = W r, one workgroup, thread i owns row i of all columns
//   amgb_rz_kernel         inside cvr_pcg_multi_device: Z = z_0, per column the partial sums of r . z and, at the start, P = Z; live columns only
// A thread owns a row: its K values lie side by side, so neighbouring lanes read neighbouring addresses, and a scalar of the row (dinv_i, agg_i, a
// W_ij) is loaded once for all columns.  The columns are walked in sub-blocks of kPack<T> (CVR_CG_MULTI_SUBBLOCKS, unrolled over the 8 there can be:
// a column's sum is a register); VEC: K is a multiple of kPack<T>, so every sub-block of the object's buffers is one 16-byte packet (a packet's
// columns >= nvec are computed and stored with the rest: they are the buffer's own, written before they are read by a wider call).  nvec is a
// runtime argument.  Per column the arithmetic is the single-vector kernels' (cvr_amg.hip), operation for operation: fp64, each operation rounded on
// its own (the file is compiled without contraction), one rounding to T per stored value -- so column c of a block apply has the bits of
// cvr_precond_apply_device on column c, given that a column of launch_spmm's product has cvr_spmv_device's bits on the same image.
// Products: K = 1: run_spmv (the handles have the default layout); K >= 2: launch_spmm on the plain image with ld = K, inside handle_enter /
// handle_leave for a mutable level-0 handle -- cvr_spmm_device's path.
#include "cvr_cg_multi_kernels.h"
#include "cvr_precond.h"
#include "cvr_amg_dev.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

// how many values of a sub-block of the object's buffers a thread moves: the whole packet, or the cc columns that exist
template <typename T, bool VEC>
__device__ __forceinline__ int moved(int cc)
{
    return VEC ? kPack<T> : cc;
}

// dst (ldd) = src (lds), rows 0 .. n - 1, columns 0 .. nvec - 1 and nothing else.  SV, DV: the block takes 16-byte packets (base and ld)
template <typename T, bool SV, bool DV>
__global__ __launch_bounds__(kThreads) void amgb_copy_kernel(const T *__restrict__ src, long long lds, T *__restrict__ dst, long long ldd, long long n, int nvec)
{
    CVR_AMG_ELEMENTS(i, n) {
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            T v[kPack<T>];
            load_pack<T, SV>(src, i * lds + cb, cc, v);
            store_pack<T, DV>(dst, i * ldd + cb, cc, v);
        }
    }
}

// z_ic = T(dinv_i * r_ic)
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void amgb_first_kernel(const T *__restrict__ dinv, const T *__restrict__ r, T *__restrict__ z, long long n, int K, int nvec)
{
    CVR_AMG_ELEMENTS(i, n) {
        const double d = (double)dinv[i];
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            T rv[kPack<T>], zv[kPack<T>];
            load_pack<T, VEC>(r, i * K + cb, moved<T, VEC>(cc), rv);
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) zv[j] = (T)(d * (double)rv[j]);
            store_pack<T, VEC>(z, i * K + cb, moved<T, VEC>(cc), zv);
        }
    }
}

// behind Q = A Z: z_ic = T(z_ic + dinv_i * (r_ic - q_ic))
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void amgb_smooth_kernel(const T *__restrict__ dinv, const T *__restrict__ r, const T *__restrict__ q, T *__restrict__ z, long long n, int K,
                                                               int nvec)
{
    CVR_AMG_ELEMENTS(i, n) {
        const double d = (double)dinv[i];
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            T rv[kPack<T>], qv[kPack<T>], zv[kPack<T>];
            load_pack<T, VEC>(r, i * K + cb, moved<T, VEC>(cc), rv);
            load_pack<T, VEC>(q, i * K + cb, moved<T, VEC>(cc), qv);
            load_pack<T, VEC>(z, i * K + cb, moved<T, VEC>(cc), zv);
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) zv[j] = (T)((double)zv[j] + d * ((double)rv[j] - (double)qv[j]));
            store_pack<T, VEC>(z, i * K + cb, moved<T, VEC>(cc), zv);
        }
    }
}

// behind Q = A Z: rc_Ic = T(+0 + (r_ic - q_ic) + ..) over the rows of aggregate I, ascending; a lane per aggregate, a sum per column
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void amgb_restrict_kernel(const int64_t *__restrict__ mrp, const int32_t *__restrict__ mem, const T *__restrict__ r, const T *__restrict__ q,
                                                                 T *__restrict__ rc, long long nc, int K, int nvec)
{
    CVR_AMG_ELEMENTS(I, nc) {
        double s[kCols] = {};
        for (long long m = mrp[I]; m < mrp[I + 1]; m++) {
            const long long i = mem[m];
            CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
                T rv[kPack<T>], qv[kPack<T>];
                load_pack<T, VEC>(r, i * K + cb, moved<T, VEC>(cc), rv);
                load_pack<T, VEC>(q, i * K + cb, moved<T, VEC>(cc), qv);
#pragma unroll
                for (int j = 0; j < kPack<T>; j++) s[cb + j] = s[cb + j] + ((double)rv[j] - (double)qv[j]);
            }
        }
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            T v[kPack<T>];
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) v[j] = (T)s[cb + j];
            store_pack<T, VEC>(rc, I * K + cb, moved<T, VEC>(cc), v);
        }
    }
}

// z_ic = T(z_ic + scale * zc[agg_i][c]): the gather of a K-wide row
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void amgb_prolong_kernel(const int32_t *__restrict__ agg, const T *__restrict__ zc, T *__restrict__ z, long long n, double scale, int K, int nvec)
{
    CVR_AMG_ELEMENTS(i, n) {
        const long long I = agg[i];
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            T cv[kPack<T>], zv[kPack<T>];
            load_pack<T, VEC>(zc, I * K + cb, moved<T, VEC>(cc), cv);
            load_pack<T, VEC>(z, i * K + cb, moved<T, VEC>(cc), zv);
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) zv[j] = (T)((double)zv[j] + scale * (double)cv[j]);
            store_pack<T, VEC>(z, i * K + cb, moved<T, VEC>(cc), zv);
        }
    }
}

// behind Q = A Z: t_ic = T(r_ic - q_ic), the input of R's product
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void amgb_residual_kernel(const T *__restrict__ r, const T *__restrict__ q, T *__restrict__ t, long long n, int K, int nvec)
{
    CVR_AMG_ELEMENTS(i, n) {
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            T rv[kPack<T>], qv[kPack<T>], tv[kPack<T>];
            load_pack<T, VEC>(r, i * K + cb, moved<T, VEC>(cc), rv);
            load_pack<T, VEC>(q, i * K + cb, moved<T, VEC>(cc), qv);
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) tv[j] = (T)((double)rv[j] - (double)qv[j]);
            store_pack<T, VEC>(t, i * K + cb, moved<T, VEC>(cc), tv);
        }
    }
}

// behind E = P Zc: z_ic = T(z_ic + scale * e_ic)
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void amgb_correct_kernel(const T *__restrict__ e, T *__restrict__ z, long long n, double scale, int K, int nvec)
{
    CVR_AMG_ELEMENTS(i, n) {
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            T ev[kPack<T>], zv[kPack<T>];
            load_pack<T, VEC>(e, i * K + cb, moved<T, VEC>(cc), ev);
            load_pack<T, VEC>(z, i * K + cb, moved<T, VEC>(cc), zv);
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) zv[j] = (T)((double)zv[j] + scale * (double)ev[j]);
            store_pack<T, VEC>(z, i * K + cb, moved<T, VEC>(cc), zv);
        }
    }
}

// the directly solved coarsest level, n <= CVR_AMG_MAX_COARSE: z_ic = T(t_0 + t_1 + ..), t_j = W_ij * r_jc, left to right from t_0 per column.
// Thread i owns row i of all columns and reads W_ji (W is symmetric bit for bit), each value once for all columns; row j of r is the same address in
// every lane
template <typename T, bool VEC>
__global__ __launch_bounds__(CVR_AMG_MAX_COARSE) void amgb_dense_kernel(const T *__restrict__ w, const T *__restrict__ r, T *__restrict__ z, int n, int K, int nvec)
{
    const int i = threadIdx.x;
    if (i >= n) return;
    double s[kCols] = {};
    {
        const double wv = (double)w[i];
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            T rv[kPack<T>];
            load_pack<T, VEC>(r, cb, moved<T, VEC>(cc), rv);
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) s[cb + j] = wv * (double)rv[j];
        }
    }
    for (int k = 1; k < n; k++) {
        const double wv = (double)w[(size_t)k * n + i];
        CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
            T rv[kPack<T>];
            load_pack<T, VEC>(r, (long long)k * K + cb, moved<T, VEC>(cc), rv);
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) s[cb + j] = s[cb + j] + wv * (double)rv[j];
        }
    }
    CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
        T v[kPack<T>];
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) v[j] = (T)s[cb + j];
        store_pack<T, VEC>(z, (long long)i * K + cb, moved<T, VEC>(cc), v);
    }
}

// The solver's last launch of an apply, on the solvers' grid: Z = zo (the object's z_0, ld = K) on the solver's blocks (ld = nvec; LV: they take
// 16-byte packets) and per column the partial sums of r . z, the terms double(r_i) * double(z_i) added in the thread that owns element i, in element
// order -- precond_rz_kernel's sum, column by column, into set 1 of that column's partials.  START: before the cells exist; P = Z as well.
// Otherwise a column whose cell holds a stop is not written, neither its Z nor its partials, and without a live column nothing is done (no workgroup
// of this kernel sets a stop).
template <typename T, bool START, bool LV, bool VEC>
__global__ __launch_bounds__(kThreads) void amgb_rz_kernel(const T *__restrict__ R, const T *__restrict__ zo, int K, T *__restrict__ Z, T *__restrict__ P, long long n, int nvec,
                                                           double *__restrict__ out, const CgCell *__restrict__ cells)
{
    __shared__ double sh[kCols][1][kWaves];
    uint32_t          live = (1u << nvec) - 1;
    if constexpr (!START) {
        live = 0;
        for (int c = 0; c < nvec; c++) live |= (cells[c].stop ? 0u : 1u) << c;
        if (!live) return;
    }
    double acc[kCols][1] = {};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
#pragma unroll
        for (int jj = 0; jj < kPack<T>; jj++) {
            if (jj < cnt) {
                const long long row = e + jj;
                CVR_CG_MULTI_SUBBLOCKS(T, cb, cc) {
                    const uint32_t m = live >> cb & ((1u << cc) - 1);
                    if (!m) continue;
                    T rv[kPack<T>], zv[kPack<T>];
                    load_pack<T, LV>(R, row * nvec + cb, cc, rv);
                    load_pack<T, VEC>(zo, row * K + cb, moved<T, VEC>(cc), zv);
#pragma unroll
                    for (int i = 0; i < kPack<T>; i++) acc[cb + i][0] += (double)rv[i] * (double)zv[i];
                    store_cols<T, LV>(Z, row * nvec + cb, m, zv);
                    if constexpr (START) store_cols<T, LV>(P, row * nvec + cb, m, zv);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < kCols; c++)
        if (c < nvec && (live >> c & 1u)) store_partials<1>(acc[c], out + (size_t)c * kSets * kBlocks + kBlocks, sh[c]);
}

// ---- the host half

// the object's buffers take 16-byte packets: K values of T fill whole packets
template <typename T>
bool packets(const Amg *a)
{
    return a->width % kPack<T> == 0;
}

// Y = A X for nvec columns of two of the object's blocks
int product(cvr_handle *h, const void *X, void *Y, int K, int nvec, hipStream_t st)
{
    if (K == 1) {
        HIP_TRY(run_spmv(h, X, Y, st));
        return CVR_OK;
    }
    if (h->d_map) HIP_TRY(handle_enter(h, st));          // (a mutable handle's image: ordered with its updates, as cvr_spmm_device)
    HIP_TRY(cvr::launch_spmm(h->parts[0].img, X, K, Y, K, nvec, st));
    if (h->d_map) HIP_TRY(handle_leave(h, st));
    return CVR_OK;
}

template <typename T>
int smooth_more(const Amg *a, const AmgLevel &l, int times, int nvec, hipStream_t st)
{
    const int K = a->width;
    for (int k = 0; k < times; k++) {
        if (const int rc = product(l.h, l.d_z, l.d_q, K, nvec, st)) return rc;
        with_flags([&](auto VEC) { launch_level(amgb_smooth_kernel<T, VEC>, l.n, st, static_cast<const T *>(l.d_dinv), static_cast<const T *>(l.d_r), static_cast<const T *>(l.d_q), static_cast<T *>(l.d_z), (long long)l.n, K, nvec); },
                   packets<T>(a));
    }
    return CVR_OK;
}

// the cycle of cvr_amg.hip's enqueue_cycle for the nvec columns that lie in r_0: z_0 holds the result
template <typename T>
int enqueue_block_cycle(const cvr_precond *pc, int nvec, hipStream_t st)
{
    const Amg   *a = pc->amg;
    const size_t L = a->lv.size();
    const int    sweeps = a->H.opt.sweeps, K = a->width;
    const bool   vec = packets<T>(a);
    const double scale = a->H.opt.coarse_scale;
    for (size_t l = 0; l + 1 < L; l++) {
        const AmgLevel &f = a->lv[l], &c = a->lv[l + 1];
        with_flags([&](auto VEC) { launch_level(amgb_first_kernel<T, VEC>, f.n, st, static_cast<const T *>(f.d_dinv), static_cast<const T *>(f.d_r), static_cast<T *>(f.d_z), (long long)f.n, K, nvec); }, vec);
        if (const int rc = smooth_more<T>(a, f, sweeps - 1, nvec, st)) return rc;
        if (const int rc = product(f.h, f.d_z, f.d_q, K, nvec, st)) return rc;
        if (a->H.smoothed) {
            with_flags([&](auto VEC) { launch_level(amgb_residual_kernel<T, VEC>, f.n, st, static_cast<const T *>(f.d_r), static_cast<const T *>(f.d_q), static_cast<T *>(f.d_t), (long long)f.n, K, nvec); }, vec);
            if (const int rc = product(f.hr, f.d_t, c.d_r, K, nvec, st)) return rc;
        } else
            with_flags([&](auto VEC) { launch_level(amgb_restrict_kernel<T, VEC>, f.nc, st, static_cast<const int64_t *>(f.d_mrp), static_cast<const int32_t *>(f.d_mem), static_cast<const T *>(f.d_r), static_cast<const T *>(f.d_q), static_cast<T *>(c.d_r), (long long)f.nc, K, nvec); },
                       vec);
    }
    const AmgLevel &last = a->lv[L - 1];
    if (a->H.coarse_direct)
        with_flags([&](auto VEC) { hipLaunchKernelGGL((amgb_dense_kernel<T, VEC>), dim3(1), dim3(CVR_AMG_MAX_COARSE), 0, st, static_cast<const T *>(a->d_winv), static_cast<const T *>(last.d_r), static_cast<T *>(last.d_z), (int)last.n, K, nvec); },
                   vec);
    else {
        with_flags([&](auto VEC) { launch_level(amgb_first_kernel<T, VEC>, last.n, st, static_cast<const T *>(last.d_dinv), static_cast<const T *>(last.d_r), static_cast<T *>(last.d_z), (long long)last.n, K, nvec); }, vec);
        if (const int rc = smooth_more<T>(a, last, 2 * sweeps - 1, nvec, st)) return rc;
    }
    for (size_t l = L - 1; l-- > 0;) {
        const AmgLevel &f = a->lv[l], &c = a->lv[l + 1];
        if (a->H.smoothed) {
            if (const int rc = product(f.hp, c.d_z, f.d_e, K, nvec, st)) return rc;
            with_flags([&](auto VEC) { launch_level(amgb_correct_kernel<T, VEC>, f.n, st, static_cast<const T *>(f.d_e), static_cast<T *>(f.d_z), (long long)f.n, scale, K, nvec); }, vec);
        } else
            with_flags([&](auto VEC) { launch_level(amgb_prolong_kernel<T, VEC>, f.n, st, static_cast<const int32_t *>(f.d_agg), static_cast<const T *>(c.d_z), static_cast<T *>(f.d_z), (long long)f.n, scale, K, nvec); }, vec);
        if (const int rc = smooth_more<T>(a, f, sweeps, nvec, st)) return rc;
    }
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

// r_0 = the first nvec columns of R (ld = ldr)
template <typename T>
int copy_in(const cvr_precond *pc, const T *R, long long ldr, int nvec, hipStream_t st)
{
    const Amg *a = pc->amg;
    const bool sv = ((uintptr_t)R & 15u) == 0 && ldr % kPack<T> == 0;
    with_flags([&](auto SV, auto DV) { launch_level(amgb_copy_kernel<T, SV, DV>, pc->n, st, R, ldr, static_cast<T *>(a->lv[0].d_r), (long long)a->width, (long long)pc->n, nvec); }, sv, packets<T>(a));
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

template <typename T>
int apply_multi(const cvr_precond *pc, const T *R, long long ldr, T *Z, long long ldz, int nvec, hipStream_t st)
{
    const Amg *a = pc->amg;
    if (const int rc = copy_in<T>(pc, R, ldr, nvec, st)) return rc;
    if (const int rc = enqueue_block_cycle<T>(pc, nvec, st)) return rc;
    const bool dv = ((uintptr_t)Z & 15u) == 0 && ldz % kPack<T> == 0;
    with_flags([&](auto SV, auto DV) { launch_level(amgb_copy_kernel<T, SV, DV>, pc->n, st, static_cast<const T *>(a->lv[0].d_z), (long long)a->width, Z, ldz, (long long)pc->n, nvec); }, packets<T>(a), dv);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

int amg_block_apply_multi(const cvr_precond *p, const void *R, int64_t ldr, void *Z, int64_t ldz, int32_t nvec, hipStream_t st)
{
    if (!p->amg || p->n == 0) return CVR_OK;
    return p->is_f32 ? apply_multi<float>(p, static_cast<const float *>(R), ldr, static_cast<float *>(Z), ldz, nvec, st)
                     : apply_multi<double>(p, static_cast<const double *>(R), ldr, static_cast<double *>(Z), ldz, nvec, st);
}

// batched CG's apply: R, Z and P are the solver's blocks (ld = nvec, 256-byte aligned)
template <typename T>
int amg_block_cgm_apply(const cvr_precond *pc, const T *R, T *Z, T *P, long long n, int nvec, bool lv, double *part, const void *cells, bool start, hipStream_t st, int *spmvs)
{
    const Amg *a = pc->amg;
    if (!a || pc->n == 0) return CVR_OK;
    if (const int rc = copy_in<T>(pc, R, nvec, nvec, st)) return rc;
    if (const int rc = enqueue_block_cycle<T>(pc, nvec, st)) return rc;
    if (spmvs) *spmvs += a->products;
    with_flags([&](auto START, auto LV, auto VEC) { launch(amgb_rz_kernel<T, START, LV, VEC>, st, R, static_cast<const T *>(a->lv[0].d_z), (int)a->width, Z, P, n, nvec, part, static_cast<const CgCell *>(cells)); },
               start, lv, packets<T>(a));
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

}  // namespace

namespace cvrh {
namespace krylov {

PrecondOps kAmgBlockOps = {kPrecondAmg,          "AMG",
                           amg_apply_any,        amg_release,
                           amg_cg_apply<float>,  amg_cg_apply<double>,
                           amg_block_apply_multi, amg_block_cgm_apply<float>,
                           amg_block_cgm_apply<double>};

}  // namespace krylov
}  // namespace cvrh

extern "C" {

int cvr_precond_amg_block(cvr_precond **out, cvr_handle *h, const cvr_csr_view *csr, const cvr_amg_options *opt, int32_t setup, double omega, int32_t nvec, void *stream)
{
    if (!out || !h || !csr) return fail(CVR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (setup < CVR_AMG_SETUP_PLAIN || setup > CVR_AMG_SETUP_MIS2)
        return fail(CVR_ERR_INVALID, "cvr_precond_amg_block: setup = %d: must be CVR_AMG_SETUP_PLAIN (0), CVR_AMG_SETUP_SMOOTHED (1) or CVR_AMG_SETUP_MIS2 (2)", setup);
    if (nvec < 1 || nvec > kCols) return fail(CVR_ERR_INVALID, "cvr_precond_amg_block: nvec = %d: must be 1 .. %d", nvec, kCols);
    return amg_construct(out, h, csr, opt, setup, setup == CVR_AMG_SETUP_PLAIN ? 0.0 : omega, nvec, stream);
}

int cvr_precond_amg_block_info(const cvr_precond *p, cvr_amg_block_info *info)
{
    if (!p || !info) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondAmg || !p->amg) return fail(CVR_ERR_INVALID, "cvr_precond_amg_block_info: the preconditioner is of kind %d, not an AMG object (kind %d)", p->kind, kPrecondAmg);
    if (p->amg->width == 0) return fail(CVR_ERR_INVALID, "cvr_precond_amg_block_info: the preconditioner was not built by cvr_precond_amg_block");
    memset(info, 0, sizeof(*info));
    info->nvec = p->amg->width;
    info->setup = p->amg->setup;
    info->buffer_bytes = p->amg->buffer_bytes;
    return CVR_OK;
}

}  // extern "C"
