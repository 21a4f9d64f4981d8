// cvr_fsai.hip -- the factorised sparse approximate inverse (Kolotilina-Yeremin), the fourth kind of cvr_precond (include/cvr_amd.h: cvr_precond_fsai,
// cvr_precond_fsai_info, cvr_precond_fsai_export; the host twin cvr_fsai_factor_host: cvr_fsai_host.cpp).  For a symmetric positive definite A,
// M^-1 = W^T D^-1 W with W unit lower triangular on the pattern of A's lower triangle (at most CVR_FSAI_MAX_ROW entries a row): row i of W solves the
// small dense system A(P, P) w = e_last over the row's pattern P.  The apply z = Wb^T (Wa r), Wb = D^-1 Wa, is two products on the SpMV path, so its
// cost does not depend on the level structure of a triangular sweep.
//   Set-up, fsai_factor_kernel: G = lanes_per_row lanes of one wavefront per row (the power of two from the largest m up, 4 .. 64), 64 / G rows per
//     wavefront, rows dealt to wavefronts by a grid-stride loop.  The m x m matrix S of a row lives in LDS, its lower triangle gathered from A by
//     binary search in row p_a; the right-looking LDL^T keeps s_a = S[a][k] where it is and puts l_ak into the mirrored place (k, a); the back
//     substitution keeps w_a on the diagonal (a, a).  The lanes of a group split the (a, b) pairs of the gather, for each k the divisions and the
//     columns of the trailing update, for each b the w updates; every element has one update order (ascending k, descending b), so the bits do not
//     depend on G or on the mapping.  Synchronisation stays inside the wavefront (wave_sync: LDS fence + wave barrier); every loop that holds one has
//     the wavefront's trip count (the largest m of its rows).  A bad pivot is an atomicMin of the row number into one device word.
//   Object: two handles of its own, (W pattern, Wa) and (W pattern, Wb) with transpose = 1, both from device arrays with the default options, and
//     three buffers: xin (the first product's input), t (its output and the second product's input: its pad slot is zeroed behind the first product,
//     whose dump slot it is -- what cvr_lsqr.hip does with u^), zo (the second product's output).
//   Apply: precond_copy_in_kernel (xin = r) | Wa's product | Wb^T's product | precond_copy_out_kernel (z = zo), or inside cvr_pcg_device
//     precond_rz_kernel in its place (z = zo with the partial sums of r . z and, at the start, p = z; nothing behind a stop): cvr_precond.h's.
// (The reference has no solver and no preconditioner: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_cg_kernels.h"
#include "cvr_precond.h"
#include "cvr_fsai.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace cvrh {
namespace krylov {

struct Fsai {
    int64_t              nnz = 0, truncated = 0;
    int32_t              max_row = 0, G = 4;
    std::vector<int64_t> wrp;          // W's pattern, on the host (the handles hold their own copies)
    std::vector<int32_t> wci;
    void                *d_wa = nullptr, *d_wb = nullptr;          // nnz values of T each
    cvr_handle          *ha = nullptr, *hb = nullptr;              // Wa; Wb^T
    void                *d_xin = nullptr, *d_t = nullptr, *d_zo = nullptr;
};

}  // namespace krylov
}  // namespace cvrh

namespace {

constexpr int     kFsaiWaves = 2, kFsaiThreads = 64 * kFsaiWaves;
constexpr int     kFsaiLds = 64 * fsai::kLd;          // doubles a wavefront: (64 / G) groups of min(G, 32) rows
constexpr int     kFsaiMaxBlocks = 4096;
constexpr int32_t kNoRow = 0x7fffffff;

// ---- the device half

// what the lanes of this wavefront stored into LDS before is visible to all of them after
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// entry (r, c) of A as a double, +0 when row r has no column c
template <typename T>
__device__ __forceinline__ double entry_of(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ va, long long r, int c)
{
    const long long end = rp[r + 1];
    long long       lo = rp[r], hi = end;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (ci[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && ci[lo] == c ? (double)va[lo] : 0.0;
}

template <typename T>
__global__ __launch_bounds__(kFsaiThreads) void fsai_factor_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ va,
                                                                   const int64_t *__restrict__ src, const int64_t *__restrict__ wrp, long long n, int G,
                                                                   T *__restrict__ wa, T *__restrict__ wb, int32_t *bad)
{
    __shared__ double lds[kFsaiWaves][kFsaiLds];
    constexpr int   LD = fsai::kLd;
    const int       lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int       gpw = 64 / G, grp = lane / G, l = lane - grp * G;
    const int       cap = G < fsai::kMaxRow ? G : fsai::kMaxRow;          // the rows of S a group has room for: m <= cap by the choice of G
    double         *S = lds[wave] + grp * cap * LD;
    const long long wave0 = (long long)blockIdx.x * kFsaiWaves + wave, nwaves = (long long)gridDim.x * kFsaiWaves;

    for (long long base = wave0 * gpw; base < n; base += nwaves * gpw) {          // (the same trips in every lane of the wavefront)
        const long long row = base + grp;
        bool            on = row < n;
        int             m = 0;
        long long       s0 = 0, w0 = 0;
        if (on) {
            w0 = wrp[row];
            m = (int)(wrp[row + 1] - w0);
            s0 = src[row];
            if (m < 1 || m > cap) {          // (never, by the host's pattern: a row that would not fit is reported, not written)
                on = false;
                m = 0;
                if (l == 0) atomicMin(bad, (int)row);
            }
        }
        int kmax = m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int other = __shfl_xor(kmax, o);
            kmax = other > kmax ? other : kmax;
        }

        // the lower triangle of S: entry (p_a, p_b) of A
        if (on)
            for (int t = l; t < m * m; t += G) {
                const int a = t / m, b = t - a * m;
                if (b <= a) S[a * LD + b] = entry_of<T>(rp, ci, va, (long long)ci[s0 + a], ci[s0 + b]);
            }
        wave_sync();

        bool broken = false;          // (the same in every lane of the group)
        for (int k = 0; k < kmax; k++) {
            bool   go = on && !broken && k < m;
            double d = 1.0;
            if (go) {
                d = S[k * LD + k];
                if (!(d > 0 && d <= kDblMax)) {
                    broken = true;
                    go = false;
                }
            }
            if (go)
                for (int a = k + 1 + l; a < m; a += G) S[k * LD + a] = S[a * LD + k] / d;
            wave_sync();
            if (go)
                for (int a = k + 1; a < m; a++) {
                    const double lak = S[k * LD + a];
                    for (int b = k + 1 + l; b <= a; b += G) S[a * LD + b] = S[a * LD + b] - lak * S[b * LD + k];
                }
            wave_sync();
        }

        const bool go = on && !broken;
        double     dl = 1.0;
        if (go) dl = S[(m - 1) * LD + (m - 1)];
        wave_sync();          // (every lane has d_(m-1) before w takes the diagonal)
        if (go)
            for (int a = l; a < m; a += G) S[a * LD + a] = a == m - 1 ? 1.0 : 0.0;
        wave_sync();
        for (int b = kmax - 1; b >= 1; b--) {
            if (go && b < m) {
                const double wv = S[b * LD + b];
                for (int a = l; a < b; a += G) S[a * LD + a] = S[a * LD + a] - S[a * LD + b] * wv;
            }
            wave_sync();
        }
        if (go)
            for (int a = l; a < m; a += G) {
                const double w = S[a * LD + a];
                wa[w0 + a] = (T)w;
                wb[w0 + a] = (T)(w / dl);
            }
        if (on && broken && l == 0) atomicMin(bad, (int)row);
        wave_sync();          // (the next row's gather overwrites S)
    }
}

// ---- the host half

constexpr const char *kEntry = "cvr_precond_fsai";

template <typename T>
void launch_factor(const int64_t *rp, const int32_t *ci, const void *va, const int64_t *src, const int64_t *wrp, long long n, int G, void *wa, void *wb, int32_t *bad, hipStream_t st)
{
    const long long rows_per_block = (long long)kFsaiWaves * (64 / G);
    const long long blocks = std::min<long long>((n + rows_per_block - 1) / rows_per_block, kFsaiMaxBlocks);
    hipLaunchKernelGGL(fsai_factor_kernel<T>, dim3((unsigned)blocks), dim3(kFsaiThreads), 0, st, rp, ci, static_cast<const T *>(va), src, wrp, n, G, static_cast<T *>(wa), static_cast<T *>(wb), bad);
}

int build(cvr_precond *p, const cvr_csr_view *csr, hipStream_t st)
{
    HostCsr h;
    if (const int rc = stage_host(kEntry, csr, h, false, st)) return rc;
    const int64_t n = p->n;
    Fsai         *f = p->fsai;
    const size_t  vsz = p->is_f32 ? 4 : 8;
    std::vector<int64_t> src;
    fsai::Pattern        pat;
    try {
        f->wrp.assign((size_t)n + 1, 0);
        src.assign((size_t)n, 0);
        if (const int rc = fsai::pattern(n, h.rp, h.ci, "cvr_precond_fsai", f->wrp.data(), src.data(), &pat)) return rc;
        f->wci.resize((size_t)pat.nnz);
        for (int64_t i = 0; i < n; i++) std::copy(h.ci + src[(size_t)i], h.ci + src[(size_t)i] + (f->wrp[(size_t)i + 1] - f->wrp[(size_t)i]), f->wci.begin() + f->wrp[(size_t)i]);
    } catch (const std::bad_alloc &) {
        return fail(CVR_ERR_NOMEM, "cvr_precond_fsai: out of host memory for the pattern (%lld rows)", (long long)n);
    }
    f->nnz = pat.nnz;
    f->max_row = pat.max_row;
    f->truncated = pat.truncated;
    f->G = fsai::lanes_of(pat.max_row);
    if (n == 0) return CVR_OK;
    if (pat.nnz >= ((int64_t)1 << 32)) return fail(CVR_ERR_INVALID, "cvr_precond_fsai: W has %lld entries: the handle of its transpose needs fewer than 2^32", (long long)pat.nnz);

    const int64_t nnz_a = h.rp[n];
    if (const int rc = device_alloc(kEntry, &f->d_wa, vsz * (size_t)pat.nnz, "Wa")) return rc;
    if (const int rc = device_alloc(kEntry, &f->d_wb, vsz * (size_t)pat.nnz, "Wb")) return rc;
    {
        Scratch     s;
        void       *d_rp = nullptr, *d_ci = nullptr, *d_va = nullptr, *d_src = nullptr, *d_wrp = nullptr, *d_wci = nullptr, *d_bad = nullptr;
        const void *rp = csr->row_ptr, *ci = csr->col_idx, *va = csr->vals;
        if (!csr->arrays_on_device) {
            if (const int rc = scratch_alloc(kEntry, s, &d_rp, sizeof(int64_t) * (size_t)(n + 1), "row_ptr")) return rc;
            if (const int rc = scratch_alloc(kEntry, s, &d_ci, sizeof(int32_t) * (size_t)nnz_a, "col_idx")) return rc;
            if (const int rc = scratch_alloc(kEntry, s, &d_va, vsz * (size_t)nnz_a, "vals")) return rc;
            HIP_TRY(hipMemcpyAsync(d_rp, csr->row_ptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_ci, csr->col_idx, sizeof(int32_t) * (size_t)nnz_a, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_va, csr->vals, vsz * (size_t)nnz_a, hipMemcpyHostToDevice, st));
            rp = d_rp;
            ci = d_ci;
            va = d_va;
        }
        if (const int rc = scratch_alloc(kEntry, s, &d_src, sizeof(int64_t) * (size_t)n, "the rows' first entries")) return rc;
        if (const int rc = scratch_alloc(kEntry, s, &d_wrp, sizeof(int64_t) * (size_t)(n + 1), "W's row_ptr")) return rc;
        if (const int rc = scratch_alloc(kEntry, s, &d_wci, sizeof(int32_t) * (size_t)pat.nnz, "W's col_idx")) return rc;
        if (const int rc = scratch_alloc(kEntry, s, &d_bad, sizeof(int32_t), "the pivot word")) return rc;
        int32_t bad = kNoRow;
        HIP_TRY(hipMemcpyAsync(d_src, src.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_wrp, f->wrp.data(), sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_wci, f->wci.data(), sizeof(int32_t) * (size_t)pat.nnz, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_bad, &bad, sizeof(bad), hipMemcpyHostToDevice, st));
        if (p->is_f32)
            launch_factor<float>(static_cast<const int64_t *>(rp), static_cast<const int32_t *>(ci), va, static_cast<const int64_t *>(d_src), static_cast<const int64_t *>(d_wrp), (long long)n,
                                 (int)f->G, f->d_wa, f->d_wb, static_cast<int32_t *>(d_bad), st);
        else
            launch_factor<double>(static_cast<const int64_t *>(rp), static_cast<const int32_t *>(ci), va, static_cast<const int64_t *>(d_src), static_cast<const int64_t *>(d_wrp), (long long)n,
                                  (int)f->G, f->d_wa, f->d_wb, static_cast<int32_t *>(d_bad), st);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) {
            (void)hipStreamSynchronize(st);
            return fail(CVR_ERR_HIP, "cvr_precond_fsai: the set-up kernel: %s", hipGetErrorString(le));
        }
        HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));          // (the staged copies are released behind this; the handles below read W on their own streams)
        if (bad != kNoRow) return fail(CVR_ERR_STATE, "cvr_precond_fsai: the pivot of row %d is not finite or not > 0", bad);
        cvr_csr_view w{};          // the object's two handles: (W pattern, Wa), and (W pattern, Wb) transposed
        w.nrows = w.ncols = n;
        w.row_ptr = static_cast<const int64_t *>(d_wrp);
        w.col_idx = static_cast<const int32_t *>(d_wci);
        w.vals = f->d_wa;
        w.is_f32 = p->is_f32;
        w.arrays_on_device = 1;
        if (const int rc = make_handle(&f->ha, w, p->device, 0)) return rc;
        w.vals = f->d_wb;
        if (const int rc = make_handle(&f->hb, w, p->device, 1)) return rc;
        HIP_TRY(hipDeviceSynchronize());          // (the handles' copies of W are complete before the scratch goes)
    }
    // the three buffers, zeroed: xin[n] and t[n] are pad slots of an SpMV input
    const size_t bytes[3] = {x_ext_bytes(f->ha), vsz * (size_t)std::max<int64_t>({f->ha->info.yext_elems, f->hb->info.x_elems, n + 1}), y_ext_bytes(f->hb)};
    void       **bufs[3] = {&f->d_xin, &f->d_t, &f->d_zo};
    const char  *names[3] = {"xin", "t", "zo"};
    for (int i = 0; i < 3; i++)
        if (const int rc = zeroed(kEntry, bufs[i], bytes[i], names[i])) return rc;
    HIP_TRY(hipDeviceSynchronize());          // (whatever stream the first apply comes on finds them zeroed)
    return CVR_OK;
}

// xin = r | t = Wa xin | t[n] = 0 | zo = Wb^T t
template <typename T>
int enqueue_products(const cvr_precond *pc, const T *r, bool al, hipStream_t st)
{
    const Fsai     *f = pc->fsai;
    const long long n = pc->n;
    with_flags([&](auto AL) { launch(precond_copy_in_kernel<T, AL>, st, r, static_cast<T *>(f->d_xin), n); }, al);
    HIP_TRY(hipGetLastError());
    HIP_TRY(run_spmv(f->ha, f->d_xin, f->d_t, st));
    if (const int rc = zero_pad_slot(f->d_t, sizeof(T) * (size_t)n, sizeof(T), st)) return rc;          // (the product's dump slot is the next one's pad slot)
    HIP_TRY(run_spmv(f->hb, f->d_t, f->d_zo, st));
    return CVR_OK;
}

int fsai_apply_any(const cvr_precond *p, const void *r, void *z, hipStream_t st)
{
    const Fsai *f = p->fsai;
    if (!f || p->n == 0) return CVR_OK;
    const bool      ral = ((uintptr_t)r & 15u) == 0, zal = ((uintptr_t)z & 15u) == 0;
    const long long n = p->n;
    if (p->is_f32) {
        if (const int rc = enqueue_products<float>(p, static_cast<const float *>(r), ral, st)) return rc;
        with_flags([&](auto AL) { launch(precond_copy_out_kernel<float, AL>, st, static_cast<const float *>(f->d_zo), static_cast<float *>(z), n); }, zal);
    } else {
        if (const int rc = enqueue_products<double>(p, static_cast<const double *>(r), ral, st)) return rc;
        with_flags([&](auto AL) { launch(precond_copy_out_kernel<double, AL>, st, static_cast<const double *>(f->d_zo), static_cast<double *>(z), n); }, zal);
    }
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

template <typename T>
int fsai_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *spmvs)
{
    const Fsai *f = pc->fsai;
    if (!f || pc->n == 0) return CVR_OK;
    if (const int rc = enqueue_products<T>(pc, r, true, st)) return rc;
    if (spmvs) *spmvs += 2;
    with_flags([&](auto START) { launch(precond_rz_kernel<T, START, true>, st, r, static_cast<const T *>(f->d_zo), z, p, (long long)pc->n, part_rz, static_cast<const CgCell *>(cell)); }, start);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}
void fsai_release(cvr_precond *p)
{
    Fsai *f = p->fsai;
    if (!f) return;
    if (f->ha) (void)cvr_destroy(f->ha);
    if (f->hb) (void)cvr_destroy(f->hb);
    for (void *buf : {f->d_wa, f->d_wb, f->d_xin, f->d_t, f->d_zo})
        if (buf) (void)hipFree(buf);
    delete f;
    p->fsai = nullptr;
}

}  // namespace

namespace cvrh {
namespace krylov {

PrecondOps kFsaiOps = {kPrecondFsai, "FSAI", fsai_apply_any, fsai_release, fsai_cg_apply<float>, fsai_cg_apply<double>};

}  // namespace krylov
}  // namespace cvrh

extern "C" {

int cvr_precond_fsai(cvr_precond **out, const cvr_csr_view *csr, int32_t device, void *stream)
{
    if (!out || !csr) return fail(CVR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (csr->nrows != csr->ncols) return fail(CVR_ERR_INVALID, "FSAI needs a square matrix (%lld x %lld)", (long long)csr->nrows, (long long)csr->ncols);
    if (csr->nrows < 0) return fail(CVR_ERR_INVALID, "null or negative-size CSR view");
    if (csr->nrows >= (int64_t)0x7fffffff) return fail(CVR_ERR_INVALID, "cvr_precond_fsai: nrows (%lld) must stay below 2^31 - 1: the rows of W are the column indices of W^T", (long long)csr->nrows);
    if (device < 0 || device >= cvr_device_count()) return fail(CVR_ERR_NO_DEVICE, "device %d of %d", device, cvr_device_count());
    Range range("cvr_precond_fsai");
    HIP_TRY(hipSetDevice(device));
    cvr_precond *p = new (std::nothrow) cvr_precond;
    Fsai        *f = new (std::nothrow) Fsai;
    if (!p || !f) {
        delete p;
        delete f;
        return fail(CVR_ERR_NOMEM, "out of host memory");
    }
    p->kind = kPrecondFsai;
    p->ops = &kFsaiOps;
    p->device = device;
    p->n = csr->nrows;
    p->bs = 0;
    p->is_f32 = csr->is_f32 ? 1 : 0;
    p->fsai = f;
    if (const int rc = build(p, csr, (hipStream_t)stream)) return abandon(p, rc);
    *out = p;
    return CVR_OK;
}

int cvr_precond_fsai_info(const cvr_precond *p, cvr_fsai_info *info)
{
    if (!p || !info) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondFsai || !p->fsai) return fail(CVR_ERR_INVALID, "cvr_precond_fsai_info: the preconditioner is of kind %d, not an FSAI object (kind %d)", p->kind, kPrecondFsai);
    const Fsai *f = p->fsai;
    memset(info, 0, sizeof(*info));
    info->n = p->n;
    info->nnz = f->nnz;
    info->max_row = f->max_row;
    info->lanes_per_row = f->G;
    info->truncated_rows = f->truncated;
    info->is_f32 = p->is_f32;
    return CVR_OK;
}

int cvr_precond_fsai_export(const cvr_precond *p, int64_t *row_ptr, int32_t *col_idx, void *wa, void *wb)
{
    if (!p || !row_ptr) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondFsai || !p->fsai) return fail(CVR_ERR_INVALID, "cvr_precond_fsai_export: the preconditioner is of kind %d, not an FSAI object (kind %d)", p->kind, kPrecondFsai);
    const Fsai *f = p->fsai;
    if (f->nnz > 0 && (!col_idx || !wa || !wb)) return fail(CVR_ERR_INVALID, "null argument");
    std::copy(f->wrp.begin(), f->wrp.end(), row_ptr);
    if (f->nnz == 0) return CVR_OK;
    std::copy(f->wci.begin(), f->wci.end(), col_idx);
    HIP_TRY(hipSetDevice(p->device));
    const size_t bytes = (p->is_f32 ? 4 : 8) * (size_t)f->nnz;
    HIP_TRY(hipMemcpy(wa, f->d_wa, bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(wb, f->d_wb, bytes, hipMemcpyDeviceToHost));
    return CVR_OK;
}

}  // extern "C"
