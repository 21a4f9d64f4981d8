// cvr_mcsgs.hip -- the multicolour symmetric Gauss-Seidel preconditioner, the sixth kind of cvr_precond (include/cvr_amd.h: cvr_precond_mcsgs,
// cvr_precond_mcsgs_info, cvr_precond_mcsgs_export).  M = (D + L) D^-1 (D + U) with the rows ordered by a colouring of A's graph (cvr_color.hip):
// L holds the entries a_ij with color[j] < color[i], U those with color[j] > color[i], and no off-diagonal entry joins two rows of one colour, so
// the rows of a colour are independent and a triangular sweep is one launch per colour -- 2 ncolors launches per apply, about ten on a Laplacian,
// where ILU(0)'s levels in the natural order are thousands.  No factorisation: the values are A's own.
//   Set-up, on the device: the colouring; then per row in perm order the sizes of its two parts, the diagonal as a double and the lowest row
//     whose diagonal is zero or not finite (atomicMin); rocprim's scans of the sizes; then the two parts written as one CSR-like store in perm
//     order (all L parts, then all U parts), each part in A's column order with the original column numbers.  The host waits on the words of
//     the colouring, the ncolors + 1 colour offsets and the bad-row word, never on an array of n.
//   Apply: G lanes per row by ILU(0)'s rule and with ILU(0)'s sum (lane l adds double(a_ij) * double(v_j) over the entries l, l + G, .. of the
//     row's part from +0; the xor butterfly G/2 .. 1).  Forward over the colours y_i = T((double(r_i) - s) / double(a_ii)), backward
//     z_i = T(double(y_i) - s / double(a_ii)).  y is a buffer of the object.
//   Where the time goes: a launch reads its rows' slots (16 bytes each), entries and diagonals as contiguous streams, because they are stored in
//     perm order; what is not contiguous is the gather of v_j and the one value stored per row at its original number.
// (The reference has no solver and no preconditioner: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include <rocprim/device/device_scan.hpp>

#include "cvr_krylov.h"
#include "cvr_cg_kernels.h"
#include "cvr_color.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace cvrh {
namespace krylov {

// a row in perm order: the entries of one of its parts are beg .. beg + cnt - 1 of the object's store
struct McSlot {
    long long beg;
    int32_t   cnt, row;
};
static_assert(sizeof(McSlot) == 16, "one 16-byte load per row");

struct McSgs {
    int64_t              nnz = 0;
    int32_t              G = 1, ncolors = 0, rounds = 0;
    std::vector<int32_t> color_ptr{0};          // ncolors + 1: where each colour begins in perm
    int32_t             *d_color = nullptr, *d_perm = nullptr;
    McSlot              *d_lo = nullptr, *d_up = nullptr;          // n each, in perm order
    int32_t             *d_ci = nullptr;                           // nnz - n: every L part, then every U part
    void                *d_va = nullptr;                           // ... their values of T
    double              *d_diag = nullptr;                         // n, in perm order
    void                *d_y = nullptr;                            // n values of T
};

}  // namespace krylov
}  // namespace cvrh

namespace {

constexpr int32_t     kNoRow = 0x7fffffff;
constexpr const char *kEntry = "cvr_precond_mcsgs";

#define CVR_MCSGS_ROWS(k, n) for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < (n); k += (long long)gridDim.x * kThreads)

// ---- the device half

// of the row at place k: the sizes of its parts, its diagonal; bad = the lowest row whose diagonal is zero or not finite
template <typename T>
__global__ __launch_bounds__(kThreads) void mcsgs_count_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ va, long long n,
                                                               const int32_t *__restrict__ color, const int32_t *__restrict__ perm, long long *__restrict__ nlo,
                                                               long long *__restrict__ nup, double *__restrict__ diag, int32_t *__restrict__ bad)
{
    CVR_MCSGS_ROWS(k, n) {
        const int i = perm[k], c = color[i];
        long long lo = 0, up = 0;
        double    d = 0;
        for (long long q = rp[i]; q < rp[i + 1]; q++) {
            const int j = ci[q];
            if (j == i) d = (double)va[q];
            else if (color[j] < c) lo++;
            else up++;
        }
        nlo[k] = lo;
        nup[k] = up;
        diag[k] = d;
        if (!usable(d)) atomicMin(bad, i);
    }
}

// the parts of the row at place k, behind the scans of their sizes (plo and pup: n + 1 each; the U parts begin at plo[n])
template <typename T>
__global__ __launch_bounds__(kThreads) void mcsgs_fill_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ va, long long n,
                                                              const int32_t *__restrict__ color, const int32_t *__restrict__ perm, const long long *__restrict__ plo,
                                                              const long long *__restrict__ pup, McSlot *__restrict__ lo, McSlot *__restrict__ up, int32_t *__restrict__ pci,
                                                              T *__restrict__ pva)
{
    const long long u0 = plo[n];
    CVR_MCSGS_ROWS(k, n) {
        const int i = perm[k], c = color[i];
        long long l = plo[k], u = u0 + pup[k];
        lo[k] = {l, (int32_t)(plo[k + 1] - plo[k]), i};
        up[k] = {u, (int32_t)(pup[k + 1] - pup[k]), i};
        for (long long q = rp[i]; q < rp[i + 1]; q++) {
            const int j = ci[q];
            if (j == i) continue;
            const long long at = color[j] < c ? l++ : u++;
            pci[at] = j;
            pva[at] = va[q];
        }
    }
}

// One colour of a sweep: the rows at the places slot0 .. slot0 + nslots - 1, G lanes each.  v: the vector being solved for (y forward, z
// backward), rhs: r or y.  Nothing is written once *stop is set (stop may be null).
template <typename T, bool BACK>
__global__ __launch_bounds__(kThreads) void mcsgs_sweep_kernel(const McSlot *__restrict__ slots, int slot0, int nslots, int G, const int32_t *__restrict__ ci, const T *__restrict__ va,
                                                               const double *__restrict__ diag, const T *rhs, T *v, const int32_t *__restrict__ stop)
{
    if (stop && *stop) return;
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long k = t / G;
    const int       l = (int)(t - k * G);
    const bool      active = k < nslots;
    McSlot          s{0, 0, 0};
    if (active) s = slots[slot0 + k];
    double acc = 0;
    for (int e = l; e < s.cnt; e += G) {          // (an idle lane's cnt is 0)
        const long long q = s.beg + e;
        acc += (double)va[q] * (double)v[ci[q]];
    }
    for (int o = G >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o);          // every lane of the wavefront is here
    if (active && l == 0) {
        const double d = diag[slot0 + k];
        if constexpr (BACK) v[s.row] = (T)((double)rhs[s.row] - acc / d);
        else v[s.row] = (T)(((double)rhs[s.row] - acc) / d);
    }
}

// ---- the host half

// G: the power of two from the mean number of entries of a row in one part, ceil((nnz - n) / (2 n)), up; 1 .. 64 (ILU(0)'s rule)
int32_t lanes_of(int64_t n, int64_t nnz)
{
    const int64_t mean = n > 0 ? (nnz - n + 2 * n - 1) / (2 * n) : 0;
    int32_t       G = 1;
    while (G < mean && G < 64) G <<= 1;
    return G;
}

template <typename... P, typename... A>
void launch_rows(void (*kernel)(P...), long long n, hipStream_t st, A... args)
{
    const long long blocks = std::min<long long>((n + kThreads - 1) / kThreads, kBlocks);
    hipLaunchKernelGGL(kernel, dim3((unsigned)std::max<long long>(blocks, 1)), dim3(kThreads), 0, st, args...);
}

template <typename T>
int build_parts(cvr_precond *p, const cvr_csr_view &dv, hipStream_t st)
{
    McSgs          *m = p->mcsgs;
    const long long n = p->n;
    const T        *va = static_cast<const T *>(dv.vals);
    Scratch         s;
    void           *d_nlo = nullptr, *d_nup = nullptr, *d_plo = nullptr, *d_pup = nullptr, *d_bad = nullptr, *d_tmp = nullptr;
    const size_t    words = sizeof(long long) * (size_t)(n + 1);
    if (const int rc = scratch_alloc(kEntry, s, &d_nlo, words, "the L parts' sizes")) return rc;
    if (const int rc = scratch_alloc(kEntry, s, &d_nup, words, "the U parts' sizes")) return rc;
    if (const int rc = scratch_alloc(kEntry, s, &d_plo, words, "the L parts' places")) return rc;
    if (const int rc = scratch_alloc(kEntry, s, &d_pup, words, "the U parts' places")) return rc;
    if (const int rc = scratch_alloc(kEntry, s, &d_bad, sizeof(int32_t), "the bad-row word")) return rc;
    long long *nlo = static_cast<long long *>(d_nlo), *nup = static_cast<long long *>(d_nup), *plo = static_cast<long long *>(d_plo), *pup = static_cast<long long *>(d_pup);
    int32_t    bad = kNoRow;
    HIP_TRY(hipMemcpyAsync(d_bad, &bad, sizeof(bad), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(nlo + n, 0, sizeof(long long), st));          // (the scans' last element: the totals)
    HIP_TRY(hipMemsetAsync(nup + n, 0, sizeof(long long), st));
    launch_rows(mcsgs_count_kernel<T>, n, st, dv.row_ptr, dv.col_idx, va, n, (const int32_t *)m->d_color, (const int32_t *)m->d_perm, nlo, nup, m->d_diag, static_cast<int32_t *>(d_bad));
    HIP_TRY(hipGetLastError());
    size_t bytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, bytes, nlo, plo, 0ll, (size_t)(n + 1), rocprim::plus<long long>(), st));
    if (const int rc = scratch_alloc(kEntry, s, &d_tmp, bytes, "the scan's workspace")) return rc;
    HIP_TRY(rocprim::exclusive_scan(d_tmp, bytes, nlo, plo, 0ll, (size_t)(n + 1), rocprim::plus<long long>(), st));
    HIP_TRY(rocprim::exclusive_scan(d_tmp, bytes, nup, pup, 0ll, (size_t)(n + 1), rocprim::plus<long long>(), st));
    launch_rows(mcsgs_fill_kernel<T>, n, st, dv.row_ptr, dv.col_idx, va, n, (const int32_t *)m->d_color, (const int32_t *)m->d_perm, (const long long *)plo, (const long long *)pup, m->d_lo,
                m->d_up, m->d_ci, static_cast<T *>(m->d_va));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));          // (the scratch goes)
    if (bad != kNoRow) return fail(CVR_ERR_STATE, "cvr_precond_mcsgs: the diagonal entry of row %d is zero or not finite", bad);
    return CVR_OK;
}

int build(cvr_precond *p, const cvr_csr_view *csr, hipStream_t st)
{
    McSgs               *m = p->mcsgs;
    const int64_t        n = p->n;
    Scratch              s;
    cvr_csr_view         dv;
    std::vector<int64_t> rp_own;
    const int64_t       *rp = nullptr;
    if (const int rc = stage_device(kEntry, csr, true, s, &dv, rp_own, &rp, st)) return rc;
    if (n == 0) return CVR_OK;
    const int64_t nnz = rp[n] - rp[0];
    const size_t  vsz = p->is_f32 ? 4 : 8;
    m->nnz = nnz;
    m->G = lanes_of(n, nnz);
    if (const char *e = cvr::debug_env("mcsgs_lanes")) {          // (an experiment: tools/mcsgs_probe.py)
        const long long g = atoll(e);
        if (g >= 1 && g <= 64 && (g & (g - 1)) == 0) m->G = (int32_t)g;
    }
    if (const int rc = device_alloc(kEntry, reinterpret_cast<void **>(&m->d_color), sizeof(int32_t) * (size_t)n, "the colours")) return rc;
    if (const int rc = device_alloc(kEntry, reinterpret_cast<void **>(&m->d_perm), sizeof(int32_t) * (size_t)n, "perm")) return rc;
    if (const int rc = color_device(kEntry, dv, rp, m->d_color, m->d_perm, m->color_ptr, &m->ncolors, &m->rounds, st)) return rc;
    // (a pattern that passed the rules holds n diagonal entries: nnz - n is not negative)
    if (const int rc = device_alloc(kEntry, reinterpret_cast<void **>(&m->d_lo), sizeof(McSlot) * (size_t)n, "the forward sweep's rows")) return rc;
    if (const int rc = device_alloc(kEntry, reinterpret_cast<void **>(&m->d_up), sizeof(McSlot) * (size_t)n, "the backward sweep's rows")) return rc;
    if (const int rc = device_alloc(kEntry, reinterpret_cast<void **>(&m->d_ci), sizeof(int32_t) * (size_t)(nnz - n), "the parts' columns")) return rc;
    if (const int rc = device_alloc(kEntry, &m->d_va, vsz * (size_t)(nnz - n), "the parts' values")) return rc;
    if (const int rc = device_alloc(kEntry, reinterpret_cast<void **>(&m->d_diag), sizeof(double) * (size_t)n, "the diagonal")) return rc;
    if (const int rc = device_alloc(kEntry, &m->d_y, vsz * (size_t)n, "y")) return rc;
    HIP_TRY(hipMemsetAsync(m->d_y, 0, vsz * (size_t)n, st));
    return p->is_f32 ? build_parts<float>(p, dv, st) : build_parts<double>(p, dv, st);
}

// the 2 ncolors launches of one apply
template <typename T>
int mcsgs_sweeps(const cvr_precond *pc, const T *r, T *z, const int32_t *stop, hipStream_t st)
{
    const McSgs *m = pc->mcsgs;
    if (!m || pc->n == 0) return CVR_OK;
    T       *y = static_cast<T *>(m->d_y);
    const T *va = static_cast<const T *>(m->d_va);
    auto     blocks = [&](int32_t rows) { return dim3((unsigned)(((long long)rows * m->G + kThreads - 1) / kThreads)); };
    for (int32_t c = 0; c < m->ncolors; c++) {
        const int32_t a = m->color_ptr[(size_t)c], rows = m->color_ptr[(size_t)c + 1] - a;
        hipLaunchKernelGGL((mcsgs_sweep_kernel<T, false>), blocks(rows), dim3(kThreads), 0, st, (const McSlot *)m->d_lo, (int)a, (int)rows, (int)m->G, (const int32_t *)m->d_ci, va,
                           (const double *)m->d_diag, r, y, stop);
    }
    for (int32_t c = m->ncolors - 1; c >= 0; c--) {
        const int32_t a = m->color_ptr[(size_t)c], rows = m->color_ptr[(size_t)c + 1] - a;
        hipLaunchKernelGGL((mcsgs_sweep_kernel<T, true>), blocks(rows), dim3(kThreads), 0, st, (const McSlot *)m->d_up, (int)a, (int)rows, (int)m->G, (const int32_t *)m->d_ci, va,
                           (const double *)m->d_diag, (const T *)y, z, stop);
    }
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

int mcsgs_apply(const cvr_precond *p, const void *r, void *z, hipStream_t st)          // by the object's type
{
    if (p->is_f32) return mcsgs_sweeps<float>(p, static_cast<const float *>(r), static_cast<float *>(z), nullptr, st);
    return mcsgs_sweeps<double>(p, static_cast<const double *>(r), static_cast<double *>(z), nullptr, st);
}

// the sweeps into z, then one kernel on the solvers' grid with the partial sums and, at the start, p = z: exactly as ILU(0)'s
template <typename T>
int mcsgs_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *)
{
    const CgCell *c = static_cast<const CgCell *>(cell);
    if (const int rc = mcsgs_sweeps<T>(pc, r, z, start ? nullptr : &c->stop, st)) return rc;
    with_flags([&](auto START) { launch(precond_rz_kernel<T, START, false>, st, r, (const T *)z, (T *)nullptr, p, (long long)pc->n, part_rz, c); }, start);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

void mcsgs_release(cvr_precond *p)
{
    McSgs *m = p->mcsgs;
    if (!m) return;
    for (void *buf : {(void *)m->d_color, (void *)m->d_perm, (void *)m->d_lo, (void *)m->d_up, (void *)m->d_ci, m->d_va, (void *)m->d_diag, m->d_y})
        if (buf) (void)hipFree(buf);
    delete m;
    p->mcsgs = nullptr;
}

int not_this_kind(const cvr_precond *p, const char *entry)
{
    return fail(CVR_ERR_INVALID, "%s: the preconditioner is of kind %d, not a multicolour SGS object (kind %d)", entry, p->kind, kPrecondMcSgs);
}

}  // namespace

namespace cvrh {
namespace krylov {
PrecondOps kMcSgsOps = {kPrecondMcSgs, "multicolour SGS", mcsgs_apply, mcsgs_release, mcsgs_cg_apply<float>, mcsgs_cg_apply<double>};
}  // namespace krylov
}  // namespace cvrh

extern "C" {

int cvr_precond_mcsgs(cvr_precond **out, const cvr_csr_view *csr, int32_t device, void *stream)
{
    if (!out || !csr) return fail(CVR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (csr->nrows != csr->ncols) return fail(CVR_ERR_INVALID, "multicolour SGS needs a square matrix (%lld x %lld)", (long long)csr->nrows, (long long)csr->ncols);
    if (csr->nrows < 0) return fail(CVR_ERR_INVALID, "null or negative-size CSR view");
    if (csr->nrows > (int64_t)0x7fffffff) return fail(CVR_ERR_INVALID, "%s: nrows (%lld) must stay below 2^31", kEntry, (long long)csr->nrows);
    if (device < 0 || device >= cvr_device_count()) return fail(CVR_ERR_NO_DEVICE, "device %d of %d", device, cvr_device_count());
    cvr::debug_refresh();
    Range range(kEntry);
    HIP_TRY(hipSetDevice(device));
    cvr_precond *p = new (std::nothrow) cvr_precond;
    McSgs       *m = new (std::nothrow) McSgs;
    if (!p || !m) {
        delete p;
        delete m;
        return fail(CVR_ERR_NOMEM, "out of host memory");
    }
    p->kind = kPrecondMcSgs;
    p->ops = &kMcSgsOps;
    p->device = device;
    p->n = csr->nrows;
    p->bs = 0;
    p->is_f32 = csr->is_f32 ? 1 : 0;
    p->mcsgs = m;
    if (const int rc = build(p, csr, (hipStream_t)stream)) return abandon(p, rc);
    *out = p;
    return CVR_OK;
}

int cvr_precond_mcsgs_info(const cvr_precond *p, cvr_mcsgs_info *info)
{
    if (!p || !info) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondMcSgs || !p->mcsgs) return not_this_kind(p, "cvr_precond_mcsgs_info");
    const McSgs *m = p->mcsgs;
    memset(info, 0, sizeof(*info));
    info->n = p->n;
    info->nnz = m->nnz;
    info->ncolors = m->ncolors;
    info->rounds = m->rounds;
    info->launches_per_apply = 2 * m->ncolors;
    info->lanes_per_row = m->G;
    for (int32_t c = 0; c < m->ncolors; c++) {
        const int32_t rows = m->color_ptr[(size_t)c + 1] - m->color_ptr[(size_t)c];
        info->max_color_rows = std::max(info->max_color_rows, rows);
        info->min_color_rows = c == 0 ? rows : std::min(info->min_color_rows, rows);
    }
    info->is_f32 = p->is_f32;
    return CVR_OK;
}

int cvr_precond_mcsgs_export(const cvr_precond *p, int32_t *color_host, int32_t *perm_host, int32_t *color_ptr_host)
{
    if (!p || !color_ptr_host) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondMcSgs || !p->mcsgs) return not_this_kind(p, "cvr_precond_mcsgs_export");
    if (p->n > 0 && (!color_host || !perm_host)) return fail(CVR_ERR_INVALID, "null argument");
    const McSgs *m = p->mcsgs;
    std::copy(m->color_ptr.begin(), m->color_ptr.end(), color_ptr_host);
    if (p->n == 0) return CVR_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpy(color_host, m->d_color, sizeof(int32_t) * (size_t)p->n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(perm_host, m->d_perm, sizeof(int32_t) * (size_t)p->n, hipMemcpyDeviceToHost));
    return CVR_OK;
}

}  // extern "C"
