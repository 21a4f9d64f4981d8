// cvr_precond.hip -- the block-Jacobi preconditioner (include/cvr_amd.h: cvr_precond_*), the entry points all kinds of object share (apply and
// destroy: they call the kind's table, cvr_precond.h's PrecondOps) and the helpers every kind's constructor builds with.  The object is built once
// from a CSR view -- one kernel gathers the diagonal blocks into
// LDS, inverts them there in fp64 and stores the inverses W in the matrix's type -- and applied by a kernel on the solvers' grid: thread g forms z for
// the elements CVR_KRYLOV_PACKETS gives it (cvr_precond.h: the struct and the apply of one packet, shared with cvr_bicgstab.hip and cvr_gmres.hip).
//   precond_build_kernel   one wavefront per workgroup; L = 8, 16 or 32 lanes per block (the power of two from bs up), 64 / L blocks per wavefront
//   precond_apply_kernel   z = W r
//   pcg_apply_kernel       the same inside the solver, with the partial sums of r . z (set 1 of cg_direction_kernel<T, true>) and, at the start, p = z
// W lies block after block, each block TRANSPOSED (element (i, j) at j * bs + i): for a fixed j the threads that own neighbouring rows load neighbouring
// values.  The solver is cvr_cg.hip's cg_solve, which enqueues pcg_apply_kernel through kBlockJacobiOps' cg_apply (cvr_precond.h); this file launches no
// cg_* kernel and holds no solve loop (cvr_cg_kernels.h is included for the state cell the apply reads).
// (The reference has no solver and no preconditioner: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_cg_kernels.h"
#include "cvr_precond.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

constexpr int kBuildLanes = 64;                                              // one wavefront per workgroup
constexpr int kBuildLds = CVR_PRECOND_MAX_BLOCK * (CVR_PRECOND_MAX_BLOCK + 1) * 2;   // doubles: (64 / L) * bs * (bs + 1) is largest at bs = 32 (two blocks)
constexpr int kNoOwner = 0x7fffffff;

// bs rounded up to a power of two, and at least 8: a row is scanned by 8 lanes or more, eight blocks of bs <= 8 share a wavefront
inline int lanes_per_block(int bs)
{
    int L = 8;
    while (L < bs) L <<= 1;
    return L;
}

// Gathers and inverts the blocks of one wavefront.  Lane = blk * L + sub: the L lanes of a block scan its rows together (row after row, L entries a
// trip), then lane sub < bs owns row sub of the block through the elimination.  Every loop bound is the same in all 64 lanes (the longest row of the
// wavefront's blocks sets the trips of a scan), so the barriers between the LDS phases are met by all of them.
// Entry (i, j) is the fp64 sum of the row's entries with that column in CSR order: of the lanes that find the same (i, j) in one trip the lowest goes
// first (an LDS claim word per column, atomicMin), the others go round again.
template <typename T>
__global__ __launch_bounds__(kBuildLanes) void precond_build_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ va,
                                                                    long long n, int bs, int L, long long nblocks, T *__restrict__ wt,
                                                                    unsigned long long *__restrict__ nidentity)
{
    __shared__ double A[kBuildLds];
    __shared__ int    owner[kBuildLanes], piv[kBuildLanes];
    const int       lane = threadIdx.x, blk = lane / L, sub = lane - blk * L, bpw = kBuildLanes / L;
    const long long kb = (long long)blockIdx.x * bpw + blk;          // this lane's block
    const bool      live = kb < nblocks;
    const long long row0 = kb * bs;
    const int       ld = bs + 1;                                     // the pitch of a row: lanes that own neighbouring rows fall on different LDS banks
    double         *a = A + blk * bs * ld;                           // row-major, bs x bs
    int            *own = owner + blk * bs, *pv = piv + blk * bs;

    // the block starts as zero, with the identity in the rows a short last block does not have
    for (int t = sub; t < bs * bs; t += L) {
        const int i = t / bs, j = t - i * bs;
        a[i * ld + j] = (i == j && live && row0 + i >= n) ? 1.0 : 0.0;
    }
    if (sub < bs) own[sub] = kNoOwner;
    __syncthreads();

    for (int i = 0; i < bs; i++) {
        const long long row = row0 + i;
        const bool      has = live && row < n;
        const long long beg = has ? rp[row] : 0, end = has ? rp[row + 1] : 0;
        long long       trips = (end - beg + L - 1) / L;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long other = __shfl_xor(trips, o);
            trips = other > trips ? other : trips;
        }
        for (long long t = 0; t < trips; t++) {
            const long long idx = beg + t * L + sub;
            bool            pending = false;
            int             j = 0;
            double          v = 0;
            if (idx < end) {
                const long long c = (long long)ci[idx] - row0;
                if (c >= 0 && c < bs) { pending = true; j = (int)c; v = (double)va[idx]; }
            }
            while (__any(pending)) {
                if (pending) atomicMin(&own[j], sub);
                __syncthreads();
                const bool mine = pending && own[j] == sub;
                if (mine) a[i * ld + j] += v;
                __syncthreads();
                if (mine) { own[j] = kNoOwner; pending = false; }
                __syncthreads();
            }
        }
    }
    __syncthreads();

    // Gauss-Jordan in place with partial pivoting (the largest |.| of the column from the diagonal down, the first of equals); rows are swapped, the
    // swaps are undone on the columns of the inverse at the end.  A pivot that is zero or not finite, or a candidate that is a NaN: the block is bad.
    const bool rowlane = live && sub < bs;
    bool       bad = false;
    for (int c = 0; c < bs; c++) {
        double cand = -1.0;
        int    at = sub;
        bool   nan = false;
        if (rowlane && sub >= c) {
            const double x = a[sub * ld + c];
            nan = x != x;
            cand = nan ? -1.0 : fabs(x);
        }
        for (int o = L >> 1; o > 0; o >>= 1) {
            const double oc = __shfl_xor(cand, o);
            const int    oa = __shfl_xor(at, o);
            const bool   on = __shfl_xor((int)nan, o) != 0;
            if (oc > cand || (oc == cand && oa < at)) { cand = oc; at = oa; }
            nan = nan || on;
        }
        if (nan || !(cand > 0) || !(cand <= kDblMax)) bad = true;          // (the same in every lane of the block)
        if (rowlane && sub == 0) pv[c] = bad ? c : at;
        __syncthreads();
        if (rowlane && !bad && at != c) {          // lane sub swaps column sub of rows c and at
            const double x = a[c * ld + sub], y = a[at * ld + sub];
            a[c * ld + sub] = y;
            a[at * ld + sub] = x;
        }
        __syncthreads();
        const double p = rowlane && !bad ? a[c * ld + c] : 1.0;
        __syncthreads();
        if (rowlane && !bad) a[c * ld + sub] = (sub == c ? 1.0 : a[c * ld + sub]) / p;          // the pivot row, column by column
        __syncthreads();
        if (rowlane && !bad && sub != c) {          // row sub -= f * (pivot row), with the column of the pivot taken over by the inverse
            const double f = a[sub * ld + c];
            a[sub * ld + c] = 0.0;
            for (int j = 0; j < bs; j++) a[sub * ld + j] -= f * a[c * ld + j];
        }
        __syncthreads();
    }
    if (rowlane && !bad) {
        for (int c = bs - 1; c >= 0; c--) {
            const int q = pv[c];
            if (q != c) {
                const double x = a[sub * ld + c];
                a[sub * ld + c] = a[sub * ld + q];
                a[sub * ld + q] = x;
            }
        }
    }
    // an inverse with a value that is not finite (an overflow on the way) is bad as well
    int notfinite = 0;
    if (rowlane && !bad)
        for (int j = 0; j < bs; j++) notfinite |= !(fabs(a[sub * ld + j]) <= kDblMax);
    for (int o = L >> 1; o > 0; o >>= 1) notfinite |= __shfl_xor(notfinite, o);
    bad = bad || notfinite != 0;
    if (rowlane) {
        T *w = wt + kb * bs * bs;
        for (int j = 0; j < bs; j++) w[j * bs + sub] = bad ? (T)(j == sub ? 1 : 0) : (T)a[sub * ld + j];
        if (bad && sub == 0) atomicAdd(nidentity, 1ull);
    }
}

// z = W r.  AL: z, the caller's array, is 16-byte aligned (r is read value by value)
template <typename T, bool AL>
__global__ __launch_bounds__(kThreads) void precond_apply_kernel(const T *__restrict__ wt, int bs, const T *__restrict__ r, T *__restrict__ z, long long n)
{
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T zv[kPack<T>];
        apply_pack<T>(wt, bs, r, n, e, (int)cnt, zv);
        store_pack<T, AL>(z, e, (int)cnt, zv);
    }
}

// The solver's form: z = W r and the partial sums of r . z, the terms double(r_i) * double(z_i) added in the thread that owns element i, in element
// order -- what cg_update_kernel<T, true, AL> puts into set 1.  START: before the state cell exists; p = z as well.  Otherwise nothing is written
// once the cell holds a stop (no workgroup of this kernel sets it).
template <typename T, bool START>
__global__ __launch_bounds__(kThreads) void pcg_apply_kernel(const T *__restrict__ wt, int bs, const T *__restrict__ r, T *__restrict__ z, T *__restrict__ p,
                                                             long long n, double *__restrict__ out, const CgCell *__restrict__ cell)
{
    __shared__ double sh[1][kWaves];
    if constexpr (!START)
        if (cell->stop) return;
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T rv[kPack<T>], zv[kPack<T>];
        load_pack<T, true>(r, e, (int)cnt, rv);
        apply_pack<T>(wt, bs, r, n, e, (int)cnt, zv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) if (j < cnt) acc[0] += (double)rv[j] * (double)zv[j];
        store_pack<T, true>(z, e, (int)cnt, zv);
        if constexpr (START) store_pack<T, true>(p, e, (int)cnt, zv);
    }
    store_partials<1>(acc, out, sh);
}

// ---- the object

// the CSR arrays in device memory: the caller's own, or copies that live as long as this object
struct DeviceCsr {
    const int64_t *rp = nullptr;
    const int32_t *ci = nullptr;
    const void    *va = nullptr;
    void          *owned[3] = {nullptr, nullptr, nullptr};
    DeviceCsr() = default;
    DeviceCsr(const DeviceCsr &) = delete;
    DeviceCsr &operator=(const DeviceCsr &) = delete;
    ~DeviceCsr()
    {
        for (void *p : owned)
            if (p) (void)hipFree(p);
    }
};

constexpr const char *kEntry = "cvr_precond_block_jacobi";

// checks the view as cvr_create does and leaves its arrays on the device
int stage_csr(const cvr_csr_view *c, DeviceCsr &d, hipStream_t st)
{
    const int64_t n = c->nrows;
    const size_t  vsz = c->is_f32 ? 4 : 8;
    if (!c->arrays_on_device) {
        if (const int rc = check_csr(c, true)) return rc;
        if (n == 0) return CVR_OK;
        const int64_t nnz = c->row_ptr[n];
        if (const int rc = device_alloc(kEntry, &d.owned[0], sizeof(int64_t) * (size_t)(n + 1), "row_ptr")) return rc;
        if (const int rc = device_alloc(kEntry, &d.owned[1], sizeof(int32_t) * (size_t)nnz, "col_idx")) return rc;
        if (const int rc = device_alloc(kEntry, &d.owned[2], vsz * (size_t)nnz, "vals")) return rc;
        HIP_TRY(hipMemcpyAsync(d.owned[0], c->row_ptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, st));
        if (nnz > 0) {
            HIP_TRY(hipMemcpyAsync(d.owned[1], c->col_idx, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d.owned[2], c->vals, vsz * (size_t)nnz, hipMemcpyHostToDevice, st));
        }
        d.rp = static_cast<const int64_t *>(d.owned[0]);
        d.ci = static_cast<const int32_t *>(d.owned[1]);
        d.va = d.owned[2];
        return CVR_OK;
    }
    std::vector<int64_t> rp_host;          // (8 bytes per row, for the checks only)
    if (const int rc = check_device_view(kEntry, c, rp_host, st)) return rc;
    d.rp = c->row_ptr;
    d.ci = c->col_idx;
    d.va = c->vals;
    return CVR_OK;
}

template <typename T>
hipError_t launch_build(const DeviceCsr &d, const cvr_precond *p, unsigned long long *count, hipStream_t st)
{
    const int       L = lanes_per_block(p->bs), bpw = kBuildLanes / L;
    const long long groups = (p->nblocks + bpw - 1) / bpw;
    hipLaunchKernelGGL(precond_build_kernel<T>, dim3((unsigned)groups), dim3(kBuildLanes), 0, st, d.rp, d.ci, static_cast<const T *>(d.va), (long long)p->n,
                       (int)p->bs, L, (long long)p->nblocks, static_cast<T *>(p->d_w), count);
    return hipGetLastError();
}

int build(cvr_precond *p, const cvr_csr_view *csr, hipStream_t st)
{
    DeviceCsr d;
    if (const int rc = stage_csr(csr, d, st)) return rc;
    if (p->nblocks == 0) return CVR_OK;
    const size_t vsz = p->is_f32 ? 4 : 8;
    if (const int rc = device_alloc(kEntry, &p->d_w, vsz * (size_t)p->nblocks * (size_t)p->bs * (size_t)p->bs, "the inverse blocks")) return rc;
    void *count = nullptr;
    if (const int rc = device_alloc(kEntry, &count, sizeof(unsigned long long), "the counter")) return rc;
    unsigned long long bad = 0;
    hipError_t         e = hipMemsetAsync(count, 0, sizeof(bad), st);
    if (e == hipSuccess) e = p->is_f32 ? launch_build<float>(d, p, static_cast<unsigned long long *>(count), st) : launch_build<double>(d, p, static_cast<unsigned long long *>(count), st);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, count, sizeof(bad), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);          // (the staged copies of the CSR are released behind this)
    (void)hipFree(count);
    if (e != hipSuccess) return fail(CVR_ERR_HIP, "cvr_precond_block_jacobi: %s", hipGetErrorString(e));
    p->identity_blocks = (int64_t)bad;
    return CVR_OK;
}

// ---- kBlockJacobiOps

int block_jacobi_apply(const cvr_precond *p, const void *r, void *z, hipStream_t st)
{
    const bool      al = ((uintptr_t)z & 15u) == 0;
    const long long n = p->n;
    if (p->is_f32)
        with_flags([&](auto AL) { launch(precond_apply_kernel<float, AL>, st, static_cast<const float *>(p->d_w), (int)p->bs, static_cast<const float *>(r), static_cast<float *>(z), n); }, al);
    else
        with_flags([&](auto AL) { launch(precond_apply_kernel<double, AL>, st, static_cast<const double *>(p->d_w), (int)p->bs, static_cast<const double *>(r), static_cast<double *>(z), n); }, al);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

void block_jacobi_release(cvr_precond *p)
{
    if (p->d_w) (void)hipFree(p->d_w);
    p->d_w = nullptr;
}

template <typename T>
int block_jacobi_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *)
{
    with_flags([&](auto START) { launch(pcg_apply_kernel<T, START>, st, static_cast<const T *>(pc->d_w), (int)pc->bs, r, z, p, (long long)pc->n, part_rz, static_cast<const CgCell *>(cell)); }, start);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

}  // namespace

namespace cvrh {
namespace krylov {

PrecondOps kBlockJacobiOps = {kPrecondBlockJacobi,          "block-Jacobi",          block_jacobi_apply,           block_jacobi_release,          block_jacobi_cg_apply<float>,
                              block_jacobi_cg_apply<double>, block_jacobi_apply_multi, block_jacobi_cgm_apply<float>, block_jacobi_cgm_apply<double>};

// ---- the constructors' helpers (cvr_precond.h)

int device_alloc(const char *entry, void **out, size_t bytes, const char *what)
{
    const hipError_t e = hipMalloc(out, bytes ? bytes : 1);
    if (e == hipSuccess) return CVR_OK;
    *out = nullptr;
    (void)hipGetLastError();
    if (e == hipErrorOutOfMemory) return fail(CVR_ERR_NOMEM, "%s: no device memory for %s (%zu bytes)", entry, what, bytes);
    return fail(CVR_ERR_HIP, "%s: hipMalloc of %s: %s", entry, what, hipGetErrorString(e));
}

int upload(const char *entry, void **out, const void *src, size_t bytes, const char *what)
{
    if (const int rc = device_alloc(entry, out, bytes, what)) return rc;
    if (bytes) HIP_TRY(hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice));
    return CVR_OK;
}

int zeroed(const char *entry, void **out, size_t bytes, const char *what)
{
    if (const int rc = device_alloc(entry, out, bytes, what)) return rc;
    HIP_TRY(hipMemset(*out, 0, bytes ? bytes : 1));
    return CVR_OK;
}

int scratch_alloc(const char *entry, Scratch &s, void **out, size_t bytes, const char *what)
{
    if (const int rc = device_alloc(entry, out, bytes, what)) return rc;
    s.bufs.push_back(*out);
    return CVR_OK;
}

int check_device_view(const char *entry, const cvr_csr_view *c, std::vector<int64_t> &rp_host, hipStream_t st)
{
    const int64_t n = c->nrows;
    try {
        rp_host.assign((size_t)n + 1, 0);
    } catch (const std::bad_alloc &) {
        return fail(CVR_ERR_NOMEM, "%s: out of host memory for row_ptr (%lld rows)", entry, (long long)n);
    }
    if (n > 0) {
        if (!c->row_ptr) return fail(CVR_ERR_INVALID, "row_ptr is null");
        HIP_TRY(hipMemcpyAsync(rp_host.data(), c->row_ptr, sizeof(int64_t) * rp_host.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    cvr_csr_view hv = *c;
    hv.row_ptr = rp_host.data();
    if (const int rc = check_csr(&hv, false)) return rc;
    if (n > 0) return check_columns_device(c->col_idx, rp_host.front(), rp_host.back(), c->ncols);
    return CVR_OK;
}

int stage_host(const char *entry, const cvr_csr_view *c, HostCsr &h, bool with_values, hipStream_t st)
{
    const int64_t n = c->nrows;
    if (!c->arrays_on_device) {
        if (const int rc = check_csr(c, true)) return rc;
        h.rp = c->row_ptr;
        h.ci = c->col_idx;
        h.va = c->vals;
        return CVR_OK;
    }
    if (const int rc = check_device_view(entry, c, h.rp_own, st)) return rc;
    h.rp = h.rp_own.data();
    if (n > 0) {
        const int64_t j1 = h.rp_own.back(), j0 = with_values ? h.rp_own.front() : 0, nnz = j1 - j0;
        const size_t  vsz = c->is_f32 ? 4 : 8;
        try {
            h.ci_own.assign((size_t)j1, 0);
            if (with_values) h.va_own.assign(vsz * (size_t)j1, 0);
        } catch (const std::bad_alloc &) {
            return fail(CVR_ERR_NOMEM, "%s: out of host memory for %s (%lld entries)", entry, with_values ? "col_idx and vals" : "col_idx", (long long)nnz);
        }
        if (nnz > 0) {
            if (with_values && !c->vals) return fail(CVR_ERR_INVALID, "vals is null");
            HIP_TRY(hipMemcpy(h.ci_own.data() + j0, c->col_idx + j0, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost));
            if (with_values)
                HIP_TRY(hipMemcpy(h.va_own.data() + vsz * (size_t)j0, static_cast<const uint8_t *>(c->vals) + vsz * (size_t)j0, vsz * (size_t)nnz, hipMemcpyDeviceToHost));
        }
    }
    h.ci = h.ci_own.data();
    if (with_values) h.va = h.va_own.data();
    return CVR_OK;
}

int make_handle(cvr_handle **out, const cvr_csr_view &device_view, int device, int transpose, int nvec)
{
    cvr_options opt;
    cvr_default_options(&opt);
    opt.device = device;
    opt.transpose = transpose;
    if (nvec >= 2) opt.nvec = nvec;
    if (const int rc = cvr_create(out, &device_view, &opt)) {
        *out = nullptr;
        return rc;
    }
    return cvr_preprocess(*out, 0, nullptr);
}

int abandon(cvr_precond *p, int rc)
{
    const int device = p->device;
    char      keep[sizeof(g_err)];
    memcpy(keep, g_err, sizeof(keep));
    cvr_precond_destroy(p);
    memcpy(g_err, keep, sizeof(keep));
    (void)hipSetDevice(device);
    return rc;
}

}  // namespace krylov
}  // namespace cvrh

extern "C" {

int cvr_precond_block_jacobi(cvr_precond **out, const cvr_csr_view *csr, int32_t block_size, int32_t device, void *stream)
{
    if (!out || !csr) return fail(CVR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (block_size < 1 || block_size > CVR_PRECOND_MAX_BLOCK) return fail(CVR_ERR_INVALID, "block_size = %d: must be 1 .. %d", block_size, CVR_PRECOND_MAX_BLOCK);
    if (csr->nrows != csr->ncols) return fail(CVR_ERR_INVALID, "block-Jacobi needs a square matrix (%lld x %lld)", (long long)csr->nrows, (long long)csr->ncols);
    if (csr->nrows < 0) return fail(CVR_ERR_INVALID, "null or negative-size CSR view");
    if (device < 0 || device >= cvr_device_count()) return fail(CVR_ERR_NO_DEVICE, "device %d of %d", device, cvr_device_count());
    Range range("cvr_precond_block_jacobi");
    HIP_TRY(hipSetDevice(device));
    cvr_precond *p = new (std::nothrow) cvr_precond;
    if (!p) return fail(CVR_ERR_NOMEM, "out of host memory");
    p->ops = &kBlockJacobiOps;
    p->device = device;
    p->n = csr->nrows;
    p->bs = block_size;
    p->is_f32 = csr->is_f32 ? 1 : 0;
    p->nblocks = (csr->nrows + block_size - 1) / block_size;
    if (const int rc = build(p, csr, (hipStream_t)stream)) return abandon(p, rc);
    *out = p;
    return CVR_OK;
}

int cvr_precond_get_info(const cvr_precond *p, cvr_precond_info *info)
{
    if (!p || !info) return fail(CVR_ERR_INVALID, "null argument");
    memset(info, 0, sizeof(*info));
    info->n = p->n;
    info->block_size = p->bs;
    info->is_f32 = p->is_f32;
    info->nblocks = p->nblocks;
    info->identity_blocks = p->identity_blocks;
    info->device = p->device;
    return CVR_OK;
}

int cvr_precond_export(const cvr_precond *p, void *blocks_host)
{
    if (!p || !blocks_host) return fail(CVR_ERR_INVALID, "null argument");
    if (const int rc = check_block_jacobi(p, "cvr_precond_export")) return rc;
    if (p->nblocks == 0) return CVR_OK;
    HIP_TRY(hipSetDevice(p->device));
    const size_t vsz = p->is_f32 ? 4 : 8, bs = (size_t)p->bs, count = (size_t)p->nblocks * bs * bs;
    std::vector<uint8_t> t;
    try {
        t.resize(count * vsz);
    } catch (const std::bad_alloc &) {
        return fail(CVR_ERR_NOMEM, "cvr_precond_export: out of host memory for %zu bytes", count * vsz);
    }
    HIP_TRY(hipMemcpy(t.data(), p->d_w, count * vsz, hipMemcpyDeviceToHost));
    uint8_t *o = static_cast<uint8_t *>(blocks_host);
    for (size_t k = 0; k < (size_t)p->nblocks; k++)
        for (size_t i = 0; i < bs; i++)
            for (size_t j = 0; j < bs; j++) memcpy(o + ((k * bs + i) * bs + j) * vsz, t.data() + ((k * bs + j) * bs + i) * vsz, vsz);
    return CVR_OK;
}

int cvr_precond_apply_device(const cvr_precond *p, const void *r_dev, void *z_dev, void *stream)
{
    if (!p || !r_dev || !z_dev) return fail(CVR_ERR_INVALID, "null argument");
    if (r_dev == z_dev) return fail(CVR_ERR_INVALID, "cvr_precond_apply_device: r and z are the same array");
    if (p->n == 0) return CVR_OK;
    HIP_TRY(hipSetDevice(p->device));
    return p->ops->apply(p, r_dev, z_dev, (hipStream_t)stream);
}

int cvr_precond_destroy(cvr_precond *p)
{
    if (!p) return CVR_OK;
    (void)hipSetDevice(p->device);
    p->ops->release(p);
    delete p;
    return CVR_OK;
}

}  // extern "C"
