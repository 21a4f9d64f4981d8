// cvr_chebyshev.hip -- the Chebyshev polynomial preconditioner, the second kind of cvr_precond (include/cvr_amd.h: cvr_precond_chebyshev,
// cvr_precond_chebyshev_info, cvr_chebyshev_bounds).  z = p_d(A) r is the Chebyshev iteration for A z = r
// from z = 0 with fixed coefficients: degree - 1 products q = A z through run_spmv (cvr_spmv_device's path) on the borrowed handle, each followed by
// one element-wise kernel on the solvers' grid; no dot product, no read-back -- the scalars a[k], b[k] are computed once on the host.
//   cheb_first_kernel   step 0:      d = T(c0 r), z = d
//   cheb_step_kernel    step k >= 1: d = T(a[k] d + b[k] (r - q)), z = T(z + d)
// Both come in four modes: kInner (z goes to the object's zi: an earlier step), kLast (z goes to the caller's array: the last step of
// cvr_precond_apply_device), kSolve and kSolveStart (the last step inside cvr_pcg_device: z goes to the solver's buffer with the partial sums of
// r . z in set 1, what pcg_apply_kernel forms; at the start p = z too; behind a stop nothing is written).  With degree = 1 step 0 is the last.
// The solver is cvr_cg.hip's cg_solve, which enqueues this apply through kChebyshevOps' cg_apply (cvr_precond.h) between cg_update_kernel<T, false, AL>
// and cg_direction_kernel<T, true>: 3 + degree vector launches and degree SpMVs per step.  This file launches no cg_* kernel and holds no solve loop
// (cvr_cg_kernels.h is included for the state cell the kSolve kernels read).
// (The reference has no solver and no preconditioner: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_cg_kernels.h"
#include "cvr_precond.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace cvrh {
namespace krylov {

struct Chebyshev {
    cvr_handle *h = nullptr;          // borrowed
    int32_t     degree = 0;
    double      lmin = 0, lmax = 0, a[CVR_CHEBYSHEV_MAX_DEGREE] = {}, b[CVR_CHEBYSHEV_MAX_DEGREE] = {};
    void       *d_zi = nullptr, *d_q = nullptr, *d_d = nullptr;          // z between the steps (x_ext values, element ncols stays 0), q = A z (y_ext), d (n)
};

}  // namespace krylov
}  // namespace cvrh

namespace {

enum Mode { kInner, kLast, kSolve, kSolveStart };

// What a step's kernel does with z of a packet, by mode.  zi: the object's buffer, out: the caller's z (kLast) or the solver's (kSolve, kSolveStart).
// AL: the caller's arrays (r, and z of kLast) are 16-byte aligned; the library's always are.
template <typename T, Mode M, bool AL>
__device__ __forceinline__ void put_z(T *zi, T *out, T *p, long long e, int cnt, const T (&rv)[kPack<T>], const T (&zv)[kPack<T>], double &acc)
{
    if constexpr (M == kInner) store_pack<T, true>(zi, e, cnt, zv);
    else if constexpr (M == kLast) store_pack<T, AL>(out, e, cnt, zv);
    else {
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) if (j < cnt) acc += (double)rv[j] * (double)zv[j];
        store_pack<T, true>(out, e, cnt, zv);
        if constexpr (M == kSolveStart) store_pack<T, true>(p, e, cnt, zv);
    }
}

// Step 0: d = T(c0 * double(r)), z = d.  (d is kept only where a later step reads it: kInner.)
template <typename T, Mode M, bool AL>
__global__ __launch_bounds__(kThreads) void cheb_first_kernel(const T *__restrict__ r, T *__restrict__ d, T *zi, T *out, T *p, long long n, double c0,
                                                              double *__restrict__ part, const CgCell *__restrict__ cell)
{
    __shared__ double sh[1][kWaves];
    if constexpr (M == kSolve)
        if (cell->stop) return;          // (no workgroup of this kernel sets it)
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T rv[kPack<T>], dv[kPack<T>];
        load_pack<T, AL>(r, e, (int)cnt, rv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) dv[j] = (T)(c0 * (double)rv[j]);
        if constexpr (M == kInner) store_pack<T, true>(d, e, (int)cnt, dv);
        put_z<T, M, AL>(zi, out, p, e, (int)cnt, rv, dv, acc[0]);
    }
    if constexpr (M == kSolve || M == kSolveStart) store_partials<1>(acc, part, sh);
}

// Step k >= 1, behind q = A z: d = T(a * double(d) + b * (double(r) - double(q))), z = T(double(z) + double(d)); z is read from zi
template <typename T, Mode M, bool AL>
__global__ __launch_bounds__(kThreads) void cheb_step_kernel(const T *__restrict__ r, const T *__restrict__ q, T *__restrict__ d, T *zi, T *out, T *p, long long n,
                                                             double a, double b, double *__restrict__ part, const CgCell *__restrict__ cell)
{
    __shared__ double sh[1][kWaves];
    if constexpr (M == kSolve)
        if (cell->stop) return;          // (no workgroup of this kernel sets it)
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T rv[kPack<T>], qv[kPack<T>], dv[kPack<T>], zv[kPack<T>];
        load_pack<T, AL>(r, e, (int)cnt, rv);
        load_pack<T, true>(q, e, (int)cnt, qv);
        load_pack<T, true>(d, e, (int)cnt, dv);
        load_pack<T, true>(zi, e, (int)cnt, zv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            dv[j] = (T)(a * (double)dv[j] + b * ((double)rv[j] - (double)qv[j]));
            zv[j] = (T)((double)zv[j] + (double)dv[j]);
        }
        if constexpr (M == kInner) store_pack<T, true>(d, e, (int)cnt, dv);
        put_z<T, M, AL>(zi, out, p, e, (int)cnt, rv, zv, acc[0]);
    }
    if constexpr (M == kSolve || M == kSolveStart) store_partials<1>(acc, part, sh);
}

// the start vector of cvr_chebyshev_bounds: x_i = T(1 + double(uint32(i * 2654435761)) * 2^-32)
template <typename T>
__global__ __launch_bounds__(kThreads) void cheb_start_kernel(T *__restrict__ x, long long n)
{
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T xv[kPack<T>];
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) xv[j] = (T)(1.0 + (double)((uint32_t)(e + j) * 2654435761u) * 0x1p-32);
        store_pack<T, true>(x, e, (int)cnt, xv);
    }
}

// One apply enqueued on `st`: step 0 .. degree - 1, the last of them in mode `last` (kLast, kSolve or kSolveStart) with z going to `out`.
// AL: r (and `out` of kLast) are 16-byte aligned.  *spmvs grows by the products enqueued.
template <typename T, Mode LASTMODE, bool AL>
int enqueue_apply(const cvr_precond *pc, const T *r, T *out, T *p, double *part, const CgCell *cell, hipStream_t st, int *spmvs)
{
    const Chebyshev *c = pc->cheb;
    const long long  n = pc->n;
    T *zi = static_cast<T *>(c->d_zi), *q = static_cast<T *>(c->d_q), *d = static_cast<T *>(c->d_d);
    if (c->degree == 1) {
        launch(cheb_first_kernel<T, LASTMODE, AL>, st, r, d, zi, out, p, n, c->b[0], part, cell);
        HIP_TRY(hipGetLastError());
        return CVR_OK;
    }
    launch(cheb_first_kernel<T, kInner, AL>, st, r, d, zi, out, p, n, c->b[0], part, cell);
    HIP_TRY(hipGetLastError());
    for (int k = 1; k < c->degree; k++) {
        HIP_TRY(run_spmv(c->h, zi, q, st));
        if (spmvs) ++*spmvs;
        if (k + 1 < c->degree) launch(cheb_step_kernel<T, kInner, AL>, st, r, (const T *)q, d, zi, out, p, n, c->a[k], c->b[k], part, cell);
        else launch(cheb_step_kernel<T, LASTMODE, AL>, st, r, (const T *)q, d, zi, out, p, n, c->a[k], c->b[k], part, cell);
        HIP_TRY(hipGetLastError());
    }
    return CVR_OK;
}

// ---- the object

// the three buffers, zeroed (zi[ncols] == 0 from here on: the kernels write values 0 .. n - 1 only)
int cheb_buffers(Chebyshev *c)
{
    const size_t bytes[3] = {x_ext_bytes(c->h), y_ext_bytes(c->h), vec_bytes(c->h)};
    void       **bufs[3] = {&c->d_zi, &c->d_q, &c->d_d};
    const char  *names[3] = {"zi", "q", "d"};
    for (int i = 0; i < 3; i++)
        if (const int rc = zeroed("cvr_precond_chebyshev", bufs[i], bytes[i], names[i])) return rc;
    HIP_TRY(hipDeviceSynchronize());          // (whatever stream the first apply comes on finds them zeroed)
    return CVR_OK;
}

template <typename T>
int chebyshev_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *spmvs)
{
    if (start) return enqueue_apply<T, kSolveStart, true>(pc, r, z, p, part_rz, static_cast<const CgCell *>(cell), st, spmvs);
    return enqueue_apply<T, kSolve, true>(pc, r, z, p, part_rz, static_cast<const CgCell *>(cell), st, spmvs);
}

}  // namespace

namespace cvrh {
namespace krylov {

int chebyshev_apply(const cvr_precond *p, const void *r, void *z, hipStream_t st)
{
    const bool al = (((uintptr_t)r | (uintptr_t)z) & 15u) == 0;
    if (p->is_f32)
        return with_flags([&](auto AL) { return enqueue_apply<float, kLast, AL>(p, static_cast<const float *>(r), static_cast<float *>(z), (float *)nullptr, (double *)nullptr, (const CgCell *)nullptr, st, nullptr); }, al);
    return with_flags([&](auto AL) { return enqueue_apply<double, kLast, AL>(p, static_cast<const double *>(r), static_cast<double *>(z), (double *)nullptr, (double *)nullptr, (const CgCell *)nullptr, st, nullptr); }, al);
}

void chebyshev_release(cvr_precond *p)
{
    Chebyshev *c = p->cheb;
    if (!c) return;
    for (void *buf : {c->d_zi, c->d_q, c->d_d})
        if (buf) (void)hipFree(buf);
    delete c;
    p->cheb = nullptr;
}

PrecondOps kChebyshevOps = {kPrecondChebyshev, "Chebyshev", chebyshev_apply, chebyshev_release, chebyshev_cg_apply<float>, chebyshev_cg_apply<double>};

}  // namespace krylov
}  // namespace cvrh

extern "C" {

int cvr_precond_chebyshev(cvr_precond **out, cvr_handle *h, int32_t degree, double lmin, double lmax)
{
    if (!out || !h) return fail(CVR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (degree < 1 || degree > CVR_CHEBYSHEV_MAX_DEGREE) return fail(CVR_ERR_INVALID, "degree = %d: must be 1 .. %d", degree, CVR_CHEBYSHEV_MAX_DEGREE);
    if (!std::isfinite(lmin) || !std::isfinite(lmax) || !(lmin > 0) || !(lmin < lmax))
        return fail(CVR_ERR_INVALID, "cvr_precond_chebyshev: bounds lmin = %g, lmax = %g: must be finite with 0 < lmin < lmax", lmin, lmax);
    if (const int rc = check_square_preprocessed(h, "cvr_precond_chebyshev", "a Chebyshev preconditioner needs")) return rc;
    Range range("cvr_precond_chebyshev");
    HIP_TRY(hipSetDevice(h->device));
    cvr_precond *p = new (std::nothrow) cvr_precond;
    Chebyshev   *c = new (std::nothrow) Chebyshev;
    if (!p || !c) {
        delete p;
        delete c;
        return fail(CVR_ERR_NOMEM, "out of host memory");
    }
    p->kind = kPrecondChebyshev;
    p->ops = &kChebyshevOps;
    p->device = h->device;
    p->n = h->info.nrows;
    p->bs = 0;
    p->is_f32 = h->vsz == 4 ? 1 : 0;
    p->cheb = c;
    c->h = h;
    c->degree = degree;
    c->lmin = lmin;
    c->lmax = lmax;
    // the coefficients: every operation an fp64 one of its own (the file is compiled without contraction)
    const double theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta;
    double       rho = 1 / sigma;
    c->a[0] = 0;
    c->b[0] = 1 / theta;
    for (int k = 1; k < degree; k++) {
        const double next = 1 / (2 * sigma - rho);
        c->a[k] = next * rho;
        c->b[k] = 2 * next / delta;
        rho = next;
    }
    if (const int rc = cheb_buffers(c)) return abandon(p, rc);
    *out = p;
    return CVR_OK;
}

int cvr_precond_chebyshev_info(const cvr_precond *p, cvr_chebyshev_info *info)
{
    if (!p || !info) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondChebyshev) return fail(CVR_ERR_INVALID, "cvr_precond_chebyshev_info: the preconditioner is of kind %d (%s), not a Chebyshev object", p->kind, p->ops->name);
    const Chebyshev *c = p->cheb;
    memset(info, 0, sizeof(*info));
    info->degree = c->degree;
    info->is_f32 = p->is_f32;
    info->lmin = c->lmin;
    info->lmax = c->lmax;
    for (int k = 0; k < c->degree; k++) {
        info->a[k] = c->a[k];
        info->b[k] = c->b[k];
    }
    return CVR_OK;
}

int cvr_chebyshev_bounds(cvr_handle *h, int32_t power_iters, double eig_ratio, double *lmin, double *lmax, void *stream)
{
    if (!h || !lmin || !lmax) return fail(CVR_ERR_INVALID, "null argument");
    if (power_iters < 0) return fail(CVR_ERR_INVALID, "cvr_chebyshev_bounds: power_iters = %d: must not be negative", power_iters);
    if (!std::isfinite(eig_ratio) || !(eig_ratio > 1)) return fail(CVR_ERR_INVALID, "cvr_chebyshev_bounds: eig_ratio = %g: must be finite and > 1", eig_ratio);
    if (const int rc = check_square_preprocessed(h, "cvr_chebyshev_bounds", "the bounds need")) return rc;
    HIP_TRY(hipSetDevice(h->device));
    const hipStream_t st = (hipStream_t)stream;
    const long long   n = h->info.nrows;
    struct Buf { void *p = nullptr; ~Buf() { if (p) (void)hipFree(p); } } x;
    HIP_TRY(hipMalloc(&x.p, x_ext_bytes(h)));
    HIP_TRY(hipMemsetAsync(x.p, 0, x_ext_bytes(h), st));
    if (h->vsz == 4) launch(cheb_start_kernel<float>, st, static_cast<float *>(x.p), n);
    else launch(cheb_start_kernel<double>, st, static_cast<double *>(x.p), n);
    HIP_TRY(hipGetLastError());
    double lambda = 0, seconds = 0;
    if (const int rc = cvr_power_iteration(h, nullptr, nullptr, power_iters, x.p, &lambda, &seconds, stream)) return rc;
    HIP_TRY(hipStreamSynchronize(st));          // (the buffer is released behind everything that reads it)
    if (!std::isfinite(lambda) || !(lambda > 0)) return fail(CVR_ERR_STATE, "cvr_chebyshev_bounds: the Rayleigh quotient after %d power steps is %g: not finite or not > 0", power_iters, lambda);
    *lmax = CVR_CHEBYSHEV_LMAX_FACTOR * lambda;
    *lmin = *lmax / eig_ratio;
    return CVR_OK;
}

}  // extern "C"
