// cvr_bicgstab.hip -- BiCGSTAB on the device for nonsymmetric A (include/cvr_amd.h: cvr_bicgstab_device, cvr_bicgstab): cvr_cg.hip's plan with the
// other recurrence.  Right-preconditioned, shadow residual r^ = r0; per step two SpMVs through run_spmv (cvr_spmv_device's path) and five vector launches:
//   v = A p^
//   bicg_rv_kernel         the partial sums of r^ . v
//   bicg_s_kernel          alpha = rho / (r^ . v) from those partials (summed in every workgroup, the same order everywhere); s = r - alpha v,
//                          s^ = minv .* s and the partial sums of s . s
//   t = A s^
//   bicg_half_kernel       ||s|| <= rtol ||b||: x += alpha p^, the stop recorded (the half step); else the partial sums of t . s and t . t
//   bicg_update_kernel     omega = (t . s) / (t . t); x += alpha p^ + omega s^, r = s - omega t and the partial sums of r . r and r^ . r
//   bicg_direction_kernel  the stop test; beta = (rho' / rho)(alpha / omega); p = r + beta (p - omega v), p^ = minv .* p
// 18 vector passes per step (r^ v | r v s | t s | x p s t r^ x r | r p v p), 23 with a preconditioner, all in 16-byte packets; the sums, the grid and
// the packet helpers are cvr_krylov.h's, so a call gives the same bits every time.  The scalars that outlive a kernel sit in a state cell (BiCell) that
// workgroup 0 writes: the kernel that finds a stop records it there and every later kernel of the batch returns without writing -- the result does not
// depend on how many steps the host enqueues between two read-backs.
// The host side is cvr_krylov.h's driver: this file adds the cell, the kernels, the step and the read-back.
// (The reference has no solver: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

// The state cell.  Written by thread 0 of workgroup 0 only; a value a kernel reads is one that a kernel BEFORE it wrote (rho of this step sits in
// rho[k & 1], the next one's goes to rho[(k + 1) & 1]) -- except `stop`, which the other workgroups of the kernel that sets it may or may not see
// yet: they come to the same decision from the same sums, so either way they return without writing.  The half-step stop is the one decision behind
// which the deciding kernel still writes (x += alpha p^), so it has a flag of its own that the deciding launch does not take for a stop: `half`.
struct BiCell {
    double  bb, bnorm;         // b . b and its root
    double  rr, rnorm;         // r . r (s . s at a half-step stop) of the last iterate and its root
    double  rho[2];            // r^ . r
    double  alpha, omega;      // of the step under way: bicg_s_kernel and bicg_update_kernel write them, the kernels behind read them
    int32_t stop;              // != 0: no kernel writes a vector any more
    int32_t half;              // k + 1: stopped at the half step of step k (every kernel but that step's bicg_half_kernel treats it as `stop`)
    int32_t status;            // CVR_CG_*
    int32_t iters;             // steps applied to x
    int32_t zero_x;            // b == 0: the solution is x = 0 (the host clears it)
    int32_t pad;
};

// The start: r holds b - A x0 (the scaled product).  r^ = r, p = r, p^ = minv .* p (PRE), and the partial sums of r . r (= r^ . r) and b . b.
// AL: b and minv, the caller's arrays, are 16-byte aligned.
template <typename T, bool PRE, bool AL>
__global__ __launch_bounds__(kThreads) void bicg_init_kernel(const T *__restrict__ b, const T *__restrict__ minv, const T *__restrict__ r, T *__restrict__ rhat,
                                                             T *__restrict__ p, T *__restrict__ phat, long long n, double *__restrict__ out)
{
    __shared__ double sh[2][kWaves];
    double acc[2] = {0, 0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T bv[kPack<T>], rv[kPack<T>], mv[kPack<T>], hv[kPack<T>];
        load_pack<T, AL>(b, e, (int)cnt, bv);
        load_pack<T, true>(r, e, (int)cnt, rv);
        if constexpr (PRE) load_pack<T, AL>(minv, e, (int)cnt, mv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            if constexpr (PRE) hv[j] = (T)((double)mv[j] * (double)rv[j]);
            if (j < cnt) {
                acc[0] += (double)rv[j] * (double)rv[j];
                acc[1] += (double)bv[j] * (double)bv[j];
            }
        }
        store_pack<T, true>(rhat, e, (int)cnt, rv);
        store_pack<T, true>(p, e, (int)cnt, rv);
        if constexpr (PRE) store_pack<T, true>(phat, e, (int)cnt, hv);
    }
    store_partials<2>(acc, out, sh);
}

// one workgroup: the start's sums into the state cell, and the stop test of the start vector
__global__ __launch_bounds__(kThreads) void bicg_check_kernel(const double *__restrict__ part, double rtol, BiCell *__restrict__ cell)
{
    __shared__ double sh[2][kWaves];
    double s[2];
    sum_partials<2>(part, s, sh);
    if (threadIdx.x != 0) return;
    BiCell c;
    c.bb = s[1]; c.bnorm = sqrt(s[1]);
    c.rr = s[0]; c.rnorm = sqrt(s[0]);
    c.rho[0] = s[0]; c.rho[1] = 0;
    c.alpha = 0; c.omega = 0;
    c.stop = 0; c.half = 0; c.status = CVR_CG_MAX_ITERS; c.iters = 0; c.zero_x = 0; c.pad = 0;
    if (c.bb == 0) { c.zero_x = 1; c.rr = 0; c.rnorm = 0; c.status = CVR_CG_CONVERGED; c.stop = 1; }
    // (a residual norm that is not finite never counts as converged, although Inf <= rtol * Inf holds: step 0 then finds r^ . v not finite and
    // records the breakdown)
    else if (c.rnorm <= rtol * c.bnorm && c.rnorm <= kDblMax) { c.status = CVR_CG_CONVERGED; c.stop = 1; }
    *cell = c;
}

// the partial sums of r^ . v
template <typename T>
__global__ __launch_bounds__(kThreads) void bicg_rv_kernel(const T *__restrict__ rhat, const T *__restrict__ v, long long n, double *__restrict__ out,
                                                           const BiCell *__restrict__ cell)
{
    __shared__ double sh[1][kWaves];
    if (cell->stop | cell->half) return;          // (no workgroup of this kernel sets them)
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T hv[kPack<T>], vv[kPack<T>];
        load_pack<T, true>(rhat, e, (int)cnt, hv);
        load_pack<T, true>(v, e, (int)cnt, vv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) if (j < cnt) acc[0] += (double)hv[j] * (double)vv[j];
    }
    store_partials<1>(acc, out, sh);
}

// Step k: alpha = rho / (r^ . v); s = r - alpha v, s^ = minv .* s (PRE); the partial sums of s . s.  r^ . v zero or not finite: breakdown, recorded,
// nothing written.  AL: minv, the caller's array, is 16-byte aligned.
template <typename T, bool PRE, bool AL>
__global__ __launch_bounds__(kThreads) void bicg_s_kernel(const T *__restrict__ r, const T *__restrict__ v, const T *__restrict__ minv, T *__restrict__ s,
                                                          T *__restrict__ shat, long long n, const double *__restrict__ part_rv, double *__restrict__ out,
                                                          BiCell *__restrict__ cell, int k)
{
    __shared__ double shp[1][kWaves];
    __shared__ double sh[1][kWaves];
    __shared__ int stopped;
    if (threadIdx.x == 0) stopped = cell->stop | cell->half;
    double rv[1];
    sum_partials<1>(part_rv, rv, shp);
    if (stopped) return;
    if (!usable(rv[0])) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { cell->status = CVR_CG_BREAKDOWN; cell->stop = 1; }
        return;
    }
    const double alpha = cell->rho[k & 1] / rv[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) cell->alpha = alpha;
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T rr[kPack<T>], vv[kPack<T>], mv[kPack<T>], sv[kPack<T>], hv[kPack<T>];
        load_pack<T, true>(r, e, (int)cnt, rr);
        load_pack<T, true>(v, e, (int)cnt, vv);
        if constexpr (PRE) load_pack<T, AL>(minv, e, (int)cnt, mv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            sv[j] = (T)((double)rr[j] - alpha * (double)vv[j]);
            if constexpr (PRE) hv[j] = (T)((double)mv[j] * (double)sv[j]);
            if (j < cnt) acc[0] += (double)sv[j] * (double)sv[j];
        }
        store_pack<T, true>(s, e, (int)cnt, sv);
        if constexpr (PRE) store_pack<T, true>(shat, e, (int)cnt, hv);
    }
    store_partials<1>(acc, out, sh);
}

// Step k, behind t = A s^: s . s from its partials; ||s|| <= rtol ||b||: x += alpha p^, converged at the half step, recorded in `half` (which this
// launch does not take for a stop: every workgroup applies its share of the half step); else the partial sums of t . s (set 0) and t . t (set 1).
// AL: x, the caller's array, is 16-byte aligned.
template <typename T, bool AL>
__global__ __launch_bounds__(kThreads) void bicg_half_kernel(T *__restrict__ x, const T *__restrict__ phat, const T *__restrict__ s, const T *__restrict__ t,
                                                             long long n, const double *__restrict__ part_ss, double *__restrict__ out, BiCell *__restrict__ cell,
                                                             int k, double rtol)
{
    __shared__ double shp[1][kWaves];
    __shared__ double sh[2][kWaves];
    __shared__ int stopped;
    if (threadIdx.x == 0) stopped = cell->stop | (cell->half != 0 && cell->half != k + 1);          // (k + 1: workgroup 0 of this launch, just now)
    double ss[1];
    sum_partials<1>(part_ss, ss, shp);
    if (stopped) return;
    const double snorm = sqrt(ss[0]);
    if (snorm <= rtol * cell->bnorm && snorm <= kDblMax) {
        const double alpha = cell->alpha;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            cell->rr = ss[0]; cell->rnorm = snorm; cell->iters = k + 1;
            cell->status = CVR_CG_CONVERGED; cell->half = k + 1;
        }
        CVR_KRYLOV_PACKETS(T, e, cnt) {
            T xv[kPack<T>], pv[kPack<T>];
            load_pack<T, AL>(x, e, (int)cnt, xv);
            load_pack<T, true>(phat, e, (int)cnt, pv);
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) xv[j] = (T)((double)xv[j] + alpha * (double)pv[j]);
            store_pack<T, AL>(x, e, (int)cnt, xv);
        }
        return;
    }
    double acc[2] = {0, 0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T sv[kPack<T>], tv[kPack<T>];
        load_pack<T, true>(s, e, (int)cnt, sv);
        load_pack<T, true>(t, e, (int)cnt, tv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++)
            if (j < cnt) {
                acc[0] += (double)tv[j] * (double)sv[j];
                acc[1] += (double)tv[j] * (double)tv[j];
            }
    }
    store_partials<2>(acc, out, sh);
}

// Step k: omega = (t . s) / (t . t); x += alpha p^ + omega s^, r = s - omega t; the partial sums of r . r (set 0) and r^ . r (set 1).  t . t or omega
// zero or not finite: breakdown, recorded, nothing written.  Without a preconditioner s^ is s (one load).  AL: x is 16-byte aligned.
template <typename T, bool PRE, bool AL>
__global__ __launch_bounds__(kThreads) void bicg_update_kernel(T *__restrict__ x, T *__restrict__ r, const T *__restrict__ phat, const T *__restrict__ shat,
                                                               const T *__restrict__ s, const T *__restrict__ t, const T *__restrict__ rhat, long long n,
                                                               const double *__restrict__ part_t, double *__restrict__ out, BiCell *__restrict__ cell, int k)
{
    __shared__ double shp[2][kWaves];
    __shared__ double sh[2][kWaves];
    __shared__ int stopped;
    if (threadIdx.x == 0) stopped = cell->stop | cell->half;
    double ts[2];
    sum_partials<2>(part_t, ts, shp);
    if (stopped) return;
    const double omega = ts[0] / ts[1];
    if (!usable(ts[1]) || !usable(omega)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { cell->status = CVR_CG_BREAKDOWN; cell->stop = 1; }
        return;
    }
    const double alpha = cell->alpha;
    if (blockIdx.x == 0 && threadIdx.x == 0) { cell->omega = omega; cell->iters = k + 1; }
    double acc[2] = {0, 0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T xv[kPack<T>], pv[kPack<T>], hv[kPack<T>], sv[kPack<T>], tv[kPack<T>], qv[kPack<T>], rv[kPack<T>];
        load_pack<T, AL>(x, e, (int)cnt, xv);
        load_pack<T, true>(phat, e, (int)cnt, pv);
        load_pack<T, true>(s, e, (int)cnt, sv);
        if constexpr (PRE) load_pack<T, true>(shat, e, (int)cnt, hv);
        load_pack<T, true>(t, e, (int)cnt, tv);
        load_pack<T, true>(rhat, e, (int)cnt, qv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            const double sh_j = PRE ? (double)hv[j] : (double)sv[j];
            xv[j] = (T)(((double)xv[j] + alpha * (double)pv[j]) + omega * sh_j);
            rv[j] = (T)((double)sv[j] - omega * (double)tv[j]);
            if (j < cnt) {
                acc[0] += (double)rv[j] * (double)rv[j];
                acc[1] += (double)qv[j] * (double)rv[j];
            }
        }
        store_pack<T, AL>(x, e, (int)cnt, xv);
        store_pack<T, true>(r, e, (int)cnt, rv);
    }
    store_partials<2>(acc, out, sh);
}

// Step k, behind the update: r . r and rho' = r^ . r from its partials into the cell; ||r|| <= rtol ||b||: converged, recorded, nothing written; rho'
// zero or not finite: breakdown, recorded, nothing written; else beta = (rho' / rho)(alpha / omega), p = r + beta (p - omega v), p^ = minv .* p (PRE).
// AL: minv is 16-byte aligned.
template <typename T, bool PRE, bool AL>
__global__ __launch_bounds__(kThreads) void bicg_direction_kernel(T *__restrict__ p, T *__restrict__ phat, const T *__restrict__ r, const T *__restrict__ v,
                                                                  const T *__restrict__ minv, long long n, const double *__restrict__ part, BiCell *__restrict__ cell,
                                                                  int k, double rtol)
{
    __shared__ double sh[2][kWaves];
    __shared__ int stopped;
    if (threadIdx.x == 0) stopped = cell->stop | cell->half;
    double s[2];
    sum_partials<2>(part, s, sh);
    if (stopped) return;
    const double rr = s[0], rho1 = s[1], rnorm = sqrt(rr);
    const bool   done = rnorm <= rtol * cell->bnorm && rnorm <= kDblMax;
    const bool   broken = !done && !usable(rho1);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cell->rr = rr; cell->rnorm = rnorm; cell->rho[(k + 1) & 1] = rho1;
        if (done) { cell->status = CVR_CG_CONVERGED; cell->stop = 1; }
        if (broken) { cell->status = CVR_CG_BREAKDOWN; cell->stop = 1; }
    }
    if (done || broken) return;
    const double omega = cell->omega;
    const double beta = (rho1 / cell->rho[k & 1]) * (cell->alpha / omega);
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T pv[kPack<T>], rv[kPack<T>], vv[kPack<T>], mv[kPack<T>], hv[kPack<T>];
        load_pack<T, true>(p, e, (int)cnt, pv);
        load_pack<T, true>(r, e, (int)cnt, rv);
        load_pack<T, true>(v, e, (int)cnt, vv);
        if constexpr (PRE) load_pack<T, AL>(minv, e, (int)cnt, mv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            pv[j] = (T)((double)rv[j] + beta * ((double)pv[j] - omega * (double)vv[j]));
            if constexpr (PRE) hv[j] = (T)((double)mv[j] * (double)pv[j]);
        }
        store_pack<T, true>(p, e, (int)cnt, pv);
        if constexpr (PRE) store_pack<T, true>(phat, e, (int)cnt, hv);
    }
}

#undef CVR_KRYLOV_PACKETS

// the library's buffers of one call: p and s (x_ext each: SpMV inputs without a preconditioner), p^ and s^ (x_ext each, with one),
// v, t and r (y_ext each: r takes the scaled product), r^, two sets of partial sums that the kernels use in turn, the cell
template <typename T>
struct Workspace {
    T      *p, *s, *phat, *shat, *v, *t, *r, *rhat;
    double *part_a, *part_b;
    BiCell *cell;
};

// step k up to the second SpMV: r^ . v, then alpha and s (the SpMV v = A p^ is enqueued in front).  (A kernel whose only caller's array is minv
// has no <T, false, false> form: AL || !PRE.)
template <typename T>
hipError_t launch_first_half(const Workspace<T> &w, const T *minv, long long n, bool al, int k, hipStream_t st)
{
    launch(bicg_rv_kernel<T>, st, w.rhat, w.v, n, w.part_a, w.cell);
    with_flags([&](auto PRE, auto AL) { launch(bicg_s_kernel<T, PRE, AL || !PRE>, st, w.r, w.v, minv, w.s, w.shat, n, w.part_a, w.part_b, w.cell, k); }, minv != nullptr, al);
    return hipGetLastError();
}

// the rest of step k (the SpMV t = A s^ is enqueued in front): the half-step test, the update, the stop test and the new direction
template <typename T>
hipError_t launch_second_half(const Workspace<T> &w, T *x, const T *minv, long long n, bool al, int k, double rtol, hipStream_t st)
{
    const T *ph = minv ? w.phat : w.p, *sh = minv ? w.shat : w.s;
    with_flags([&](auto AL) { launch(bicg_half_kernel<T, AL>, st, x, ph, w.s, w.t, n, w.part_b, w.part_a, w.cell, k, rtol); }, al);
    with_flags([&](auto PRE, auto AL) { launch(bicg_update_kernel<T, PRE, AL>, st, x, w.r, ph, sh, w.s, w.t, w.rhat, n, w.part_a, w.part_b, w.cell, k); }, minv != nullptr, al);
    with_flags([&](auto PRE, auto AL) { launch(bicg_direction_kernel<T, PRE, AL || !PRE>, st, w.p, w.phat, w.r, w.v, minv, n, w.part_b, w.cell, k, rtol); }, minv != nullptr, al);
    return hipGetLastError();
}

int check_handle(const cvr_handle *h) { return check_square_preprocessed(h, "cvr_bicgstab", "BiCGSTAB needs"); }

// cvr_krylov.h's driver with BiCGSTAB's start, step and cell
template <typename T>
int bicgstab_solve(cvr_handle *h, const T *b, T *x, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    const long long n = h->info.nrows;
    const size_t    vb = sizeof(T) * (size_t)n;
    const T        *minv = static_cast<const T *>(opt->minv_dev);
    const bool      al = (((uintptr_t)b | (uintptr_t)x | (uintptr_t)minv) & 15u) == 0;

    Arena        a;
    const size_t nx = x_ext_bytes(h), ny = y_ext_bytes(h), nh = minv ? nx : 0, npart = sizeof(double) * 2 * kBlocks;
    const size_t op = a.add(nx), os = a.add(nx), ophat = a.add(nh), oshat = a.add(nh), ov = a.add(ny), ot = a.add(ny), orr = a.add(ny), orhat = a.add(vec_bytes(h));
    const size_t oa = a.add(npart), ob = a.add(npart), ocell = a.add(sizeof(BiCell));
    HIP_TRY(a.alloc());
    const Workspace<T> w{a.at<T>(op), a.at<T>(os), minv ? a.at<T>(ophat) : nullptr, minv ? a.at<T>(oshat) : nullptr, a.at<T>(ov), a.at<T>(ot), a.at<T>(orr), a.at<T>(orhat),
                         a.at<double>(oa), a.at<double>(ob), a.at<BiCell>(ocell)};
    if (const int rc = a.begin(st)) return rc;

    // the pad slots of the SpMV inputs; p = x0 for the moment, r = b; r = b - A x0; then r^, p, p^ and the start's sums
    for (T *q : {w.p, w.s, w.phat, w.shat})
        if (q)
            if (const int rc = zero_pad_slot(q, vb, sizeof(T), st)) return rc;
    if (const int rc = start_residual(h, w.p, w.r, x, b, n, st)) return rc;
    int spmvs = 1;
    with_flags([&](auto PRE, auto AL) { launch(bicg_init_kernel<T, PRE, AL>, st, b, minv, w.r, w.rhat, w.p, w.phat, n, w.part_b); }, minv != nullptr, al);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bicg_check_kernel, dim3(1), dim3(kThreads), 0, st, w.part_b, opt->rtol, w.cell);
    HIP_TRY(hipGetLastError());

    const T  *ph = minv ? w.phat : w.p, *sh = minv ? w.shat : w.s;
    BiCell    cell{};
    const int rc = run_batches(
        opt,
        [&](int k) -> int {
            HIP_TRY(run_spmv(h, ph, w.v, st));
            HIP_TRY(launch_first_half(w, minv, n, al, k, st));
            HIP_TRY(run_spmv(h, sh, w.t, st));
            HIP_TRY(launch_second_half(w, x, minv, n, al, k, opt->rtol, st));
            spmvs += 2;
            return CVR_OK;
        },
        [&](int, bool *stopped) -> int {
            if (const int rc = read_cell(&cell, w.cell, sizeof(cell), st)) return rc;
            *stopped = cell.stop || cell.half;
            return CVR_OK;
        });
    if (rc) return rc;
    if (cell.zero_x && n) HIP_TRY(hipMemsetAsync(x, 0, vb, st));
    double seconds = 0;
    if (const int rc = a.seconds(st, &seconds)) return rc;
    fill_result(res, cell.iters, cell.status, spmvs, cell.rnorm, cell.bnorm, seconds);
    return CVR_OK;
}

// behind the argument checks
int bicgstab_device(cvr_handle *h, const void *b, void *x, const cvr_cg_options *opt, cvr_cg_result *res, hipStream_t st)
{
    if (const int rc = check_handle(h)) return rc;
    Range range("cvr_bicgstab_device");
    HIP_TRY(hipSetDevice(h->device));
    return with_value_type(h, [&](auto t) { return bicgstab_solve(h, static_cast<const decltype(t) *>(b), static_cast<decltype(t) *>(x), opt, res, st); });
}

}  // namespace

extern "C" {

int cvr_bicgstab_device(cvr_handle *h, const void *b_dev, void *x_dev, const cvr_cg_options *opt, cvr_cg_result *res, void *stream)
{
    if (const int rc = check_solver_args(h, b_dev, x_dev, opt, res)) return rc;
    return bicgstab_device(h, b_dev, x_dev, opt, res, (hipStream_t)stream);
}

int cvr_bicgstab(cvr_handle *h, const void *b_host, void *x_host, const cvr_cg_options *opt, cvr_cg_result *res)
{
    if (const int rc = check_solver_args(h, b_host, x_host, opt, res)) return rc;
    if (const int rc = check_handle(h)) return rc;
    return solve_from_host(h, b_host, x_host, [&](const void *b, void *x, hipStream_t st) { return bicgstab_device(h, b, x, opt, res, st); });
}

}  // extern "C"
