// cvr_bicg_kernels.h -- the state cell and the vector kernels of BiCGSTAB (cvr_bicgstab.hip: cvr_bicgstab_device, cvr_pbicgstab_device).  What each
// kernel does: cvr_bicgstab.hip's head.
#pragma once
#include "cvr_krylov.h"

namespace cvrh {
namespace krylov {
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

}  // namespace
}  // namespace krylov
}  // namespace cvrh
