// cvr_cg_kernels.h -- the vector kernels of conjugate gradients (cvr_cg.hip: cvr_cg_device, cvr_pcg_device); the state cell they keep is
// cvr_krylov.h's CgCell.  What each kernel does: cvr_cg.hip's head.
#pragma once
#include "cvr_krylov.h"

namespace cvrh {
namespace krylov {
namespace {

// The start: r holds b - A x0 (the scaled product).  z = minv .* r (PRE), p = z (or r), and the partial sums of r . r, r . z (PRE) and b . b.
// AL: b and minv, the caller's arrays, are 16-byte aligned.
template <typename T, bool PRE, bool AL>
__global__ __launch_bounds__(kThreads) void cg_init_kernel(const T *__restrict__ b, const T *__restrict__ minv, const T *__restrict__ r, T *__restrict__ z,
                                                           T *__restrict__ p, long long n, double *__restrict__ out)
{
    __shared__ double sh[3][kWaves];
    double acc[3] = {0, 0, 0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T bv[kPack<T>], rv[kPack<T>], mv[kPack<T>], zv[kPack<T>];
        load_pack<T, AL>(b, e, (int)cnt, bv);
        load_pack<T, true>(r, e, (int)cnt, rv);
        if constexpr (PRE) load_pack<T, AL>(minv, e, (int)cnt, mv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            zv[j] = PRE ? (T)((double)mv[j] * (double)rv[j]) : rv[j];
            if (j < cnt) {
                acc[0] += (double)rv[j] * (double)rv[j];
                if constexpr (PRE) acc[1] += (double)rv[j] * (double)zv[j];
                acc[2] += (double)bv[j] * (double)bv[j];
            }
        }
        if constexpr (PRE) store_pack<T, true>(z, e, (int)cnt, zv);
        store_pack<T, true>(p, e, (int)cnt, zv);
    }
    store_partials<3>(acc, out, sh);
}

// the partial sums of p . q
template <typename T>
__global__ __launch_bounds__(kThreads) void cg_pq_kernel(const T *__restrict__ p, const T *__restrict__ q, long long n, double *__restrict__ out,
                                                         const CgCell *__restrict__ cell)
{
    __shared__ double sh[1][kWaves];
    if (cell->stop) return;          // (no workgroup of this kernel sets it)
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T pv[kPack<T>], qv[kPack<T>];
        load_pack<T, true>(p, e, (int)cnt, pv);
        load_pack<T, true>(q, e, (int)cnt, qv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) if (j < cnt) acc[0] += (double)pv[j] * (double)qv[j];
    }
    store_partials<1>(acc, out, sh);
}

// Step k: alpha = r.z / p.q; x += alpha p, r -= alpha q, z = minv .* r; the partial sums of r . r (set 0) and r . z (set 1, PRE).  p.q <= 0 or not
// finite: breakdown, recorded, nothing written.  AL: x and minv, the caller's arrays, are 16-byte aligned.
template <typename T, bool PRE, bool AL>
__global__ __launch_bounds__(kThreads) void cg_update_kernel(T *__restrict__ x, T *__restrict__ r, T *__restrict__ z, const T *__restrict__ p,
                                                             const T *__restrict__ q, const T *__restrict__ minv, long long n,
                                                             const double *__restrict__ part_pq, double *__restrict__ out, CgCell *__restrict__ cell, int k)
{
    constexpr int K = PRE ? 2 : 1;
    __shared__ double shp[1][kWaves];
    __shared__ double sh[K][kWaves];
    __shared__ int stopped;
    if (threadIdx.x == 0) stopped = cell->stop;
    double pq[1];
    sum_partials<1>(part_pq, pq, shp);
    if (stopped) return;
    if (!(pq[0] > 0) || !(pq[0] <= kDblMax)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { cell->status = CVR_CG_BREAKDOWN; cell->stop = 1; }
        return;
    }
    const double alpha = cell->rz[k & 1] / pq[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) cell->iters = k + 1;
    double acc[K] = {};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T xv[kPack<T>], rv[kPack<T>], pv[kPack<T>], qv[kPack<T>], mv[kPack<T>], zv[kPack<T>];
        load_pack<T, AL>(x, e, (int)cnt, xv);
        load_pack<T, true>(r, e, (int)cnt, rv);
        load_pack<T, true>(p, e, (int)cnt, pv);
        load_pack<T, true>(q, e, (int)cnt, qv);
        if constexpr (PRE) load_pack<T, AL>(minv, e, (int)cnt, mv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            xv[j] = (T)((double)xv[j] + alpha * (double)pv[j]);
            rv[j] = (T)((double)rv[j] - alpha * (double)qv[j]);
            if constexpr (PRE) zv[j] = (T)((double)mv[j] * (double)rv[j]);
            if (j < cnt) {
                acc[0] += (double)rv[j] * (double)rv[j];
                if constexpr (PRE) acc[1] += (double)rv[j] * (double)zv[j];
            }
        }
        store_pack<T, AL>(x, e, (int)cnt, xv);
        store_pack<T, true>(r, e, (int)cnt, rv);
        if constexpr (PRE) store_pack<T, true>(z, e, (int)cnt, zv);
    }
    store_partials<K>(acc, out, sh);
}

// Step k, behind the update: r.r and r.z from its partials into the cell; ||r|| <= rtol ||b||: converged, recorded, nothing written; else
// p = z + beta p with beta = r.z / r.z of the step before.  z is r without a preconditioner.
template <typename T, bool PRE>
__global__ __launch_bounds__(kThreads) void cg_direction_kernel(T *__restrict__ p, const T *__restrict__ z, long long n, const double *__restrict__ part,
                                                                CgCell *__restrict__ cell, int k, double rtol)
{
    constexpr int K = PRE ? 2 : 1;
    __shared__ double sh[K][kWaves];
    __shared__ int stopped;
    if (threadIdx.x == 0) stopped = cell->stop;
    double s[K];
    sum_partials<K>(part, s, sh);
    if (stopped) return;
    const double rr = s[0], rz = s[K - 1], rnorm = sqrt(rr);
    const bool   done = rnorm <= rtol * cell->bnorm;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cell->rr = rr; cell->rnorm = rnorm; cell->rz[(k + 1) & 1] = rz;
        if (done) { cell->status = CVR_CG_CONVERGED; cell->stop = 1; }
    }
    if (done) return;
    const double beta = rz / cell->rz[k & 1];
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T pv[kPack<T>], zv[kPack<T>];
        load_pack<T, true>(p, e, (int)cnt, pv);
        load_pack<T, true>(z, e, (int)cnt, zv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) pv[j] = (T)((double)zv[j] + beta * (double)pv[j]);
        store_pack<T, true>(p, e, (int)cnt, pv);
    }
}

// the library's buffers of one call: p (x_ext), q and r (y_ext each: r takes the scaled product), z, the partial sums, the cell
template <typename T>
struct Workspace {
    T      *p, *q, *r, *z;
    double *part_pq, *part;
    CgCell *cell;
};

}  // namespace
}  // namespace krylov
}  // namespace cvrh
