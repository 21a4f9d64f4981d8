// cvr_minres_kernels.h -- the state cell and the vector kernels of MINRES (cvr_minres.hip: cvr_minres_device).  What each kernel does: cvr_minres.hip's head.
#pragma once
#include "cvr_krylov.h"

namespace cvrh {
namespace krylov {
namespace {

// The scalars a step hands to the next one.  minres_x_kernel of step k reads st[k & 1] in every workgroup while thread 0 of workgroup 0 writes
// st[(k + 1) & 1], which the three kernels of step k + 1 read: no kernel reads a slot that a workgroup of the same launch writes.
struct MinresScalars {
    double beta, oldb;           // of the Lanczos process: sqrt(r2 . z) of the last step and of the one before
    double dbar, epsln, phibar;
    double cs, sn;               // the last rotation
    double tnorm2;               // the running sum of alfa^2 + oldb^2 + beta'^2
    double gmax, gmin;           // over the steps' gamma
};

// The state cell.  Written by thread 0 of workgroup 0 only.  `stop` is the one word a workgroup may read while another one of the same launch
// writes it: minres_x_kernel of step k sets it to k + 1 and does not take that value for a stop (every workgroup still applies its share of the
// step's update of x, or, at a breakdown, comes to the same decision from the same sums and returns); the start sets it to -1.
struct MinresCell {
    MinresScalars st[2];
    double  bnorm, rnorm;        // sqrt(b . M^-1 b); the residual norm of the last iterate (phibar)
    double  anorm, acond;        // cvr_minres_info's
    int32_t stop;                // != 0: no kernel writes a vector any more (k + 1: found by step k; -1: by the start)
    int32_t status;              // CVR_CG_*
    int32_t iters;               // steps applied to x
    int32_t zero_x;              // b == 0: the solution is x = 0 (the host clears it)
};

// The start: r2 holds b - A x0 (the scaled product) and x0 the start vector; with a shift r2 = T(double(r2) + shift * double(x0)), the residual of
// A - shift I.  z = T(minv * r2) (PRE) and the partial sums of b . b (set 0), b . T(minv * b) (set 1, PRE) and r2 . z (set 2; z is r2 without PRE).
// AL: b and minv, the caller's arrays, are 16-byte aligned.
template <typename T, bool PRE, bool AL>
__global__ __launch_bounds__(kThreads) void minres_init_kernel(const T *__restrict__ b, const T *__restrict__ minv, const T *__restrict__ x0, T *__restrict__ r2,
                                                               T *__restrict__ z, long long n, double shift, double *__restrict__ out)
{
    __shared__ double sh[3][kWaves];
    double acc[3] = {0, 0, 0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T bv[kPack<T>], rv[kPack<T>], mv[kPack<T>], zv[kPack<T>];
        load_pack<T, AL>(b, e, (int)cnt, bv);
        load_pack<T, true>(r2, e, (int)cnt, rv);
        if constexpr (PRE) load_pack<T, AL>(minv, e, (int)cnt, mv);
        if (shift != 0) {          // (the same in every thread)
            T xv[kPack<T>];
            load_pack<T, true>(x0, e, (int)cnt, xv);
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) rv[j] = (T)((double)rv[j] + shift * (double)xv[j]);
            store_pack<T, true>(r2, e, (int)cnt, rv);
        }
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            zv[j] = PRE ? (T)((double)mv[j] * (double)rv[j]) : rv[j];
            if (j < cnt) {
                acc[0] += (double)bv[j] * (double)bv[j];
                if constexpr (PRE) acc[1] += (double)bv[j] * (double)(T)((double)mv[j] * (double)bv[j]);
                acc[2] += (double)rv[j] * (double)zv[j];
            }
        }
        if constexpr (PRE) store_pack<T, true>(z, e, (int)cnt, zv);
    }
    store_partials<3>(acc, out, sh);
}

// The start, behind the sums: bnorm and beta into a fresh cell with the stops of the start (b == 0; r2 . z negative or not finite; beta <= rtol bnorm);
// else v = T(double(z) / beta) and the scalars of step 0.  z is r2 without a preconditioner.
template <typename T>
__global__ __launch_bounds__(kThreads) void minres_start_kernel(const T *__restrict__ z, T *__restrict__ v, long long n, const double *__restrict__ part, int pre,
                                                                MinresCell *__restrict__ cell, double rtol)
{
    __shared__ double sh[3][kWaves];
    double s[3];
    sum_partials<3>(part, s, sh);
    const double bnorm = sqrt(pre ? s[1] : s[0]), beta = sqrt(s[2]);
    const bool   zero = s[0] == 0, broken = !zero && !(s[2] >= 0 && s[2] <= kDblMax), done = !zero && !broken && beta <= rtol * bnorm;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        MinresCell c{};
        c.st[0].beta = beta; c.st[0].phibar = beta; c.st[0].cs = -1; c.st[0].gmin = kDblMax;
        c.bnorm = bnorm; c.rnorm = zero ? 0 : beta;
        c.status = broken ? CVR_CG_BREAKDOWN : (zero || done) ? CVR_CG_CONVERGED : CVR_CG_MAX_ITERS;
        c.stop = (zero || broken || done) ? -1 : 0;
        c.zero_x = zero ? 1 : 0;
        *cell = c;
    }
    if (zero || broken || done) return;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T zv[kPack<T>];
        load_pack<T, true>(z, e, (int)cnt, zv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) zv[j] = (T)((double)zv[j] / beta);
        store_pack<T, true>(v, e, (int)cnt, zv);
    }
}

// Step k, behind q = A v: y' = T((double(q) - shift * double(v)) - (beta / oldb) * double(r1)) in r1's place and the partial sums of v . y'.  SHIFT:
// shift != 0, else no shift term; R1: k > 0, else no r1 term (and r1 is not read).
template <typename T, bool SHIFT, bool R1>
__global__ __launch_bounds__(kThreads) void minres_yp_kernel(const T *__restrict__ q, const T *__restrict__ v, T *__restrict__ r1, long long n, double *__restrict__ out,
                                                             const MinresCell *__restrict__ cell, int k, double shift)
{
    __shared__ double sh[1][kWaves];
    if (cell->stop) return;          // (no workgroup of this kernel sets it)
    const double ratio = R1 ? cell->st[k & 1].beta / cell->st[k & 1].oldb : 0.0;
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T qv[kPack<T>], vv[kPack<T>], rv[kPack<T>];
        load_pack<T, true>(q, e, (int)cnt, qv);
        load_pack<T, true>(v, e, (int)cnt, vv);
        if constexpr (R1) load_pack<T, true>(r1, e, (int)cnt, rv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            double t = (double)qv[j];
            if constexpr (SHIFT) t = t - shift * (double)vv[j];
            if constexpr (R1) t = t - ratio * (double)rv[j];
            rv[j] = (T)t;
            if (j < cnt) acc[0] += (double)vv[j] * (double)rv[j];
        }
        store_pack<T, true>(r1, e, (int)cnt, rv);
    }
    store_partials<1>(acc, out, sh);
}

// Step k: alfa = v . y' from its partials; y = T(double(y') - (alfa / beta) * double(r2)) in y's place, z = T(double(minv) * double(y)) (PRE) and the
// partial sums of y . z (z is y without PRE): y is the next step's r2.  AL: minv, the caller's array, is 16-byte aligned.
template <typename T, bool PRE, bool AL>
__global__ __launch_bounds__(kThreads) void minres_r_kernel(T *__restrict__ y, const T *__restrict__ r2, const T *__restrict__ minv, T *__restrict__ z, long long n,
                                                            const double *__restrict__ part, double *__restrict__ out, const MinresCell *__restrict__ cell, int k)
{
    __shared__ double shp[1][kWaves];
    __shared__ double sh[1][kWaves];
    __shared__ int stopped;
    if (threadIdx.x == 0) stopped = cell->stop;          // (no workgroup of this kernel sets it)
    double s[1];
    sum_partials<1>(part, s, shp);
    if (stopped) return;
    const double ratio = s[0] / cell->st[k & 1].beta;
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T yv[kPack<T>], rv[kPack<T>], mv[kPack<T>], zv[kPack<T>];
        load_pack<T, true>(y, e, (int)cnt, yv);
        load_pack<T, true>(r2, e, (int)cnt, rv);
        if constexpr (PRE) load_pack<T, AL>(minv, e, (int)cnt, mv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            yv[j] = (T)((double)yv[j] - ratio * (double)rv[j]);
            zv[j] = PRE ? (T)((double)mv[j] * (double)yv[j]) : yv[j];
            if (j < cnt) acc[0] += (double)yv[j] * (double)zv[j];
        }
        store_pack<T, true>(y, e, (int)cnt, yv);
        if constexpr (PRE) store_pack<T, true>(z, e, (int)cnt, zv);
    }
    store_partials<1>(acc, out, sh);
}

// Step k: alfa and r2 . z from the two sets of partials, the rotation, the breakdown test, w = T(((double(v) - oldeps * double(w1)) - delta * double(w2)) / gamma)
// in w1's place, x = T(double(x) + phi * double(w)), the stop test; not stopped: v = T(double(z) / beta') and the scalars of step k + 1.  z is r2 without a
// preconditioner.  AL: x, the caller's array, is 16-byte aligned.
template <typename T, bool AL>
__global__ __launch_bounds__(kThreads) void minres_x_kernel(T *__restrict__ x, T *__restrict__ v, T *__restrict__ w1, const T *__restrict__ w2, const T *__restrict__ z,
                                                            long long n, const double *__restrict__ part, MinresCell *__restrict__ cell, int k, double rtol)
{
    __shared__ double sh[2][kWaves];
    __shared__ int stopped;
    if (threadIdx.x == 0) stopped = cell->stop != 0 && cell->stop != k + 1;          // (k + 1: workgroup 0 of this launch, just now)
    double s[2];
    sum_partials<2>(part, s, sh);
    if (stopped) return;
    const MinresScalars in = cell->st[k & 1];
    const double alfa = s[0], betan = sqrt(s[1]);
    const double tnorm2 = in.tnorm2 + ((alfa * alfa + in.oldb * in.oldb) + betan * betan);
    const double oldeps = in.epsln, delta = in.cs * in.dbar + in.sn * alfa, gbar = in.sn * in.dbar - in.cs * alfa;
    const double epsln = in.sn * betan, dbar = -in.cs * betan;
    const double gamma = sqrt(gbar * gbar + betan * betan);
    const double cs = gbar / gamma, sn = betan / gamma, phi = cs * in.phibar, phibar = sn * in.phibar;
    const bool   first = blockIdx.x == 0 && threadIdx.x == 0;
    if (!(fabs(alfa) <= kDblMax) || !(s[1] >= 0 && s[1] <= kDblMax) || !usable(gamma) || !(fabs(phi / gamma) <= kDblMax)) {          // found before x is touched
        if (first) { cell->status = CVR_CG_BREAKDOWN; cell->stop = k + 1; }
        return;
    }
    const double gmax = fmax(in.gmax, gamma), gmin = fmin(in.gmin, gamma);
    const bool   done = phibar <= kDblMax && phibar <= rtol * cell->bnorm;
    if (first) {
        cell->rnorm = phibar; cell->anorm = sqrt(tnorm2); cell->acond = gmax / gmin; cell->iters = k + 1;
        if (done) { cell->status = CVR_CG_CONVERGED; cell->stop = k + 1; }
        else cell->st[(k + 1) & 1] = MinresScalars{betan, in.beta, dbar, epsln, phibar, cs, sn, tnorm2, gmax, gmin};
    }
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T xv[kPack<T>], vv[kPack<T>], av[kPack<T>], bv[kPack<T>];
        load_pack<T, AL>(x, e, (int)cnt, xv);
        load_pack<T, true>(v, e, (int)cnt, vv);
        load_pack<T, true>(w1, e, (int)cnt, av);
        load_pack<T, true>(w2, e, (int)cnt, bv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            av[j] = (T)((((double)vv[j] - oldeps * (double)av[j]) - delta * (double)bv[j]) / gamma);
            xv[j] = (T)((double)xv[j] + phi * (double)av[j]);
        }
        store_pack<T, AL>(x, e, (int)cnt, xv);
        store_pack<T, true>(w1, e, (int)cnt, av);
        if (done) continue;          // (the same in every thread)
        load_pack<T, true>(z, e, (int)cnt, vv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) vv[j] = (T)((double)vv[j] / betan);
        store_pack<T, true>(v, e, (int)cnt, vv);
    }
}

}  // namespace
}  // namespace krylov
}  // namespace cvrh
