// cvr_lsqr_kernels.h -- the state cell and the vector kernels of LSQR (cvr_lsqr.hip: cvr_lsqr_device).  What each kernel does: cvr_lsqr.hip's head.
#pragma once
#include "cvr_krylov.h"

namespace cvrh {
namespace krylov {
namespace {

// The scalars a step hands to the next one.  lsqr_x_kernel of step k reads st[k & 1] in every workgroup while thread 0 of workgroup 0 writes
// st[(k + 1) & 1], which lsqr_u_kernel and lsqr_x_kernel of step k + 1 read: no kernel reads a slot that a workgroup of the same launch writes.
struct LsqrScalars {
    double alpha, beta;          // of the bidiagonalisation: ||v^|| and ||u^|| of the last step
    double rhobar, phibar;
    double anorm2, psi2;         // the running sums of alpha^2 + beta^2 + damp^2 and of psi^2
};

// The state cell.  Written by thread 0 of workgroup 0 only.  `stop` is the one word a workgroup may read while another one of the same launch
// writes it: lsqr_x_kernel of step k sets it to k + 1 and does not take that value for a stop (every workgroup still applies its share of the
// step's update of x, or, at a breakdown, comes to the same decision from the same sums and returns); the start sets it to -1.
struct LsqrCell {
    LsqrScalars st[2];
    double  bnorm, rnorm;        // sqrt(b . b); the residual estimate of the last iterate
    double  arnorm, anorm;       // cvr_lsqr_info's
    int32_t stop;                // != 0: no kernel writes a vector any more (k + 1: found by step k; -1: by the start)
    int32_t stop_test;           // cvr_lsqr_info's
    int32_t status;              // CVR_CG_*
    int32_t iters;               // steps applied to x
    int32_t zero_x;              // b == 0: the solution is x = 0 (the host clears it)
    int32_t pad;
};

// The start, over m: the partial sums of b . b (set 0) and u^ . u^ (set 1); u^ holds b - A x0 (the scaled product).  AL: b, the caller's array,
// is 16-byte aligned.
template <typename T, bool AL>
__global__ __launch_bounds__(kThreads) void lsqr_init_kernel(const T *__restrict__ b, const T *__restrict__ u, long long n, double *__restrict__ out)
{
    __shared__ double sh[2][kWaves];
    double acc[2] = {0, 0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T bv[kPack<T>], uv[kPack<T>];
        load_pack<T, AL>(b, e, (int)cnt, bv);
        load_pack<T, true>(u, e, (int)cnt, uv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++)
            if (j < cnt) {
                acc[0] += (double)bv[j] * (double)bv[j];
                acc[1] += (double)uv[j] * (double)uv[j];
            }
    }
    store_partials<2>(acc, out, sh);
}

// The start, over n, behind p = A^T u^: bnorm and beta from the partials into a fresh cell, with the stops that need no alpha (b == 0; beta not
// finite; beta <= rtol bnorm); else v^ = T(double(p) / beta) into v and the partial sums of v^ . v^.
template <typename T>
__global__ __launch_bounds__(kThreads) void lsqr_v0_kernel(const T *__restrict__ p, T *__restrict__ v, long long n, const double *__restrict__ part, double *__restrict__ out,
                                                           LsqrCell *__restrict__ cell, double rtol)
{
    __shared__ double shp[2][kWaves];
    __shared__ double sh[1][kWaves];
    double s[2];
    sum_partials<2>(part, s, shp);
    const double bnorm = sqrt(s[0]), beta = sqrt(s[1]);
    const bool   zero = s[0] == 0, broken = !zero && !(fabs(beta) <= kDblMax), done = !zero && !broken && beta <= rtol * bnorm;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        LsqrCell c{};
        c.st[0].beta = beta; c.st[0].phibar = beta;
        c.bnorm = bnorm; c.rnorm = zero ? 0 : beta;
        c.status = broken ? CVR_CG_BREAKDOWN : (zero || done) ? CVR_CG_CONVERGED : CVR_CG_MAX_ITERS;
        c.stop = (zero || broken || done) ? -1 : 0;
        c.stop_test = done ? 1 : 0;
        c.zero_x = zero ? 1 : 0;
        *cell = c;
    }
    if (zero || broken || done) return;
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T pv[kPack<T>], vv[kPack<T>];
        load_pack<T, true>(p, e, (int)cnt, pv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            vv[j] = (T)((double)pv[j] / beta);
            if (j < cnt) acc[0] += (double)vv[j] * (double)vv[j];
        }
        store_pack<T, true>(v, e, (int)cnt, vv);
    }
    store_partials<1>(acc, out, sh);
}

// The start, over n: alpha = sqrt(v^ . v^) from its partials; alpha not finite: breakdown; alpha == 0: converged by test 2; else v = T(double(v^) / alpha),
// w = v and the scalars of step 0.
template <typename T>
__global__ __launch_bounds__(kThreads) void lsqr_start_kernel(T *__restrict__ v, T *__restrict__ w, long long n, const double *__restrict__ part, LsqrCell *__restrict__ cell)
{
    __shared__ double sh[1][kWaves];
    __shared__ int stopped;
    if (threadIdx.x == 0) stopped = cell->stop;          // (lsqr_v0_kernel's, or the one workgroup 0 records below: every workgroup comes to that one itself)
    double s[1];
    sum_partials<1>(part, s, sh);
    if (stopped) return;
    const double alpha = sqrt(s[0]), beta = cell->st[0].beta;
    const bool   broken = !(fabs(alpha) <= kDblMax), done = !broken && alpha == 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cell->st[0].alpha = alpha; cell->st[0].rhobar = alpha;
        cell->arnorm = alpha * beta;
        if (broken) { cell->status = CVR_CG_BREAKDOWN; cell->stop = -1; }
        if (done) { cell->status = CVR_CG_CONVERGED; cell->stop_test = 2; cell->stop = -1; }
    }
    if (broken || done) return;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T vv[kPack<T>];
        load_pack<T, true>(v, e, (int)cnt, vv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) vv[j] = (T)((double)vv[j] / alpha);
        store_pack<T, true>(v, e, (int)cnt, vv);
        store_pack<T, true>(w, e, (int)cnt, vv);
    }
}

// Step k, over m, behind q = A v: u^ = T(double(q) - (alpha / beta) double(u^)) and the partial sums of u^ . u^.
template <typename T>
__global__ __launch_bounds__(kThreads) void lsqr_u_kernel(const T *__restrict__ q, T *__restrict__ u, long long n, double *__restrict__ out, const LsqrCell *__restrict__ cell, int k)
{
    __shared__ double sh[1][kWaves];
    if (cell->stop) return;          // (no workgroup of this kernel sets it)
    const double ratio = cell->st[k & 1].alpha / cell->st[k & 1].beta;
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T qv[kPack<T>], uv[kPack<T>];
        load_pack<T, true>(q, e, (int)cnt, qv);
        load_pack<T, true>(u, e, (int)cnt, uv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            uv[j] = (T)((double)qv[j] - ratio * (double)uv[j]);
            if (j < cnt) acc[0] += (double)uv[j] * (double)uv[j];
        }
        store_pack<T, true>(u, e, (int)cnt, uv);
    }
    store_partials<1>(acc, out, sh);
}

// Step k, over n, behind p = A^T u^: beta' = sqrt(u^ . u^) from its partials; zero or not finite: nothing written (lsqr_x_kernel reads the same
// sum); else v^ = T(double(p) / beta' - beta' double(v)) in v's place and the partial sums of v^ . v^.
template <typename T>
__global__ __launch_bounds__(kThreads) void lsqr_v_kernel(const T *__restrict__ p, T *__restrict__ v, long long n, const double *__restrict__ part, double *__restrict__ out,
                                                          const LsqrCell *__restrict__ cell)
{
    __shared__ double shp[1][kWaves];
    __shared__ double sh[1][kWaves];
    __shared__ int stopped;
    if (threadIdx.x == 0) stopped = cell->stop;
    double s[1];
    sum_partials<1>(part, s, shp);
    if (stopped) return;
    const double beta = sqrt(s[0]);
    if (!usable(beta)) return;
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T pv[kPack<T>], vv[kPack<T>];
        load_pack<T, true>(p, e, (int)cnt, pv);
        load_pack<T, true>(v, e, (int)cnt, vv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            vv[j] = (T)((double)pv[j] / beta - beta * (double)vv[j]);
            if (j < cnt) acc[0] += (double)vv[j] * (double)vv[j];
        }
        store_pack<T, true>(v, e, (int)cnt, vv);
    }
    store_partials<1>(acc, out, sh);
}

// Step k, over n: beta' and alpha' from the two sets of partials (u^ . u^, v^ . v^), the rotations, the breakdown test, x = T(double(x) + (phi / rho)
// double(w)), the norms and the stop tests; not stopped: v = T(double(v^) / alpha'), w = T(double(v) - (theta / rho) double(w)) and the scalars of
// step k + 1.  AL: x, the caller's array, is 16-byte aligned.
template <typename T, bool AL>
__global__ __launch_bounds__(kThreads) void lsqr_x_kernel(T *__restrict__ x, T *__restrict__ v, T *__restrict__ w, long long n, const double *__restrict__ part,
                                                          LsqrCell *__restrict__ cell, int k, double damp, double rtol)
{
    __shared__ double sh[2][kWaves];
    __shared__ int stopped;
    if (threadIdx.x == 0) stopped = cell->stop != 0 && cell->stop != k + 1;          // (k + 1: workgroup 0 of this launch, just now)
    double s[2];
    sum_partials<2>(part, s, sh);
    if (stopped) return;
    const LsqrScalars in = cell->st[k & 1];
    const double betan = sqrt(s[0]), alphan = betan == 0 ? 0.0 : sqrt(s[1]);
    const double anorm2 = in.anorm2 + ((in.alpha * in.alpha + betan * betan) + damp * damp);
    double rhobar1 = in.rhobar, phibar = in.phibar, psi = 0;
    if (damp > 0) {
        rhobar1 = sqrt(in.rhobar * in.rhobar + damp * damp);
        psi = (damp / rhobar1) * phibar;
        phibar = (in.rhobar / rhobar1) * phibar;
    }
    const double rho = sqrt(rhobar1 * rhobar1 + betan * betan);
    const double c = rhobar1 / rho, sn = betan / rho;
    const double theta = sn * alphan, rhobarn = -c * alphan, phi = c * phibar, phibarn = sn * phibar;
    const double t1 = phi / rho, t2 = theta / rho;
    const bool   first = blockIdx.x == 0 && threadIdx.x == 0;
    if (!(fabs(betan) <= kDblMax) || !(fabs(alphan) <= kDblMax) || !usable(rho) || !(fabs(t1) <= kDblMax)) {          // found before x is touched
        if (first) { cell->status = CVR_CG_BREAKDOWN; cell->stop = k + 1; }
        return;
    }
    const double psi2 = in.psi2 + psi * psi;
    const double rnorm = sqrt(phibarn * phibarn + psi2), arnorm = alphan * fabs(sn * phi), anorm = sqrt(anorm2);
    const bool   finite = rnorm <= kDblMax && arnorm <= kDblMax && anorm <= kDblMax;
    const int    test = !finite ? 0 : rnorm <= rtol * cell->bnorm ? 1 : arnorm <= (rtol * anorm) * rnorm ? 2 : 0;
    if (first) {
        cell->rnorm = rnorm; cell->arnorm = arnorm; cell->anorm = anorm; cell->iters = k + 1;
        if (test) { cell->status = CVR_CG_CONVERGED; cell->stop_test = test; cell->stop = k + 1; }
        else cell->st[(k + 1) & 1] = LsqrScalars{alphan, betan, rhobarn, phibarn, anorm2, psi2};
    }
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T xv[kPack<T>], vv[kPack<T>], wv[kPack<T>];
        load_pack<T, AL>(x, e, (int)cnt, xv);
        load_pack<T, true>(w, e, (int)cnt, wv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) xv[j] = (T)((double)xv[j] + t1 * (double)wv[j]);
        store_pack<T, AL>(x, e, (int)cnt, xv);
        if (test) continue;          // (the same in every thread)
        load_pack<T, true>(v, e, (int)cnt, vv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) {
            vv[j] = (T)((double)vv[j] / alphan);
            wv[j] = (T)((double)vv[j] - t2 * (double)wv[j]);
        }
        store_pack<T, true>(v, e, (int)cnt, vv);
        store_pack<T, true>(w, e, (int)cnt, wv);
    }
}

}  // namespace
}  // namespace krylov
}  // namespace cvrh
