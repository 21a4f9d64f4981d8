// cvr_gmres_kernels.h -- the state cell, the vector kernels and the column-group macro of GMRES(m) (cvr_gmres.hip: cvr_gmres_device,
// cvr_pgmres_device; cvr_fgmres.hip: cvr_fgmres_device).  What each kernel does: cvr_gmres.hip's head.
#pragma once
#include "cvr_krylov.h"
#include "cvr_basis_groups.h"

namespace cvrh {
namespace krylov {
namespace {

constexpr int    kMaxM = CVR_GMRES_MAX_RESTART;

// what the host reads back
struct GmresHead {
    double  bb, bnorm;         // b . b and its root
    double  rnorm;             // residual_norm: the true ||r|| at a cycle's start, the estimate |g_(j+1)| behind a step, |g_j| at a breakdown
    double  hrot;              // H_j of the step under way behind the earlier rotations (the second gmres_update_kernel writes it, gmres_finish_kernel reads it)
    int32_t stop;              // != 0: no kernel writes a vector any more (gmres_x_kernel apart: see owed)
    int32_t status;            // CVR_CG_*
    int32_t iters;             // steps counted
    int32_t zero_x;            // b == 0: the solution is x = 0 (the host clears it)
    int32_t owed;              // columns of the current cycle that x is still owed (y holds their coefficients); 0: none
    int32_t owed_at;           // k + 1 of the step k whose gmres_finish_kernel set `owed`: a gmres_x_kernel acts when its range of steps (lo, hi] holds it, so
                               // nobody has to clear `owed` in the kernel that reads it
};

// The state cell.  g[i] is final (behind rotation i), gbar[i] the running value in front of it: rotation j reads gbar[j] and writes g[j] and gbar[j + 1], never
// what another workgroup of the same kernel may be reading.  R is column-major: R_(i,l) at R[l * kMaxM + i].
struct GmresCell {
    GmresHead hd;
    double    g[kMaxM], gbar[kMaxM + 1], cs[kMaxM], sn[kMaxM];
    double    h[kMaxM];          // pass 1's h_i of the step under way
    double    y[kMaxM];
    double    R[kMaxM * kMaxM];
};

// set i of `out` = the partial sums of v_i . w for i < ncols, v_i at V + i * stride
template <typename T>
__global__ __launch_bounds__(kThreads) void gmres_dots_kernel(const T *__restrict__ V, long long stride, const T *__restrict__ w, long long n, int ncols,
                                                              double *__restrict__ out, const GmresCell *__restrict__ cell)
{
    __shared__ double sh[kGroup][kWaves];
    if (cell->hd.stop) return;          // (no workgroup of this kernel sets it)
    int c0 = 0;
    for (; c0 + kGroup <= ncols; c0 += kGroup) {
        dot_group<T, kGroup>(V + c0 * stride, stride, w, n, out + (size_t)c0 * kBlocks, sh);
        __syncthreads();          // thread 0 has read sh before the next group writes it
    }
    const T *Vr = V + c0 * stride;
    double  *outr = out + (size_t)c0 * kBlocks;
    switch (ncols - c0) {
    case 1: dot_group<T, 1>(Vr, stride, w, n, outr, sh); break;
    case 2: dot_group<T, 2>(Vr, stride, w, n, outr, sh); break;
    case 3: dot_group<T, 3>(Vr, stride, w, n, outr, sh); break;
    case 4: dot_group<T, 4>(Vr, stride, w, n, outr, sh); break;
    case 5: dot_group<T, 5>(Vr, stride, w, n, outr, sh); break;
    case 6: dot_group<T, 6>(Vr, stride, w, n, outr, sh); break;
    case 7: dot_group<T, 7>(Vr, stride, w, n, outr, sh); break;
    default: break;
    }
}

// Step with column j, one Gram-Schmidt pass: the coefficients c_i = v_i . w (i = 0..j) from the partials of the dots in front; per value
// t = double(w), t = t - c_0 double(v_0), ..., t = t - c_j double(v_j), w = T(t).  Workgroup 0 keeps the coefficients: pass 1 (!SECOND) stores h_i; pass 2
// forms H_i = h_i + d_i, applies the rotations 0 .. j - 1 to the column, stores R_(i,j) for i < j and the rotated H_j (hrot) -- and every workgroup adds the
// partial sums of w . w of the new w.
template <typename T, bool SECOND>
__global__ __launch_bounds__(kThreads) void gmres_update_kernel(const T *__restrict__ V, long long stride, T *__restrict__ w, long long n, int j,
                                                                const double *__restrict__ part, double *__restrict__ out_ww, GmresCell *__restrict__ cell)
{
    __shared__ double shs[kMaxM][kWaves];
    __shared__ double hs[kMaxM];
    __shared__ double shw[1][kWaves];
    __shared__ int    stopped;
    if (threadIdx.x == 0) stopped = cell->hd.stop;
    sum_sets(part, j + 1, hs, shs);
    if (stopped) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if constexpr (!SECOND) {
            for (int i = 0; i <= j; i++) cell->h[i] = hs[i];
        } else {
            double cur = cell->h[0] + hs[0];          // H_i in front of rotation i
            for (int i = 0; i < j; i++) {
                const double nxt = cell->h[i + 1] + hs[i + 1], cs = cell->cs[i], sn = cell->sn[i];
                const double t = cs * cur + sn * nxt;
                const double u = cs * nxt - sn * cur;
                cell->R[j * kMaxM + i] = t;
                cur = u;
            }
            cell->hd.hrot = cur;
        }
    }
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T      wv[kPack<T>];
        double t[kPack<T>];
        load_pack<T, true>(w, e, (int)cnt, wv);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) t[l] = (double)wv[l];
        CVR_GMRES_GROUPS(sub_group, j + 1, hs, t);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) {
            wv[l] = (T)t[l];
            if constexpr (SECOND) if (l < cnt) acc[0] += (double)wv[l] * (double)wv[l];
        }
        store_pack<T, true>(w, e, (int)cnt, wv);
    }
    if constexpr (SECOND) store_partials<1>(acc, out_ww, shw);
}

// y of the q columns of the cycle by back substitution, descending, each row's terms ascending (one thread)
__device__ void solve_y(GmresCell *__restrict__ cell, int q)
{
    for (int i = q - 1; i >= 0; i--) {
        double t = cell->g[i];
        for (int l = i + 1; l < q; l++) t = t - cell->R[l * kMaxM + i] * cell->y[l];
        cell->y[i] = t / cell->R[i * kMaxM + i];
    }
}

// Step k with column j, behind the second pass: H_(j+1) = sqrt(w . w), rho, the rotation and the stop test (the same decision in every workgroup, from the
// same sums; workgroup 0 records it); a cycle that goes on gets v_(j+1) = T(double(w) / H_(j+1)) and, with a preconditioner, z_(j+1).  AL: minv is aligned.
template <typename T, bool PRE, bool AL>
__global__ __launch_bounds__(kThreads) void gmres_finish_kernel(const T *__restrict__ w, const T *__restrict__ minv, T *__restrict__ vnext, T *__restrict__ z,
                                                                long long n, const double *__restrict__ part_ww, GmresCell *__restrict__ cell, int j, int k, int m,
                                                                int max_iters, double rtol)
{
    __shared__ double sh[1][kWaves];
    __shared__ int    stopped;
    if (threadIdx.x == 0) stopped = cell->hd.stop;
    double s[1];
    sum_partials<1>(part_ww, s, sh);
    if (stopped) return;
    const bool   first = blockIdx.x == 0 && threadIdx.x == 0;
    const double hn = sqrt(s[0]), hj = cell->hd.hrot, gj = cell->gbar[j];
    const double rho = sqrt(hj * hj + hn * hn);
    if (!usable(rho)) {          // found before the step is counted: x from the j columns before it
        if (first) {
            cell->hd.rnorm = fabs(gj);
            cell->hd.status = CVR_CG_BREAKDOWN;
            solve_y(cell, j);
            cell->hd.owed = j; cell->hd.owed_at = k + 1;
            cell->hd.stop = 1;
        }
        return;
    }
    const double cs = hj / rho, sn = hn / rho;
    const double gn = -(sn * gj), est = fabs(gn);
    const bool   done = est <= rtol * cell->hd.bnorm && est <= kDblMax;
    const bool   last = k + 1 == max_iters, full = j + 1 == m;
    if (first) {
        cell->cs[j] = cs; cell->sn[j] = sn;
        cell->R[j * kMaxM + j] = rho;
        cell->g[j] = cs * gj; cell->gbar[j + 1] = gn;
        cell->hd.iters = k + 1; cell->hd.rnorm = est;
        if (done || last || full) {
            solve_y(cell, j + 1);
            cell->hd.owed = j + 1; cell->hd.owed_at = k + 1;
        }
        if (done) { cell->hd.status = CVR_CG_CONVERGED; cell->hd.stop = 1; }
    }
    if (done || last || full) return;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T wv[kPack<T>], mv[kPack<T>], zv[kPack<T>];
        load_pack<T, true>(w, e, (int)cnt, wv);
        if constexpr (PRE) load_pack<T, AL>(minv, e, (int)cnt, mv);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) {
            wv[l] = (T)((double)wv[l] / hn);
            if constexpr (PRE) zv[l] = (T)((double)mv[l] * (double)wv[l]);
        }
        store_pack<T, true>(vnext, e, (int)cnt, wv);
        if constexpr (PRE) store_pack<T, true>(z, e, (int)cnt, zv);
    }
}

// A cycle's start: r holds b - A x (the scaled product).  The partial sums of r . r (set 0) and, at the call's start (FIRST), of b . b (set 1).
// AL: b, the caller's array, is 16-byte aligned.
template <typename T, bool FIRST, bool AL>
__global__ __launch_bounds__(kThreads) void gmres_rr_kernel(const T *__restrict__ r, const T *__restrict__ b, long long n, double *__restrict__ out,
                                                            const GmresCell *__restrict__ cell)
{
    __shared__ double sh[2][kWaves];
    if constexpr (!FIRST) if (cell->hd.stop) return;
    double acc[2] = {0, 0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T rv[kPack<T>], bv[kPack<T>];
        load_pack<T, true>(r, e, (int)cnt, rv);
        if constexpr (FIRST) load_pack<T, AL>(b, e, (int)cnt, bv);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++)
            if (l < cnt) {
                acc[0] += (double)rv[l] * (double)rv[l];
                if constexpr (FIRST) acc[1] += (double)bv[l] * (double)bv[l];
            }
    }
    store_partials<2>(acc, out, sh);          // (a later cycle's set 1 is +0 and nobody reads it)
}

// A cycle's start, behind gmres_rr_kernel: the stop test on the true residual (`first`: the call's start, which fills the cell); a cycle that starts gets
// g_0 = ||r||, v_0 = T(double(r) / ||r||) and, with a preconditioner, z_0.  AL: minv is aligned.
template <typename T, bool PRE, bool AL>
__global__ __launch_bounds__(kThreads) void gmres_begin_kernel(const T *__restrict__ r, const T *__restrict__ minv, T *__restrict__ v0, T *__restrict__ z, long long n,
                                                               const double *__restrict__ part, double rtol, int first, GmresCell *__restrict__ cell)
{
    __shared__ double sh[2][kWaves];
    __shared__ int    stopped;
    if (threadIdx.x == 0) stopped = first ? 0 : cell->hd.stop;
    double s[2];
    sum_partials<2>(part, s, sh);
    if (stopped) return;
    const double bb = first ? s[1] : cell->hd.bb, bnorm = first ? sqrt(s[1]) : cell->hd.bnorm;
    const double rnorm = sqrt(s[0]);
    const bool   zero = first && bb == 0;
    const bool   done = !zero && rnorm <= rtol * bnorm && rnorm <= kDblMax;
    const bool   broken = !zero && !done && !(rnorm <= kDblMax);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (first) {
            GmresHead hd;
            hd.bb = bb; hd.bnorm = bnorm; hd.rnorm = zero ? 0 : rnorm; hd.hrot = 0;
            hd.stop = zero || done || broken; hd.status = broken ? CVR_CG_BREAKDOWN : zero || done ? CVR_CG_CONVERGED : CVR_CG_MAX_ITERS;
            hd.iters = 0; hd.zero_x = zero; hd.owed = 0; hd.owed_at = 0;
            cell->hd = hd;
        } else {
            cell->hd.rnorm = rnorm;
            cell->hd.owed = 0;
            if (done) { cell->hd.status = CVR_CG_CONVERGED; cell->hd.stop = 1; }
            if (broken) { cell->hd.status = CVR_CG_BREAKDOWN; cell->hd.stop = 1; }
        }
        cell->gbar[0] = rnorm;
    }
    if (zero || done || broken) return;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T rv[kPack<T>], mv[kPack<T>], zv[kPack<T>];
        load_pack<T, true>(r, e, (int)cnt, rv);
        if constexpr (PRE) load_pack<T, AL>(minv, e, (int)cnt, mv);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) {
            rv[l] = (T)((double)rv[l] / rnorm);
            if constexpr (PRE) zv[l] = (T)((double)mv[l] * (double)rv[l]);
        }
        store_pack<T, true>(v0, e, (int)cnt, rv);
        if constexpr (PRE) store_pack<T, true>(z, e, (int)cnt, zv);
    }
}

// x from the columns the cell says are owed, when the step that said so lies in (lo, hi]: per value u = +0, u = u + y_i double(v_i) for i ascending,
// x = T(double(x) + double(minv) * u), or T(double(x) + u) without a preconditioner.  Reads the cell only.  AL: x and minv are aligned.
template <typename T, bool PRE, bool AL>
__global__ __launch_bounds__(kThreads) void gmres_x_kernel(T *__restrict__ x, const T *__restrict__ minv, const T *__restrict__ V, long long stride, long long n,
                                                           const GmresCell *__restrict__ cell, int lo, int hi)
{
    __shared__ double ys[kMaxM];
    const int q = cell->hd.owed, at = cell->hd.owed_at;
    if (q <= 0 || at <= lo || at > hi) return;
    for (int i = threadIdx.x; i < q; i += kThreads) ys[i] = cell->y[i];
    __syncthreads();
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T      xv[kPack<T>], mv[kPack<T>];
        double u[kPack<T>];
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) u[l] = 0;
        load_pack<T, AL>(x, e, (int)cnt, xv);
        if constexpr (PRE) load_pack<T, AL>(minv, e, (int)cnt, mv);
        CVR_GMRES_GROUPS(add_group, q, ys, u);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) {
            if constexpr (PRE) xv[l] = (T)((double)xv[l] + (double)mv[l] * u[l]);
            else xv[l] = (T)((double)xv[l] + u[l]);
        }
        store_pack<T, AL>(x, e, (int)cnt, xv);
    }
}

}  // namespace
}  // namespace krylov
}  // namespace cvrh
