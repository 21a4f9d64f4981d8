// cvr_lanczos_kernels.h -- the state cell and the vector kernels of the thick-restart Lanczos eigensolver (cvr_lanczos.hip: cvr_eigsh_device).
// What each kernel does: cvr_lanczos.hip's head.  The sums against the basis and the updates by it are cvr_basis_groups.h's, GMRES's own.
#pragma once
#include "cvr_krylov.h"
#include "cvr_basis_groups.h"

namespace cvrh {
namespace krylov {
namespace {

constexpr int kEigMaxM = CVR_EIG_MAX_NCV;
constexpr int kEigInvariant = 100;          // LanCell::status behind a step that closed the space (the host turns it into CVR_EIG_CONVERGED or CVR_EIG_INVARIANT)
constexpr int kInFlight = 8;                // input columns of the restart product whose packets are in flight together

// The state cell: thread 0 of workgroup 0 writes it, and a value a kernel reads is one that a kernel BEFORE it wrote.
struct LanCell {
    int32_t stop;              // != 0: no kernel writes a vector any more
    int32_t status;            // 0, CVR_EIG_BREAKDOWN or kEigInvariant
    int32_t q;                 // columns of the projected matrix so far: j + 1 behind step j
    int32_t reserved;
    double  hj;                // pass 1's h_j of the step under way
    double  alpha[kEigMaxM];   // alpha_j
    double  beta[kEigMaxM + 1];          // beta_(j+1) at [j + 1]
};

// the partial sums of v0 . v0.  AL: v0, the caller's array, is 16-byte aligned.
template <typename T, bool AL>
__global__ __launch_bounds__(kThreads) void lanczos_vv_kernel(const T *__restrict__ v0, long long n, double *__restrict__ out)
{
    __shared__ double sh[1][kWaves];
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T vv[kPack<T>];
        load_pack<T, AL>(v0, e, (int)cnt, vv);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) if (l < cnt) acc[0] += (double)vv[l] * (double)vv[l];
    }
    store_partials<1>(acc, out, sh);
}

// The start, behind lanczos_vv_kernel: s = v0 . v0 (the same in every workgroup); workgroup 0 fills the cell; s finite and > 0: v_0 = T(double(v0) / sqrt(s))
template <typename T, bool AL>
__global__ __launch_bounds__(kThreads) void lanczos_begin_kernel(const T *__restrict__ v0, T *__restrict__ first, long long n, const double *__restrict__ part,
                                                                 LanCell *__restrict__ cell)
{
    __shared__ double sh[1][kWaves];
    double s[1];
    sum_partials<1>(part, s, sh);
    const bool ok = s[0] > 0 && s[0] <= kDblMax;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cell->stop = !ok; cell->status = ok ? 0 : CVR_EIG_BREAKDOWN; cell->q = 0; cell->reserved = 0; cell->hj = 0;
    }
    if (!ok) return;
    const double nrm = sqrt(s[0]);
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T vv[kPack<T>];
        load_pack<T, AL>(v0, e, (int)cnt, vv);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) vv[l] = (T)((double)vv[l] / nrm);
        store_pack<T, true>(first, e, (int)cnt, vv);
    }
}

// set i of `out` = the partial sums of v_i . w for i < ncols, v_i at V + i * stride (gmres_dots_kernel with this solver's cell)
template <typename T>
__global__ __launch_bounds__(kThreads) void lanczos_dots_kernel(const T *__restrict__ V, long long stride, const T *__restrict__ w, long long n, int ncols,
                                                                double *__restrict__ out, const LanCell *__restrict__ cell)
{
    __shared__ double sh[kGroup][kWaves];
    if (cell->stop) return;          // (no workgroup of this kernel sets it)
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

// Step with column j, one Gram-Schmidt pass (gmres_update_kernel's): the coefficients c_i = v_i . w (i = 0..j) from the partials of the dots in front;
// per value t = double(w), t = t - c_0 double(v_0), ..., t = t - c_j double(v_j), w = T(t).  Workgroup 0: pass 1 (!SECOND) keeps h_j, pass 2 stores
// alpha_j = h_j + d_j -- and every workgroup adds the partial sums of w . w of the new w (pass 1: set 0 of out_ww, pass 2: set 1).
template <typename T, bool SECOND>
__global__ __launch_bounds__(kThreads) void lanczos_update_kernel(const T *__restrict__ V, long long stride, T *__restrict__ w, long long n, int j,
                                                                  const double *__restrict__ part, double *__restrict__ out_ww, LanCell *__restrict__ cell)
{
    __shared__ double shs[kEigMaxM][kWaves];
    __shared__ double hs[kEigMaxM];
    __shared__ double shw[1][kWaves];
    __shared__ int    stopped;
    if (threadIdx.x == 0) stopped = cell->stop;
    sum_sets(part, j + 1, hs, shs);
    if (stopped) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if constexpr (!SECOND) cell->hj = hs[j];
        else cell->alpha[j] = cell->hj + hs[j];
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
            if (l < cnt) acc[0] += (double)wv[l] * (double)wv[l];
        }
        store_pack<T, true>(w, e, (int)cnt, wv);
    }
    store_partials<1>(acc, out_ww + (SECOND ? kBlocks : 0), shw);
}

// Step with column j, behind the second pass: ww1 = w . w between the passes, ww = w . w of the new w, beta_(j+1) = sqrt(ww) (the same in every
// workgroup; workgroup 0 records it); a sum or alpha_j not finite: breakdown; ww <= ww1 / 4 (beta == 0 included): the space is closed with j + 1
// columns; otherwise v_(j+1) = T(double(w) / beta_(j+1)).
template <typename T>
__global__ __launch_bounds__(kThreads) void lanczos_finish_kernel(const T *__restrict__ w, T *__restrict__ vnext, long long n, const double *__restrict__ part_ww,
                                                                  LanCell *__restrict__ cell, int j)
{
    __shared__ double sh[2][kWaves];
    __shared__ int    stopped;
    if (threadIdx.x == 0) stopped = cell->stop;
    double s[2];
    sum_partials<2>(part_ww, s, sh);
    if (stopped) return;
    const bool   first = blockIdx.x == 0 && threadIdx.x == 0;
    const double alpha = cell->alpha[j], beta = sqrt(s[1]);
    const bool   closed = s[1] <= 0.25 * s[0];
    if (!(fabs(s[0]) <= kDblMax) || !(fabs(s[1]) <= kDblMax) || !(fabs(alpha) <= kDblMax)) {
        if (first) { cell->status = CVR_EIG_BREAKDOWN; cell->stop = 1; }
        return;
    }
    if (first) {
        cell->beta[j + 1] = beta;
        cell->q = j + 1;
        if (closed) { cell->status = kEigInvariant; cell->stop = 1; }
    }
    if (closed) return;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T wv[kPack<T>];
        load_pack<T, true>(w, e, (int)cnt, wv);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) wv[l] = (T)((double)wv[l] / beta);
        store_pack<T, true>(vnext, e, (int)cnt, wv);
    }
}

// acc[c][.] = acc[c][.] + S[l][c] * double(v_l) for the C input columns l at V, in that order, their packets loaded together; ss: row l of the group's
// coefficients at ss + l * kEigMaxM (LDS)
template <typename T, int G, int C>
__device__ __forceinline__ void restart_accumulate(const T *__restrict__ V, long long stride, long long e, int cnt, const double *__restrict__ ss,
                                                   double (&acc)[G][kPack<T>])
{
    T vv[C][kPack<T>];
#pragma unroll
    for (int l = 0; l < C; l++) load_pack<T, true>(V + l * stride, e, cnt, vv[l]);
#pragma unroll
    for (int l = 0; l < C; l++)
#pragma unroll
        for (int c = 0; c < G; c++) {
            const double sc = ss[l * kEigMaxM + c];
#pragma unroll
            for (int p = 0; p < kPack<T>; p++) acc[c][p] = acc[c][p] + sc * (double)vv[l][p];
        }
}

// G output columns at out (column c at out + c * ldo) from the q input columns at V: per value u = +0, u = u + S[l][c] * double(v_l) for l ascending,
// T(u).  A thread owns its packets; the input columns stream in groups of kInFlight (the rest in 4, 2 and 1).  AL: the output columns are 16-byte aligned.
template <typename T, int G, bool AL>
__device__ __forceinline__ void restart_group(const T *__restrict__ V, long long stride, int q, const double *__restrict__ ss, T *__restrict__ out, long long ldo,
                                              long long n)
{
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        double acc[G][kPack<T>];
#pragma unroll
        for (int c = 0; c < G; c++)
#pragma unroll
            for (int p = 0; p < kPack<T>; p++) acc[c][p] = 0;
        int l = 0;
        for (; l + kInFlight <= q; l += kInFlight) restart_accumulate<T, G, kInFlight>(V + l * stride, stride, e, (int)cnt, ss + l * kEigMaxM, acc);
        if (q - l >= 4) { restart_accumulate<T, G, 4>(V + l * stride, stride, e, (int)cnt, ss + l * kEigMaxM, acc); l += 4; }
        if (q - l >= 2) { restart_accumulate<T, G, 2>(V + l * stride, stride, e, (int)cnt, ss + l * kEigMaxM, acc); l += 2; }
        if (q - l >= 1) restart_accumulate<T, G, 1>(V + l * stride, stride, e, (int)cnt, ss + l * kEigMaxM, acc);
#pragma unroll
        for (int c = 0; c < G; c++) {
            T ov[kPack<T>];
#pragma unroll
            for (int p = 0; p < kPack<T>; p++) ov[p] = (T)acc[c][p];
            store_pack<T, AL>(out + c * ldo, e, (int)cnt, ov);
        }
    }
}

// The restart product: out[:, 0..nout-1] = V[:, 0..q-1] . S, S (q x nout, row l at S + l * kEigMaxM, fp64) read from LDS, loaded once per workgroup; the
// output columns in compile-time groups of up to kGroup.  out never overlaps V (another workgroup may still be reading a column).  Enqueued behind a
// read-back only, so it has no stop to look at.
template <typename T, bool AL>
__global__ __launch_bounds__(kThreads) void lanczos_restart_kernel(const T *__restrict__ V, long long stride, int q, const double *__restrict__ S, int nout,
                                                                   T *__restrict__ out, long long ldo, long long n)
{
    __shared__ double ss[kEigMaxM * kEigMaxM];
    for (int i = threadIdx.x; i < q * kEigMaxM; i += kThreads) ss[i] = (i % kEigMaxM) < nout ? S[i] : 0.0;
    __syncthreads();
    int c0 = 0;
    for (; c0 + kGroup <= nout; c0 += kGroup) restart_group<T, kGroup, AL>(V, stride, q, ss + c0, out + c0 * ldo, ldo, n);
    T            *outr = out + c0 * ldo;
    const double *sr = ss + c0;
    switch (nout - c0) {
    case 1: restart_group<T, 1, AL>(V, stride, q, sr, outr, ldo, n); break;
    case 2: restart_group<T, 2, AL>(V, stride, q, sr, outr, ldo, n); break;
    case 3: restart_group<T, 3, AL>(V, stride, q, sr, outr, ldo, n); break;
    case 4: restart_group<T, 4, AL>(V, stride, q, sr, outr, ldo, n); break;
    case 5: restart_group<T, 5, AL>(V, stride, q, sr, outr, ldo, n); break;
    case 6: restart_group<T, 6, AL>(V, stride, q, sr, outr, ldo, n); break;
    case 7: restart_group<T, 7, AL>(V, stride, q, sr, outr, ldo, n); break;
    default: break;
    }
}

}  // namespace
}  // namespace krylov
}  // namespace cvrh
