// cvr_svds_kernels.h -- the state cell and the half-step kernels of the thick-restart Golub-Kahan-Lanczos solver (cvr_svds.hip: cvr_svds_device).
// What each kernel does: cvr_svds.hip's head.  The sums against a basis and the updates by it are cvr_basis_groups.h's, GMRES's and Lanczos's own;
// the restart product is cvr_lanczos_kernels.h's lanczos_restart_kernel as it is.  A half step is Lanczos's step but for three things: the basis it
// orthogonalises against (U over nrows values in the left half, V over ncols values in the right one) is not the basis the product's input came
// from, the left half of step 0 has no column to work against, and what enters the cell is the norm of the new vector, not a coefficient.
#pragma once
#include "cvr_krylov.h"
#include "cvr_basis_groups.h"

namespace cvrh {
namespace krylov {
namespace {

constexpr int kSvdMaxM = CVR_SVD_MAX_NCV;
constexpr int kSvdClosedLeft = 100, kSvdClosedRight = 101;          // SvdCell::status behind a half step that closed its space

// The state cell: thread 0 of workgroup 0 writes it, and a value a kernel reads is one that a kernel BEFORE it wrote.
struct SvdCell {
    int32_t stop;              // != 0: no kernel writes a vector any more
    int32_t status;            // 0, CVR_EIG_BREAKDOWN, kSvdClosedLeft or kSvdClosedRight
    int32_t j;                 // the step whose half closed the space
    int32_t reserved;
    double  alpha[kSvdMaxM];   // alpha_j
    double  beta[kSvdMaxM + 1];          // beta_(j+1) at [j + 1]
};

// The start, behind the partial sums of v0 . v0: s = v0 . v0 (the same in every workgroup); workgroup 0 fills the cell; s finite and > 0:
// v_0 = T(double(v0) / sqrt(s)).  AL: v0, the caller's array, is 16-byte aligned.
template <typename T, bool AL>
__global__ __launch_bounds__(kThreads) void svds_begin_kernel(const T *__restrict__ v0, T *__restrict__ first, long long n, const double *__restrict__ part,
                                                              SvdCell *__restrict__ cell)
{
    __shared__ double sh[1][kWaves];
    double s[1];
    sum_partials<1>(part, s, sh);
    const bool ok = s[0] > 0 && s[0] <= kDblMax;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cell->stop = !ok; cell->status = ok ? 0 : CVR_EIG_BREAKDOWN; cell->j = 0; cell->reserved = 0;
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

// set i of `out` = the partial sums of b_i . w for i < ncols (ncols >= 1), b_i at B + i * stride, over n values
template <typename T>
__global__ __launch_bounds__(kThreads) void svds_dots_kernel(const T *__restrict__ B, long long stride, const T *__restrict__ w, long long n, int ncols,
                                                             double *__restrict__ out, const SvdCell *__restrict__ cell)
{
    __shared__ double sh[kGroup][kWaves];
    if (cell->stop) return;          // (no workgroup of this kernel sets it)
    int c0 = 0;
    for (; c0 + kGroup <= ncols; c0 += kGroup) {
        dot_group<T, kGroup>(B + c0 * stride, stride, w, n, out + (size_t)c0 * kBlocks, sh);
        __syncthreads();          // thread 0 has read sh before the next group writes it
    }
    const T *Br = B + c0 * stride;
    double  *outr = out + (size_t)c0 * kBlocks;
    switch (ncols - c0) {
    case 1: dot_group<T, 1>(Br, stride, w, n, outr, sh); break;
    case 2: dot_group<T, 2>(Br, stride, w, n, outr, sh); break;
    case 3: dot_group<T, 3>(Br, stride, w, n, outr, sh); break;
    case 4: dot_group<T, 4>(Br, stride, w, n, outr, sh); break;
    case 5: dot_group<T, 5>(Br, stride, w, n, outr, sh); break;
    case 6: dot_group<T, 6>(Br, stride, w, n, outr, sh); break;
    case 7: dot_group<T, 7>(Br, stride, w, n, outr, sh); break;
    default: break;
    }
}

// One Gram-Schmidt pass of a half step against ncols columns (0 in the left half of step 0: nothing is summed or subtracted): the coefficients
// c_i = b_i . w from the partials of the dots in front; per value t = double(w), t = t - c_0 double(b_0), ..., w = T(t) -- and the partial sums of
// w . w of the new w (pass 1: set 0 of out_ww, pass 2: set 1).  The coefficients only orthogonalise: none of them is kept.
template <typename T, bool SECOND>
__global__ __launch_bounds__(kThreads) void svds_update_kernel(const T *__restrict__ V, long long stride, T *__restrict__ w, long long n, int ncols,
                                                               const double *__restrict__ part, double *__restrict__ out_ww, const SvdCell *__restrict__ cell)
{
    __shared__ double shs[kSvdMaxM][kWaves];          // the largest pass, the right half of step m - 1, has m <= kSvdMaxM columns
    __shared__ double hs[kSvdMaxM];
    __shared__ double shw[1][kWaves];
    __shared__ int    stopped;
    if (threadIdx.x == 0) stopped = cell->stop;
    sum_sets(part, ncols, hs, shs);
    if (stopped) return;
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T      wv[kPack<T>];
        double t[kPack<T>];
        load_pack<T, true>(w, e, (int)cnt, wv);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) t[l] = (double)wv[l];
        CVR_GMRES_GROUPS(sub_group, ncols, hs, t);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) {
            wv[l] = (T)t[l];
            if (l < cnt) acc[0] += (double)wv[l] * (double)wv[l];
        }
        store_pack<T, true>(w, e, (int)cnt, wv);
    }
    store_partials<1>(acc, out_ww + (SECOND ? kBlocks : 0), shw);
}

// The end of a half step of step j, behind the second pass: ww1 = w . w between the passes, ww = w . w of the new w, nrm = sqrt(ww) (the same in every
// workgroup; workgroup 0 records it: alpha_j in the left half, beta_(j+1) in the right one); a sum not finite: breakdown; ww <= ww1 / 4 (nrm == 0
// included): the half's space is closed at step j; otherwise next = T(double(w) / nrm): u_j in the left half, v_(j+1) in the right one.
template <typename T, bool LEFT>
__global__ __launch_bounds__(kThreads) void svds_finish_kernel(const T *__restrict__ w, T *__restrict__ next, long long n, const double *__restrict__ part_ww,
                                                               SvdCell *__restrict__ cell, int j)
{
    __shared__ double sh[2][kWaves];
    __shared__ int    stopped;
    if (threadIdx.x == 0) stopped = cell->stop;
    double s[2];
    sum_partials<2>(part_ww, s, sh);
    if (stopped) return;
    const bool   first = blockIdx.x == 0 && threadIdx.x == 0;
    const double nrm = sqrt(s[1]);
    const bool   closed = s[1] <= 0.25 * s[0];
    if (!(fabs(s[0]) <= kDblMax) || !(fabs(s[1]) <= kDblMax)) {
        if (first) { cell->status = CVR_EIG_BREAKDOWN; cell->stop = 1; }
        return;
    }
    if (first) {
        if constexpr (LEFT) cell->alpha[j] = nrm;
        else cell->beta[j + 1] = nrm;
        if (closed) { cell->status = LEFT ? kSvdClosedLeft : kSvdClosedRight; cell->j = j; cell->stop = 1; }
    }
    if (closed) return;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T wv[kPack<T>];
        load_pack<T, true>(w, e, (int)cnt, wv);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) wv[l] = (T)((double)wv[l] / nrm);
        store_pack<T, true>(next, e, (int)cnt, wv);
    }
}

}  // namespace
}  // namespace krylov
}  // namespace cvrh
