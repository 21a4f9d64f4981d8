// cvr_lobpcg_kernels.h -- the vector kernels of the block eigensolver (cvr_lobpcg.hip: cvr_lobpcg_device).  What each kernel does: cvr_lobpcg.hip's
// head.  All of them run on cvr_krylov.h's grid over the library's own blocks (16-byte packets, every column at a multiple of 256 bytes), every sum
// is store_partials' tree into partials of its own and sum_partials' tree over them, and none waits on another workgroup.
// KB: the block size k rounded up to 1, 2, 4 or 8 -- the compile-time extent of the loops over a block's columns; columns k .. KB - 1 do not exist:
// they are not loaded, not stored, and the sums they would enter are never read.
#pragma once
#include "cvr_krylov.h"
#include "cvr_basis_groups.h"

namespace cvrh {
namespace krylov {
namespace {

constexpr int kLobMaxK = CVR_LOBPCG_MAX_BLOCK, kLobMaxM = 3 * kLobMaxK;
constexpr int kLobPairs = 6;                                    // the 8 x 8 blocks of the lower triangle of a 24 x 24 matrix
constexpr int kLobGramSets = 2 * kLobPairs * kLobMaxK * kLobMaxK;          // G and H

struct LobTheta { double v[kLobMaxK]; };          // the Ritz values of X, by value

// the packets at e of the k columns at V (the others 0)
template <typename T, int KB>
__device__ __forceinline__ void load_block(const T *__restrict__ V, long long stride, int k, long long e, int cnt, T (&v)[KB][kPack<T>])
{
#pragma unroll
    for (int c = 0; c < KB; c++) {
        if (c < k) load_pack<T, true>(V + c * stride, e, cnt, v[c]);
        else {
#pragma unroll
            for (int l = 0; l < kPack<T>; l++) v[c][l] = (T)0;
        }
    }
}

// set i * KB + j of `out` = the partial sums of A_i . B_j for the k x k column pairs of two blocks: KB * KB fp64 accumulators per thread, a packet of
// each of the 2 k columns loaded once per trip; the terms double(a) * double(b) added in element order from +0 (dot_group's order, entry by entry)
template <typename T, int KB>
__device__ __forceinline__ void gram_block(const T *__restrict__ A, const T *__restrict__ B, long long stride, long long n, int k, double *__restrict__ out,
                                           double (&sh)[KB * KB][kWaves])
{
    double acc[KB * KB];
#pragma unroll
    for (int i = 0; i < KB * KB; i++) acc[i] = 0;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T av[KB][kPack<T>], bv[KB][kPack<T>];
        load_block<T, KB>(A, stride, k, e, (int)cnt, av);
        load_block<T, KB>(B, stride, k, e, (int)cnt, bv);
#pragma unroll
        for (int i = 0; i < KB; i++)
#pragma unroll
            for (int j = 0; j < KB; j++)
#pragma unroll
                for (int l = 0; l < kPack<T>; l++) if (l < cnt) acc[i * KB + j] += (double)av[i][l] * (double)bv[j][l];
    }
    store_partials<KB * KB>(acc, out, sh);
}

// Step 1: R_c = T(double(AX_c) - theta_c * double(X_c)) and the partial sums of R_c . R_c (set c), all columns in one launch
template <typename T, int KB>
__global__ __launch_bounds__(kThreads) void lobpcg_residual_kernel(const T *__restrict__ X, const T *__restrict__ AX, long long stride, long long n, int k,
                                                                   LobTheta th, T *__restrict__ R, double *__restrict__ part_rn)
{
    __shared__ double sh[KB][kWaves];
    double acc[KB];
#pragma unroll
    for (int c = 0; c < KB; c++) acc[c] = 0;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
#pragma unroll
        for (int c = 0; c < KB; c++) {
            if (c < k) {
                T xv[kPack<T>], av[kPack<T>];
                load_pack<T, true>(X + c * stride, e, (int)cnt, xv);
                load_pack<T, true>(AX + c * stride, e, (int)cnt, av);
#pragma unroll
                for (int l = 0; l < kPack<T>; l++) {
                    av[l] = (T)((double)av[l] - th.v[c] * (double)xv[l]);
                    if (l < cnt) acc[c] += (double)av[l] * (double)av[l];
                }
                store_pack<T, true>(R + c * stride, e, (int)cnt, av);
            }
        }
    }
    store_partials<KB>(acc, part_rn, sh);
}

// Step 3, the sums: set i * KB + c of `part` = the partial sums of X_i . W_c
template <typename T, int KB>
__global__ __launch_bounds__(kThreads) void lobpcg_dots_kernel(const T *__restrict__ X, const T *__restrict__ W, long long stride, long long n, int k,
                                                               double *__restrict__ part)
{
    __shared__ double sh[KB * KB][kWaves];
    gram_block<T, KB>(X, W, stride, n, k, part, sh);
}

// Step 3, one pass: the coefficients h_ic = X_i . W_c from the partials in front, summed in every workgroup in the same order (gmres_update_kernel's
// way: no read-back); per value t = double(w_c), t = t - h_0c * double(x_0), ..., t = t - h_(k-1)c * double(x_(k-1)), w_c = T(t); and the partial
// sums of W_c . W_c of the new W (set c of part_ww)
template <typename T, int KB>
__global__ __launch_bounds__(kThreads) void lobpcg_update_kernel(const T *__restrict__ X, T *__restrict__ W, long long stride, long long n, int k,
                                                                 const double *__restrict__ part, double *__restrict__ part_ww)
{
    __shared__ double shs[KB * KB][kWaves];
    __shared__ double hs[KB * KB];
    __shared__ double shw[KB][kWaves];
    sum_sets(part, KB * KB, hs, shs);
    double acc[KB];
#pragma unroll
    for (int c = 0; c < KB; c++) acc[c] = 0;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T xv[KB][kPack<T>];
        load_block<T, KB>(X, stride, k, e, (int)cnt, xv);
#pragma unroll
        for (int c = 0; c < KB; c++) {
            if (c < k) {
                T      wv[kPack<T>];
                double t[kPack<T>];
                load_pack<T, true>(W + c * stride, e, (int)cnt, wv);
#pragma unroll
                for (int l = 0; l < kPack<T>; l++) t[l] = (double)wv[l];
#pragma unroll
                for (int i = 0; i < KB; i++) {
                    if (i < k) {
                        const double h = hs[i * KB + c];
#pragma unroll
                        for (int l = 0; l < kPack<T>; l++) t[l] = t[l] - h * (double)xv[i][l];
                    }
                }
#pragma unroll
                for (int l = 0; l < kPack<T>; l++) {
                    wv[l] = (T)t[l];
                    if (l < cnt) acc[c] += (double)wv[l] * (double)wv[l];
                }
                store_pack<T, true>(W + c * stride, e, (int)cnt, wv);
            }
        }
    }
    store_partials<KB>(acc, part_ww, shw);
}

// s_c = the sum of set c of `part` (the same in every workgroup; workgroup 0 stores it at norm2[c]); a column whose s_c is finite and > 0 is divided
// by sqrt(s_c): A_c = T(double(A_c) / sqrt(s_c)), and B_c as well where B is not null.  A column whose s_c is not is left as it is: the host sees
// s_c in the read-back.
template <typename T>
__global__ __launch_bounds__(kThreads) void lobpcg_scale_kernel(T *__restrict__ A, T *__restrict__ B, long long stride, long long n, int k,
                                                                const double *__restrict__ part, double *__restrict__ norm2)
{
    __shared__ double shs[kLobMaxK][kWaves];
    __shared__ double hs[kLobMaxK];
    sum_sets(part, k, hs, shs);
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)k) norm2[threadIdx.x] = hs[threadIdx.x];
    for (int c = 0; c < k; c++) {
        const double s = hs[c];
        if (!(s > 0 && s <= kDblMax)) continue;
        const double nrm = sqrt(s);
        CVR_KRYLOV_PACKETS(T, e, cnt) {
            T v[kPack<T>];
            load_pack<T, true>(A + c * stride, e, (int)cnt, v);
#pragma unroll
            for (int l = 0; l < kPack<T>; l++) v[l] = (T)((double)v[l] / nrm);
            store_pack<T, true>(A + c * stride, e, (int)cnt, v);
            if (B) {
                load_pack<T, true>(B + c * stride, e, (int)cnt, v);
#pragma unroll
                for (int l = 0; l < kPack<T>; l++) v[l] = (T)((double)v[l] / nrm);
                store_pack<T, true>(B + c * stride, e, (int)cnt, v);
            }
        }
    }
}

// Step 5: the partial sums of one 8 x 8 block of G = S^T S or of H = S^T (A S) per blockIdx.y = 2 * pair + (1 for H); pair 0 .. 5 = the blocks
// (0,0) (1,0) (1,1) (2,0) (2,1) (2,2) of the lower triangle, block b = the columns b k .. b k + k - 1 (X, W, P).  Entry (i, j) of the block, S_(bi k + i)
// . S_(bj k + j) or . (A S)_(bj k + j), has the set (blockIdx.y * KB + i) * KB + j.
template <typename T, int KB>
__global__ __launch_bounds__(kThreads) void lobpcg_gram_kernel(const T *__restrict__ S, const T *__restrict__ AS, long long stride, long long n, int k,
                                                               double *__restrict__ part)
{
    __shared__ double sh[KB * KB][kWaves];
    const int y = blockIdx.y, pair = y >> 1;
    const int bi = pair >= 3 ? 2 : pair >= 1 ? 1 : 0, bj = pair - bi * (bi + 1) / 2;
    gram_block<T, KB>(S + (long long)bi * k * stride, ((y & 1) ? AS : S) + (long long)bj * k * stride, stride, n, k, part + (size_t)y * KB * KB * kBlocks, sh);
}

// Step 6, the sums: out[set] = sum_partials' tree over the set, one workgroup per set (grid = the sets)
__global__ __launch_bounds__(kThreads) void lobpcg_reduce_kernel(const double *__restrict__ part, double *__restrict__ out)
{
    __shared__ double sh[1][kWaves];
    double s[1];
    sum_partials<1>(part + (size_t)blockIdx.x * kBlocks, s, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

// u = u + cs[c] * double(v) for the KB columns of one output block
template <typename T, int KB>
__device__ __forceinline__ void combine_add(const double *__restrict__ cs, const T (&v)[kPack<T>], double (&u)[KB][kPack<T>])
{
#pragma unroll
    for (int c = 0; c < KB; c++) {
        const double cc = cs[c];
#pragma unroll
        for (int q = 0; q < kPack<T>; q++) u[c][q] = u[c][q] + cc * (double)v[q];
    }
}

// Step 7: X' = S C and AX' = (A S) C over the m columns l ascending from +0, and with WITH_P also P' = S C~ and AP' = (A S) C~, which are the same sums
// over l = k .. m - 1 only (the rows of C~ in front are zero), into the other set of blocks (So, ASo: X' in block 0, P' in block 2); C (row l at
// C + l * 8, the columns past k zero) sits in LDS; a thread owns its packets and reads its m values of S and of A S once for all outputs.  WITH_P:
// the partial sums of P'_c . P'_c (set c of part_pn) for lobpcg_scale_kernel behind it.
template <typename T, int KB, bool WITH_P>
__global__ __launch_bounds__(kThreads) void lobpcg_combine_kernel(const T *__restrict__ S, const T *__restrict__ AS, long long stride, long long n, int m, int k,
                                                                  const double *__restrict__ C, T *__restrict__ So, T *__restrict__ ASo,
                                                                  double *__restrict__ part_pn)
{
    __shared__ double cs[kLobMaxM * kLobMaxK];
    __shared__ double sh[KB][kWaves];
    for (int i = threadIdx.x; i < m * kLobMaxK; i += kThreads) cs[i] = C[i];
    __syncthreads();
    double accp[KB];
#pragma unroll
    for (int c = 0; c < KB; c++) accp[c] = 0;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        double x[KB][kPack<T>], ax[KB][kPack<T>], p[WITH_P ? KB : 1][kPack<T>], ap[WITH_P ? KB : 1][kPack<T>];
#pragma unroll
        for (int c = 0; c < KB; c++)
#pragma unroll
            for (int q = 0; q < kPack<T>; q++) {
                x[c][q] = 0; ax[c][q] = 0;
                if constexpr (WITH_P) { p[c][q] = 0; ap[c][q] = 0; }
            }
        for (int l = 0; l < k; l++) {
            T sv[kPack<T>], av[kPack<T>];
            load_pack<T, true>(S + l * stride, e, (int)cnt, sv);
            load_pack<T, true>(AS + l * stride, e, (int)cnt, av);
            combine_add<T, KB>(cs + l * kLobMaxK, sv, x);
            combine_add<T, KB>(cs + l * kLobMaxK, av, ax);
        }
        for (int l = k; l < m; l++) {
            T sv[kPack<T>], av[kPack<T>];
            load_pack<T, true>(S + l * stride, e, (int)cnt, sv);
            load_pack<T, true>(AS + l * stride, e, (int)cnt, av);
            combine_add<T, KB>(cs + l * kLobMaxK, sv, x);
            combine_add<T, KB>(cs + l * kLobMaxK, av, ax);
            if constexpr (WITH_P) {
                combine_add<T, KB>(cs + l * kLobMaxK, sv, p);
                combine_add<T, KB>(cs + l * kLobMaxK, av, ap);
            }
        }
#pragma unroll
        for (int c = 0; c < KB; c++) {
            if (c < k) {
                T o[kPack<T>];
#pragma unroll
                for (int q = 0; q < kPack<T>; q++) o[q] = (T)x[c][q];
                store_pack<T, true>(So + c * stride, e, (int)cnt, o);
#pragma unroll
                for (int q = 0; q < kPack<T>; q++) o[q] = (T)ax[c][q];
                store_pack<T, true>(ASo + c * stride, e, (int)cnt, o);
                if constexpr (WITH_P) {
#pragma unroll
                    for (int q = 0; q < kPack<T>; q++) {
                        o[q] = (T)p[c][q];
                        if (q < cnt) accp[c] += (double)o[q] * (double)o[q];
                    }
                    store_pack<T, true>(So + (2 * k + c) * stride, e, (int)cnt, o);
#pragma unroll
                    for (int q = 0; q < kPack<T>; q++) o[q] = (T)ap[c][q];
                    store_pack<T, true>(ASo + (2 * k + c) * stride, e, (int)cnt, o);
                }
            }
        }
    }
    if constexpr (WITH_P) store_partials<KB>(accp, part_pn, sh);
}

}  // namespace
}  // namespace krylov
}  // namespace cvrh
