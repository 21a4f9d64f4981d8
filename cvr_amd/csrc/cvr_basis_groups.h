// cvr_basis_groups.h -- sums against a whole basis and updates by it, the columns in compile-time groups: what GMRES(m) (cvr_gmres_kernels.h) and the
// Lanczos eigensolver (cvr_lanczos_kernels.h) share.  Every translation unit that includes it gets the same code, so a coefficient has the same bits
// whichever solver forms it.
#pragma once
#include "cvr_krylov.h"

namespace cvrh {
namespace krylov {
namespace {

constexpr int    kGroup = 8;          // columns per compile-time group: 16 accumulator VGPRs in fp64, and the group's packets in flight together

// hs[s] = the sum of the s-th set of kBlocks partials for s < nsets, in LDS: sum_partials' tree set by set (the same bits as sum_partials<1> of that set), the
// same in every workgroup.  Ends behind a barrier.
__device__ __forceinline__ void sum_sets(const double *__restrict__ part, int nsets, double *__restrict__ hs, double (*__restrict__ sh)[kWaves])
{
    for (int s = 0; s < nsets; s++) {
        double a = 0;
#pragma unroll
        for (int j = 0; j < kBlocks / kThreads; j++) a += part[(size_t)s * kBlocks + threadIdx.x + j * kThreads];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if ((threadIdx.x & 63u) == 0) sh[s][threadIdx.x >> 6] = a;
    }
    __syncthreads();
    for (int s = threadIdx.x; s < nsets; s += kThreads) {
        double a = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) a += sh[s][w];
        hs[s] = a;
    }
    __syncthreads();
}

// the partial sums of V_c . w for the C columns at V (one pass over w and over each of them)
template <typename T, int C>
__device__ __forceinline__ void dot_group(const T *__restrict__ V, long long stride, const T *__restrict__ w, long long n, double *__restrict__ out,
                                          double (&sh)[kGroup][kWaves])
{
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 0;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T wv[kPack<T>], vv[C][kPack<T>];
        load_pack<T, true>(w, e, (int)cnt, wv);
#pragma unroll
        for (int c = 0; c < C; c++) load_pack<T, true>(V + c * stride, e, (int)cnt, vv[c]);
#pragma unroll
        for (int c = 0; c < C; c++)
#pragma unroll
            for (int j = 0; j < kPack<T>; j++) if (j < cnt) acc[c] += (double)vv[c][j] * (double)wv[j];
    }
    store_partials<C>(acc, out, reinterpret_cast<double (&)[C][kWaves]>(sh));
}

// t = t - hs[c] * double(V_c) for c = 0 .. C - 1 in that order, the C packets loaded together
template <typename T, int C>
__device__ __forceinline__ void sub_group(const T *__restrict__ V, long long stride, long long e, int cnt, const double *__restrict__ hs, double (&t)[kPack<T>])
{
    T vv[C][kPack<T>];
#pragma unroll
    for (int c = 0; c < C; c++) load_pack<T, true>(V + c * stride, e, cnt, vv[c]);
#pragma unroll
    for (int c = 0; c < C; c++) {
        const double hc = hs[c];
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) t[j] = t[j] - hc * (double)vv[c][j];
    }
}

// u = u + ys[c] * double(V_c), the same way
template <typename T, int C>
__device__ __forceinline__ void add_group(const T *__restrict__ V, long long stride, long long e, int cnt, const double *__restrict__ ys, double (&u)[kPack<T>])
{
    T vv[C][kPack<T>];
#pragma unroll
    for (int c = 0; c < C; c++) load_pack<T, true>(V + c * stride, e, cnt, vv[c]);
#pragma unroll
    for (int c = 0; c < C; c++) {
        const double yc = ys[c];
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) u[j] = u[j] + yc * (double)vv[c][j];
    }
}

#define CVR_GMRES_GROUPS(fn, ncols, coef, acc)                                                              \
    do {                                                                                                    \
        int c0_ = 0;                                                                                        \
        for (; c0_ + kGroup <= (ncols); c0_ += kGroup) fn<T, kGroup>(V + c0_ * stride, stride, e, (int)cnt, (coef) + c0_, acc); \
        const T *Vr_ = V + c0_ * stride;                                                                    \
        switch ((ncols) - c0_) {                                                                            \
        case 1: fn<T, 1>(Vr_, stride, e, (int)cnt, (coef) + c0_, acc); break;                               \
        case 2: fn<T, 2>(Vr_, stride, e, (int)cnt, (coef) + c0_, acc); break;                               \
        case 3: fn<T, 3>(Vr_, stride, e, (int)cnt, (coef) + c0_, acc); break;                               \
        case 4: fn<T, 4>(Vr_, stride, e, (int)cnt, (coef) + c0_, acc); break;                               \
        case 5: fn<T, 5>(Vr_, stride, e, (int)cnt, (coef) + c0_, acc); break;                               \
        case 6: fn<T, 6>(Vr_, stride, e, (int)cnt, (coef) + c0_, acc); break;                               \
        case 7: fn<T, 7>(Vr_, stride, e, (int)cnt, (coef) + c0_, acc); break;                               \
        default: break;                                                                                     \
        }                                                                                                   \
    } while (0)

}  // namespace
}  // namespace krylov
}  // namespace cvrh
