// cvr_krylov.h -- what the Krylov solvers' vector kernels share (cvr_cg.hip, cvr_cg_multi.hip, cvr_bicgstab.hip, cvr_gmres.hip): the fixed grid, the 16-byte packet helpers, the
// fixed-tree fp64 sums and the argument checks of their entry points.  Every translation unit that includes it gets the same code, so a sum has
// the same bits whichever solver forms it.
#pragma once
#include "cvr_internal.h"

namespace cvrh {
namespace krylov {

constexpr int kBlocks = 1024, kThreads = 256;          // cvr_iter.hip's grid: the partial count is fixed
constexpr int kWaves = kThreads / 64;
static_assert(kBlocks == 4 * kThreads, "sum_partials reads four partials per thread");
constexpr int kDefaultCheckEvery = 8;

template <typename T> struct Vec;
template <> struct Vec<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct Vec<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <typename T> constexpr int kPack = 16 / (int)sizeof(T);          // values per 16-byte packet

// the packet at p + e: one 16-byte load when it is whole and p is 16-byte aligned (VEC), else its `cnt` values one by one; the rest 0
template <typename T, bool VEC>
__device__ __forceinline__ void load_pack(const T *__restrict__ p, long long e, int cnt, T (&v)[kPack<T>])
{
    if (VEC && cnt == kPack<T>) {
        const typename Vec<T>::type t = *reinterpret_cast<const typename Vec<T>::type *>(p + e);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) v[j] = t[j];
    } else {
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) v[j] = j < cnt ? p[e + j] : (T)0;
    }
}
template <typename T, bool VEC>
__device__ __forceinline__ void store_pack(T *__restrict__ p, long long e, int cnt, const T (&v)[kPack<T>])
{
    if (VEC && cnt == kPack<T>) {
        typename Vec<T>::type t;
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) t[j] = v[j];
        *reinterpret_cast<typename Vec<T>::type *>(p + e) = t;
    } else {
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) if (j < cnt) p[e + j] = v[j];
    }
}

// s[k] = the sum of the k-th set of kBlocks partials, the same bits in every thread of every workgroup: thread t takes partials t, t + 256, t + 512,
// t + 768 in that order, the lanes of a wavefront a butterfly, the four wavefronts in order.  Ends behind a barrier (what thread 0 put into LDS
// before the call is visible after it).
template <int K>
__device__ __forceinline__ void sum_partials(const double *__restrict__ part, double (&s)[K], double (&sh)[K][kWaves])
{
#pragma unroll
    for (int k = 0; k < K; k++) {
        double a = 0;
#pragma unroll
        for (int j = 0; j < kBlocks / kThreads; j++) a += part[(size_t)k * kBlocks + threadIdx.x + j * kThreads];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if ((threadIdx.x & 63u) == 0) sh[k][threadIdx.x >> 6] = a;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        double a = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) a += sh[k][w];
        s[k] = a;
    }
}

// out[k * kBlocks + workgroup] = the workgroup's sum of acc[k]: dot_partial_kernel's tree
template <int K>
__device__ __forceinline__ void store_partials(double (&acc)[K], double *__restrict__ out, double (&sh)[K][kWaves])
{
#pragma unroll
    for (int k = 0; k < K; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
        if ((threadIdx.x & 63u) == 0) sh[k][threadIdx.x >> 6] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            double a = 0;
#pragma unroll
            for (int w = 0; w < kWaves; w++) a += sh[k][w];
            out[(size_t)k * kBlocks + blockIdx.x] = a;
        }
    }
}

// the packets of a thread over n values, in order: e = the first value of the packet, cnt = how many of its values exist
#define CVR_KRYLOV_PACKETS(T, e, cnt)                                                                                              \
    for (long long e = ((long long)blockIdx.x * kThreads + threadIdx.x) * kPack<T>, cnt = 0; e < n && ((cnt = n - e < kPack<T> ? n - e : kPack<T>), true); \
         e += (long long)kBlocks * kThreads * kPack<T>)

// what the solvers' entry points check before any device work and before the handle is looked at
inline int check_solver_args(const void *h, const void *b, const void *x, const cvr_cg_options *opt, const cvr_cg_result *res)
{
    if (!h || !b || !x || !opt || !res) return fail(CVR_ERR_INVALID, "null argument");
    if (opt->max_iters < 0 || opt->check_every < 0) return fail(CVR_ERR_INVALID, "max_iters = %d, check_every = %d: must not be negative", opt->max_iters, opt->check_every);
    if (!(opt->rtol >= 0) || !std::isfinite(opt->rtol)) return fail(CVR_ERR_INVALID, "rtol = %g: must be finite and not negative", opt->rtol);
    for (int i = 0; i < 4; i++)
        if (opt->reserved[i] != 0) return fail(CVR_ERR_INVALID, "cvr_cg_options.reserved[%d] = %d: must be 0", i, opt->reserved[i]);
    return CVR_OK;
}

}  // namespace krylov
}  // namespace cvrh
