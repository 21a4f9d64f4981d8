// cvr_krylov.h -- what the Krylov solvers share (cvr_cg.hip, cvr_cg_multi.hip, cvr_bicgstab.hip, cvr_gmres.hip, cvr_lsqr.hip, cvr_minres.hip) and the
// preconditioner objects that run on their grid (cvr_precond.hip, cvr_chebyshev.hip, cvr_pcg_multi.hip).  The device half: the fixed grid, the
// 16-byte packet helpers and the fixed-tree fp64 sums.  Every translation unit that includes it gets the same code, so a sum has the same bits
// whichever solver forms it.  The host half, below it: the argument checks and the driver every solver runs --
//   check the handle | carve one allocation (Arena) | begin the clock | zero the pad slots of the SpMV inputs | r = b - A x0 (start_residual) |
//   the solver's start kernels | batches of steps with one read-back of the state cell each (run_batches) | clear x where b == 0 | fill_result
// A solver supplies its cell, its kernels, the function that enqueues step k and the one that reads the cell back and says whether it has stopped.
// Each method has one solve function; a preconditioner (none, the diagonal opt->minv_dev, a cvr_precond object: cvr_precond.h) is an argument of it.
#pragma once
#include "cvr_internal.h"

namespace cvrh {
namespace krylov {

constexpr int kBlocks = 1024, kThreads = 256;          // cvr_iter.hip's grid: the partial count is fixed
constexpr int kWaves = kThreads / 64;
static_assert(kBlocks == 4 * kThreads, "sum_partials reads four partials per thread");
constexpr int kDefaultCheckEvery = 8;
constexpr double kDblMax = 1.7976931348623157e308;

__device__ __forceinline__ bool usable(double v) { return v != 0 && fabs(v) <= kDblMax; }          // neither zero nor Inf nor NaN

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

// The state cell of conjugate gradients (cvr_cg.hip; batched CG keeps one per column), here because the preconditioners' applies inside the solver
// read it (cvr_precond.h).  Written by thread 0 of workgroup 0 only; a value a kernel reads is one that a kernel BEFORE it wrote (r.z of the step
// before sits in rz[k & 1], this step's goes to rz[(k + 1) & 1]) -- except `stop`, which the other workgroups of the kernel that sets it may or may
// not see yet: they come to the same decision from the same sums, so either way they return without writing.
namespace {
struct CgCell {
    double  bb, bnorm;         // b . b and its root
    double  rr, rnorm;         // r . r of the last iterate and its root
    double  rz[2];
    int32_t stop;              // != 0: no kernel writes a vector any more
    int32_t status;            // CVR_CG_*
    int32_t iters;             // steps applied to x
    int32_t zero_x;            // b == 0: the solution is x = 0 (the host clears it)
};
}  // namespace

// ---- the host half

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

// what every solver asks of the handle: "<entry> before cvr_preprocess", "<needs> a square matrix (r x c)"
inline int check_square_preprocessed(const cvr_handle *h, const char *entry, const char *needs)
{
    if (!h->converted) return fail(CVR_ERR_STATE, "%s before cvr_preprocess", entry);
    if (h->info.nrows != h->info.ncols) return fail(CVR_ERR_INVALID, "%s a square matrix (%lld x %lld)", needs, (long long)h->info.nrows, (long long)h->info.ncols);
    return CVR_OK;
}

// The bytes of `cols` vectors that an SpMV of the (square) handle reads, pad slot included, and writes, and of plain ones of n values.  x_elems is
// ncols + 1 = n + 1 (cvr_capi.hip), so the first max only says so: it cannot shrink a buffer.
inline size_t x_ext_bytes(const cvr_handle *h, int cols = 1) { return h->vsz * (size_t)cols * (size_t)std::max<int64_t>(h->info.x_elems, h->info.nrows + 1); }
inline size_t y_ext_bytes(const cvr_handle *h, int cols = 1) { return h->vsz * (size_t)cols * (size_t)std::max<int64_t>({h->info.yext_elems, h->info.nrows, 1}); }
inline size_t vec_bytes(const cvr_handle *h, int cols = 1) { return h->vsz * (size_t)cols * (size_t)std::max<int64_t>(h->info.nrows, 1); }

// The library's buffers of one call in one device allocation, and the call's two timing events.  Sizes are added in 256-byte slots, in the order the
// buffers lie; then one alloc(), then at<T>(offset).
class Arena {
  public:
    Arena() = default;
    Arena(const Arena &) = delete;
    Arena &operator=(const Arena &) = delete;
    ~Arena()
    {
        if (base_) (void)hipFree(base_);
        if (e0_) (void)hipEventDestroy(e0_);
        if (e1_) (void)hipEventDestroy(e1_);
    }
    static size_t slot(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    size_t        add(size_t bytes)
    {
        const size_t off = total_;
        total_ += slot(bytes);
        return off;
    }
    size_t     total() const { return total_; }
    hipError_t alloc()
    {
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&base_), total_);
        if (e != hipSuccess) base_ = nullptr;
        return e;
    }
    template <typename T> T *at(size_t off) const { return reinterpret_cast<T *>(base_ + off); }
    int begin(hipStream_t st)          // the clock starts on `st`
    {
        HIP_TRY(hipEventCreate(&e0_));
        HIP_TRY(hipEventCreate(&e1_));
        HIP_TRY(hipEventRecord(e0_, st));
        return CVR_OK;
    }
    int seconds(hipStream_t st, double *out)          // ... and stops behind what `st` holds now; synchronises
    {
        HIP_TRY(hipEventRecord(e1_, st));
        HIP_TRY(hipStreamSynchronize(st));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e0_, e1_));
        *out = (double)ms * 1e-3;
        return CVR_OK;
    }

  private:
    uint8_t   *base_ = nullptr;
    size_t     total_ = 0;
    hipEvent_t e0_ = nullptr, e1_ = nullptr;
};

// the pad slot of an SpMV input of vb bytes of values: value n = 0
inline int zero_pad_slot(void *buf, size_t vb, size_t vsz, hipStream_t st)
{
    HIP_TRY(hipMemsetAsync(static_cast<uint8_t *>(buf) + vb, 0, vsz, st));
    return CVR_OK;
}

// xin = x (an SpMV input whose pad slot is zero), r = b, r = b - A xin: the scaled product
inline int start_residual(cvr_handle *h, void *xin, void *r, const void *x, const void *b, long long n, hipStream_t st)
{
    if (n) {
        HIP_TRY(hipMemcpyAsync(xin, x, h->vsz * (size_t)n, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(r, b, h->vsz * (size_t)n, hipMemcpyDeviceToDevice, st));
    }
    return spmv_scaled_enqueue(h, -1.0, xin, 1.0, r, st);
}

// the state cell (or its head) to the host, behind everything `st` holds
inline int read_cell(void *dst, const void *src, size_t bytes, hipStream_t st)
{
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CVR_OK;
}

// The loop: steps 0, 1, .. enqueued through enqueue_step(k) in batches of check_every (the last one shorter), behind each batch read_back(done, &stopped)
// with done = the steps enqueued so far; it ends when that says so or at max_iters.  Both return a CVR_* code; the first that is not CVR_OK ends the call.
template <typename Step, typename ReadBack>
int run_batches(const cvr_cg_options *opt, Step &&enqueue_step, ReadBack &&read_back)
{
    const int every = opt->check_every > 0 ? opt->check_every : kDefaultCheckEvery;
    for (int done = 0;;) {
        const int batch = std::min(every, opt->max_iters - done);
        for (int i = 0; i < batch; i++)
            if (const int rc = enqueue_step(done + i)) return rc;
        done += batch;
        bool stopped = false;
        if (const int rc = read_back(done, &stopped)) return rc;
        if (stopped || done >= opt->max_iters) return CVR_OK;
    }
}

inline void fill_result(cvr_cg_result *res, int32_t iters, int32_t status, int spmvs, double rnorm, double bnorm, double seconds)
{
    memset(res, 0, sizeof(*res));
    res->iterations = iters;
    res->status = status;
    res->spmv_count = spmvs;
    res->residual_norm = rnorm;
    res->b_norm = bnorm;
    res->seconds = seconds;
}

// The tail of a single-vector solve, behind run_batches: x = 0 where b == 0, the clock, the result from the cell (or its head) the host read back last
template <typename Cell>
int finish_solve(Arena &a, hipStream_t st, void *x, size_t vb, const Cell &cell, int spmvs, cvr_cg_result *res)
{
    if (cell.zero_x && vb) HIP_TRY(hipMemsetAsync(x, 0, vb, st));
    double seconds = 0;
    if (const int rc = a.seconds(st, &seconds)) return rc;
    fill_result(res, cell.iters, cell.status, spmvs, cell.rnorm, cell.bnorm, seconds);
    return CVR_OK;
}

// A host entry point around its device form fn(b_dev, x_dev, stream): the handle's own vectors carry b and x (d_x has ncols + 1 values, d_y at least nrows)
template <typename Fn>
int solve_from_host(cvr_handle *h, const void *b_host, void *x_host, Fn &&fn)
{
    HIP_TRY(hipSetDevice(h->device));
    const size_t vb = h->vsz * (size_t)h->info.nrows;
    if (vb) {
        HIP_TRY(hipMemcpyAsync(h->d_x, x_host, vb, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(h->d_y, b_host, vb, hipMemcpyHostToDevice, h->stream));
    }
    if (const int rc = fn(h->d_y, h->d_x, h->stream)) return rc;
    if (vb) HIP_TRY(hipMemcpyAsync(x_host, h->d_x, vb, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return CVR_OK;
}

// One launch on the solvers' grid.
template <typename... P, typename... A>
void launch(void (*kernel)(P...), hipStream_t st, A... args)
{
    hipLaunchKernelGGL(kernel, dim3(kBlocks), dim3(kThreads), 0, st, args...);
}

// Runtime booleans into compile-time ones: with_flags(f, a, b) calls f(std::bool_constant<a>(), std::bool_constant<b>()), so a generic lambda
// names the kernel instantiation once -- kernel<T, pre, al> -- and its argument list once.  A kernel that has no <T, false, false> form says so
// there: kernel<T, pre, al || !pre>.
template <typename F, typename... Bs>
auto with_flags(F &&f, bool b, Bs... bs)
{
    auto bound = [&](auto c) {
        if constexpr (sizeof...(bs) == 0) return f(c);
        else return with_flags([&](auto... cs) { return f(c, cs...); }, bs...);
    };
    return b ? bound(std::true_type()) : bound(std::false_type());
}
// ... and the handle's value type: f(float()) or f(double())
template <typename F>
auto with_value_type(const cvr_handle *h, F &&f)
{
    return h->vsz == 4 ? f(float()) : f(double());
}

}  // namespace krylov
}  // namespace cvrh
