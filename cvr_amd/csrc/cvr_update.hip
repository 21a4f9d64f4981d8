// cvr_update.hip -- new values for a converted handle of the same sparsity pattern (include/cvr_amd.h: cvr_options.mutable_values,
// cvr_update_values_device, cvr_update_values, cvr_update_values_supported).
//
// A mutable handle is converted with the CSR position of every value in place of the value: element i of the array the converter reads
// holds the bit pattern of i + 1 (as u64 / u32 of the value type; 0 stays the pad slots' value).  Nothing between the upload and the
// image does arithmetic or comparisons on values -- the column-panel split, the interleaved / gang sorts and the converters move them as
// they are, and with the dictionary off the image's structure depends on the pattern alone --, so the value block of that image names,
// slot by slot, where its value comes from.  value_map_kernel compacts it into one u32 per slot (the map, kept by the handle: 4 bytes per
// slot), and update_values_kernel writes values through it: the caller's values of cvr_preprocess first (the creation values), then
// every cvr_update_values*.  No converter knows of any of this.
//
// Both kernels run one wavefront per group: lane l owns elements 4 l .. 4 l + 3 of the group's value block (one dwordx4 of the map, one
// or two dwordx4 of values: a wavefront writes the whole block, full lines), the groups of all parts numbered one after the other in a
// single grid (column panels: one launch for all of them).
#include "cvr_internal.h"

using namespace cvrh;

namespace cvr {
namespace {

// the part that holds group g: the last p with parts[p].g0 <= g (parts[nparts].g0 = all groups; g is uniform over the wavefront)
__device__ inline UpdatePart part_of(const UpdatePart *__restrict__ parts, uint32_t nparts, unsigned long long g)
{
    uint32_t lo = 0, hi = nparts;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (parts[mid].g0 <= g) lo = mid; else hi = mid;
    }
    return parts[lo];
}

__device__ inline unsigned long long wave_group()
{
    return (unsigned long long)blockIdx.x * 4 + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// four consecutive values of B (u64: two dwordx4, u32: one) in global memory (the streams' addresses come out of the parts table: without
// the address space the compiler would issue flat instructions)
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t           u32x4 __attribute__((ext_vector_type(4)));
#define CVR_GLOBAL(T) __attribute__((address_space(1))) T
template <typename B> struct Quad;
template <> struct Quad<unsigned long long> {
    __device__ static void load(const unsigned long long *p, unsigned long long v[4])
    {
        const CVR_GLOBAL(u64x2) *q = (const CVR_GLOBAL(u64x2) *)(uintptr_t)p;
        const u64x2 a = q[0], b = q[1];
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    }
    __device__ static void store(unsigned long long *p, const unsigned long long v[4])
    {
        CVR_GLOBAL(u64x2) *q = (CVR_GLOBAL(u64x2) *)(uintptr_t)p;
        q[0] = u64x2{v[0], v[1]};
        q[1] = u64x2{v[2], v[3]};
    }
};
template <> struct Quad<uint32_t> {
    __device__ static void load(const uint32_t *p, uint32_t v[4])
    {
        const u32x4 a = *(const CVR_GLOBAL(u32x4) *)(uintptr_t)p;
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    }
    __device__ static void store(uint32_t *p, const uint32_t v[4]) { *(CVR_GLOBAL(u32x4) *)(uintptr_t)p = u32x4{v[0], v[1], v[2], v[3]}; }
};

// B: the bits of the value type (unsigned long long for fp64, uint32_t for fp32): values are moved, never interpreted
template <typename B>
__global__ __launch_bounds__(256) void value_map_kernel(const UpdatePart *__restrict__ parts, uint32_t nparts, unsigned long long ngroups, uint32_t *__restrict__ map,
                                                        unsigned long long nvals, uint32_t *__restrict__ err_flag)
{
    const unsigned long long g = wave_group();
    if (g >= ngroups) return;
    const uint32_t   lane = threadIdx.x & 63u;
    const UpdatePart p = part_of(parts, nparts, g);
    B                v[4];
    Quad<B>::load(reinterpret_cast<const B *>(p.stream + (g - p.g0) * p.gbytes + p.voff) + 4 * lane, v);
    uint32_t m[4];
    bool     bad = false;
    for (int q = 0; q < 4; q++) {
        bad = bad || (unsigned long long)v[q] > nvals;
        m[q] = v[q] == 0 ? kNoSource : (uint32_t)(v[q] - 1);
    }
    reinterpret_cast<uint4 *>(map)[g * 64 + lane] = make_uint4(m[0], m[1], m[2], m[3]);
    if (bad) atomicOr(err_flag, 256u);
}

template <typename B>
__global__ __launch_bounds__(256) void update_values_kernel(const UpdatePart *__restrict__ parts, uint32_t nparts, unsigned long long ngroups, const uint32_t *__restrict__ map,
                                                            const B *__restrict__ vals)
{
    const unsigned long long g = wave_group();
    if (g >= ngroups) return;
    const uint32_t   lane = threadIdx.x & 63u;
    const UpdatePart p = part_of(parts, nparts, g);
    const uint4      m = reinterpret_cast<const uint4 *>(map)[g * 64 + lane];
    B                v[4];
    v[0] = m.x != kNoSource ? vals[m.x] : (B)0;
    v[1] = m.y != kNoSource ? vals[m.y] : (B)0;
    v[2] = m.z != kNoSource ? vals[m.z] : (B)0;
    v[3] = m.w != kNoSource ? vals[m.w] : (B)0;
    Quad<B>::store(reinterpret_cast<B *>(p.stream + (g - p.g0) * p.gbytes + p.voff) + 4 * lane, v);
}

template <typename B>
__global__ __launch_bounds__(256) void index_values_kernel(B *__restrict__ out, unsigned long long n)
{
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 + 4 <= n) {
        const B v[4] = {(B)(i0 + 1), (B)(i0 + 2), (B)(i0 + 3), (B)(i0 + 4)};
        Quad<B>::store(out + i0, v);
    } else
        for (unsigned long long i = i0; i < n; i++) out[i] = (B)(i + 1);
}

uint32_t wave_blocks(uint64_t ngroups) { return (uint32_t)((ngroups + 3) / 4); }

}  // namespace

hipError_t launch_value_map(const UpdatePart *parts, uint32_t nparts, uint64_t ngroups, bool f32, uint32_t *map, uint64_t nvals, uint32_t *err_flag, hipStream_t st)
{
    if (ngroups == 0) return hipSuccess;
    if (f32) hipLaunchKernelGGL(value_map_kernel<uint32_t>, dim3(wave_blocks(ngroups)), dim3(256), 0, st, parts, nparts, (unsigned long long)ngroups, map, (unsigned long long)nvals, err_flag);
    else hipLaunchKernelGGL(value_map_kernel<unsigned long long>, dim3(wave_blocks(ngroups)), dim3(256), 0, st, parts, nparts, (unsigned long long)ngroups, map, (unsigned long long)nvals, err_flag);
    return hipGetLastError();
}

hipError_t launch_update_values(const UpdatePart *parts, uint32_t nparts, uint64_t ngroups, bool f32, const uint32_t *map, const void *vals, hipStream_t st)
{
    if (ngroups == 0) return hipSuccess;
    if (f32) hipLaunchKernelGGL(update_values_kernel<uint32_t>, dim3(wave_blocks(ngroups)), dim3(256), 0, st, parts, nparts, (unsigned long long)ngroups, map, static_cast<const uint32_t *>(vals));
    else hipLaunchKernelGGL(update_values_kernel<unsigned long long>, dim3(wave_blocks(ngroups)), dim3(256), 0, st, parts, nparts, (unsigned long long)ngroups, map, static_cast<const unsigned long long *>(vals));
    return hipGetLastError();
}

hipError_t launch_index_values(void *out, uint64_t n, bool f32, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)((n + 1023) / 1024);
    if (f32) hipLaunchKernelGGL(index_values_kernel<uint32_t>, dim3(blocks), dim3(256), 0, st, static_cast<uint32_t *>(out), (unsigned long long)n);
    else hipLaunchKernelGGL(index_values_kernel<unsigned long long>, dim3(blocks), dim3(256), 0, st, static_cast<unsigned long long *>(out), (unsigned long long)n);
    return hipGetLastError();
}

}  // namespace cvr

namespace cvrh {

int mutable_tables(cvr_handle *h)
{
    std::vector<cvr::UpdatePart> t(h->parts.size() + 1, cvr::UpdatePart{nullptr, 0ull, 0u, 0u});
    unsigned long long g = 0;
    for (size_t i = 0; i < h->parts.size(); i++) {
        const cvr::DeviceImage &img = h->parts[i].img;
        if (img.dict) return fail(CVR_ERR_INTERNAL, "mutable_values: the image has a value dictionary");
        t[i] = cvr::UpdatePart{img.stream, g, (uint32_t)cvr::group_bytes(img.f32, false, img.c16, img.tag16),
                               (uint32_t)((img.c16 ? cvr::kCols16Bytes : cvr::kColsBytes) + (img.tag16 ? cvr::kTagBytes : 0))};
        g += (unsigned long long)h->parts[i].nchunks * (unsigned long long)img.G;
    }
    t.back().g0 = g;
    if (!h->d_upd) HIP_TRY(hipMalloc(&h->d_upd, sizeof(cvr::UpdatePart) * t.size()));
    HIP_TRY(hipMemcpyAsync(h->d_upd, t.data(), sizeof(cvr::UpdatePart) * t.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->map_groups = g;
    if (!h->z_free) HIP_TRY(hipEventCreateWithFlags(&h->z_free, hipEventDisableTiming));      // (the image is what every SpMV reads and every update writes: run_spmv orders them)
    return CVR_OK;
}

int mutable_after_convert(cvr_handle *h, bool keep_csr)
{
    if (!h->mutable_vals) return CVR_OK;
    int rc = mutable_tables(h);
    if (rc) return rc;
    const bool f32 = h->vsz == 4;
    if (!h->d_map) {          // the first conversion: the image's value blocks hold CSR positions + 1
        HIP_TRY(hipMalloc(&h->d_map, std::max<size_t>(sizeof(uint32_t) * 256 * (size_t)h->map_groups, 16)));
        uint32_t err = 0;
        HIP_TRY(hipMemsetAsync(h->d_err, 0, sizeof(uint32_t), h->stream));
        HIP_TRY(cvr::launch_value_map(h->d_upd, (uint32_t)h->parts.size(), h->map_groups, f32, h->d_map, (uint64_t)h->nvals, h->d_err, h->stream));
        HIP_TRY(hipMemcpyAsync(&err, h->d_err, sizeof(err), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemsetAsync(h->d_err, 0, sizeof(uint32_t), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (err) return fail(CVR_ERR_INTERNAL, "mutable_values: a slot of the image names no CSR position (flags 0x%x)", err);
    }
    if (h->d_vals0) HIP_TRY(cvr::launch_update_values(h->d_upd, (uint32_t)h->parts.size(), h->map_groups, f32, h->d_map, h->d_vals0, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!keep_csr && h->d_vals0) { (void)hipFree(h->d_vals0); h->d_vals0 = nullptr; }      // (kept CSR: a later cvr_preprocess converts positions again and writes these once more)
    return CVR_OK;
}

}  // namespace cvrh

namespace {

int check_update(const cvr_handle *h, const void *vals)
{
    if (!h || !vals) return fail(CVR_ERR_INVALID, "null argument");
    if (!h->mutable_vals) return fail(CVR_ERR_STATE, "cvr_update_values: the handle was created without cvr_options.mutable_values");
    if (!h->converted || !h->d_map) return fail(CVR_ERR_STATE, "cvr_update_values before cvr_preprocess");
    if (h->csr_kept) return fail(CVR_ERR_STATE, "cvr_update_values: the handle keeps its device CSR (keep_csr), whose values a later cvr_preprocess would convert again");
    return CVR_OK;
}

// after check_update
int update_device(cvr_handle *h, const void *vals, hipStream_t st)
{
    HIP_TRY(hipSetDevice(h->device));          // (the NULL stream means the current device's)
    HIP_TRY(handle_enter(h, st));
    HIP_TRY(cvr::launch_update_values(h->d_upd, (uint32_t)h->parts.size(), h->map_groups, h->vsz == 4, h->d_map, vals, st));
    HIP_TRY(handle_leave(h, st));
    return CVR_OK;
}

}  // namespace

extern "C" {

int cvr_update_values_supported(const cvr_handle *h) { return h && h->mutable_vals && h->converted && h->d_map && !h->csr_kept ? 1 : 0; }

int cvr_update_values_device(cvr_handle *h, const void *vals_dev, void *stream)
{
    const int rc = check_update(h, vals_dev);
    if (rc) return rc;
    return update_device(h, vals_dev, (hipStream_t)stream);
}

int cvr_update_values(cvr_handle *h, const void *vals_host)
{
    int rc = check_update(h, vals_host);
    if (rc) return rc;
    Range range("cvr_update_values (h2d, update)");
    HIP_TRY(hipSetDevice(h->device));
    const size_t bytes = h->vsz * (size_t)h->nvals;
    struct Mem { void *p = nullptr; ~Mem() { if (p) (void)hipFree(p); } } mem;
    HIP_TRY(hipMalloc(&mem.p, std::max<size_t>(bytes, 16)));
    if (bytes) HIP_TRY(hipMemcpyAsync(mem.p, vals_host, bytes, hipMemcpyHostToDevice, h->stream));
    rc = update_device(h, mem.p, h->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return CVR_OK;
}

}  // extern "C"
