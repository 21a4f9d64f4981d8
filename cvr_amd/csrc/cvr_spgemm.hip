// cvr_spgemm.hip -- the sparse matrix-matrix product C = A B on the device (include/cvr_amd.h: cvr_spgemm_*).
// One submission on the caller's stream: the bound pass (products per row of A, B's rows checked for strictly ascending columns), the rows binned
// into classes in row order, a symbolic kernel per LDS class that counts each row's distinct columns in a hash table, the scan to row_ptr, ONE read-back
// (nnz and the statistics), then a numeric kernel per class that fills the same tables with the sums and writes every row out sorted by column.
// Only when rows spill (products >= the block limit) is the arena of their tables allocated, sized by the largest row the read-back reported, and their
// symbolic kernel, the scan and a second read-back follow.
// The lanes that serve a row take ONE position p of A's row at a time and spread over B's row: B's rows hold no duplicates, so no two lanes touch
// one slot in a step, and a slot's additions happen in ascending p.  A slot is claimed by an integer compare-and-swap on its key; its value is
// updated by a plain read-add-write.  Where a key lands in a table may depend on timing: the sorted write-out removes that.  No kernel waits on
// another workgroup; the two single-workgroup passes (binning, scan) are ordered by the stream.
#include "cvr_internal.h"
#include "cvr_spgemm.h"

using namespace cvrh;
using namespace cvrh::spgemm;

struct cvr_spgemm {
    int         device = 0;
    int32_t     is_f32 = 0;
    int64_t     m = 0, k = 0, n = 0, nnz = 0, nnzb = 0;
    int64_t     a_j0 = 0, a_j1 = 0, b_j0 = 0, b_j1 = 0;
    int64_t     group_limit = kGroupLimit, block_limit = kBlockLimit;
    // device copies of the two patterns (row pointers as given; the column arrays are addressed with the views' own positions)
    long long  *d_arp = nullptr, *d_brp = nullptr;
    int32_t    *d_aci = nullptr, *d_bci = nullptr;
    long long  *d_products = nullptr, *d_rows = nullptr, *d_status = nullptr, *d_cnt = nullptr;
    // C
    long long  *d_crp = nullptr;
    int32_t    *d_cci = nullptr;
    void       *d_cva = nullptr;
    // the spill class's tables: `spill_wgs` of 2^spill_log2 slots each
    void       *d_arena = nullptr;
    int32_t     spill_wgs = 0, spill_log2 = 0;
    long long   status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double      symbolic_s = 0, numeric_s = 0;
};

namespace {

constexpr int       kThreads = 256;
constexpr int32_t   kEmpty = 0x7fffffff;          // above every column: B's ncols stays below 2^31 - 1
constexpr long long kNoRow = 0x7fffffffffffffffll;
// d_status: the lowest row of B that is not strictly ascending, the products' total and maximum, the rows of the four classes, nnz(C)
enum { kStBad = 0, kStProducts, kStMax, kStEmpty, kStGroup, kStBlock, kStSpill, kStNnz };

struct Args {
    const long long *arp, *brp;
    const int32_t   *aci, *bci;          // addressed with the views' positions
    const void      *ava, *bva;
    const long long *products, *rows, *status;
    long long       *crp, *cnt;          // cnt[i + 1]: the distinct columns of row i (the symbolic kernels write it, the scan reads it)
    int32_t         *cci;
    void            *cva;
    void            *arena;
    long long        n, nnzb;
    int32_t          spill_log2;
};

// ---- the bound pass -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) bound_kernel(const long long *arp, const int32_t *aci, const long long *brp, long long m, long long *products)
{
    for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < m; i += (long long)gridDim.x * kThreads) {
        long long s = 0;
        for (long long p = arp[i]; p < arp[i + 1]; p++) {
            const long long c = aci[p];
            s += brp[c + 1] - brp[c];
        }
        products[i] = s;
    }
}

__global__ void __launch_bounds__(kThreads) sorted_kernel(const long long *brp, const int32_t *bci, long long k, long long *status)
{
    for (long long r = blockIdx.x * (long long)kThreads + threadIdx.x; r < k; r += (long long)gridDim.x * kThreads) {
        bool bad = false;
        for (long long q = brp[r] + 1; q < brp[r + 1] && !bad; q++) bad = bci[q] <= bci[q - 1];
        if (bad) atomicMin(reinterpret_cast<unsigned long long *>(status + kStBad), (unsigned long long)r);
    }
}

// ---- one workgroup over the rows in contiguous pieces: the classes in row order, and the scan ----------------------------------------------
constexpr int kWide = 1024;

// exclusive scan of v over the workgroup's threads (in thread order); *total = the sum
__device__ long long block_exclusive(long long v, long long *lds, long long *total)
{
    const int t = threadIdx.x;
    __syncthreads();
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < kWide; d <<= 1) {
        const long long add = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    *total = lds[kWide - 1];
    return lds[t] - v;
}

__device__ inline int class_of(long long products, long long group_limit, long long block_limit)
{
    return products <= 0 ? 0 : products < group_limit ? 1 : products < block_limit ? 2 : 3;
}

__global__ void __launch_bounds__(kWide) bin_kernel(const long long *products, long long m, long long group_limit, long long block_limit, long long *rows, long long *status)
{
    __shared__ long long lds[kWide];
    const long long per = (m + kWide - 1) / kWide, r0 = std::min<long long>(m, per * threadIdx.x), r1 = std::min<long long>(m, r0 + per);
    long long cnt[4] = {0, 0, 0, 0}, sum = 0, mx = 0;
    for (long long i = r0; i < r1; i++) {
        const long long p = products[i];
        cnt[class_of(p, group_limit, block_limit)]++;
        sum += p;
        mx = p > mx ? p : mx;
    }
    long long at[4] = {0, 0, 0, 0}, tot[4] = {0, 0, 0, 0}, sum_all;
    for (int c = 0; c < 4; c++) at[c] = block_exclusive(cnt[c], lds, &tot[c]);
    (void)block_exclusive(sum, lds, &sum_all);
    // the maximum, by a tree over the same buffer
    __syncthreads();
    lds[threadIdx.x] = mx;
    __syncthreads();
    for (int d = kWide / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) lds[threadIdx.x] = lds[threadIdx.x] > lds[threadIdx.x + d] ? lds[threadIdx.x] : lds[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        status[kStProducts] = sum_all;
        status[kStMax] = lds[0];
        status[kStEmpty] = tot[0];
        status[kStGroup] = tot[1];
        status[kStBlock] = tot[2];
        status[kStSpill] = tot[3];
    }
    at[2] += tot[1];                    // the three lists one after the other: group, block, spill
    at[3] += tot[1] + tot[2];
    for (long long i = r0; i < r1; i++) {
        const int c = class_of(products[i], group_limit, block_limit);
        if (c) rows[at[c]++] = i;
    }
}

// cnt[1 .. m] holds the rows' counts: crp[i + 1] = their inclusive scan (crp[0] = 0 stays), nnz into the status
__global__ void __launch_bounds__(kWide) scan_kernel(const long long *cnt, long long *crp, long long m, long long *status)
{
    __shared__ long long lds[kWide];
    const long long per = (m + kWide - 1) / kWide, r0 = std::min<long long>(m, per * threadIdx.x), r1 = std::min<long long>(m, r0 + per);
    long long s = 0, total;
    for (long long i = r0; i < r1; i++) s += cnt[i + 1];
    long long run = block_exclusive(s, lds, &total);
    for (long long i = r0; i < r1; i++) {
        run += cnt[i + 1];
        crp[i + 1] = run;
    }
    if (threadIdx.x == 0) status[kStNnz] = total;
}

// ---- a row in a table -------------------------------------------------------------------------------------------------------------------------
// TS lanes serve the row: the whole workgroup (TS == kThreads: barriers), or kLanes lanes of a wavefront.  For those the order between two steps
// rests on an ASSUMPTION about the target, which holds on gfx950: the lanes of a wavefront share one program counter (no independent thread
// scheduling) and the compiler structurises control flow, so the wavefront leaves the divergent loop over q, and the probe loop inside it, only when
// every lane is through, and its LDS operations are carried out in program order.  __builtin_amdgcn_wave_barrier emits no instruction: it and the
// wavefront-scope fences only keep the COMPILER from moving a slot's accesses across a step.  A port to a target that schedules lanes independently, or
// a compiler that stops structurising, needs a real barrier here.
template <int TS>
__device__ inline void team_sync()
{
    if (TS == kThreads) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

__device__ inline int ceil_log2(unsigned long long x) { return x <= 1 ? 0 : 64 - __clzll(x - 1); }

// keys / vals: 2^log2s slots.  Symbolic: the row's distinct columns into crp[i + 1].  Numeric: the sums, then the row sorted into C.
template <typename T, bool NUMERIC, int TS>
__device__ void row_in_table(const Args &a, long long i, int lane, int32_t *keys, T *vals, int log2s, int *cnt)
{
    const size_t   S = (size_t)1 << log2s, mask = S - 1;
    const uint32_t shift = 32u - (uint32_t)log2s;
    for (size_t s = lane; s < S; s += TS) {
        keys[s] = kEmpty;
        if (NUMERIC) vals[s] = T(0);
    }
    if (!NUMERIC && lane == 0) *cnt = 0;
    team_sync<TS>();
    const T *av = static_cast<const T *>(a.ava), *bv = static_cast<const T *>(a.bva);
    for (long long p = a.arp[i]; p < a.arp[i + 1]; p++) {
        const long long c = a.aci[p];
        T x = T(0);
        if (NUMERIC) x = av[p];
        for (long long q = a.brp[c] + lane; q < a.brp[c + 1]; q += TS) {
            const int32_t j = a.bci[q];
            size_t        s = (size_t)(((uint32_t)j * 2654435761u) >> shift) & mask;
            for (;;) {
                const int32_t k = __atomic_load_n(&keys[s], __ATOMIC_RELAXED);
                if (k == j) break;
                if (k == kEmpty) {
                    const int32_t old = atomicCAS(&keys[s], kEmpty, j);
                    if (old == kEmpty) {
                        if (!NUMERIC) atomicAdd(cnt, 1);
                        break;
                    }
                    if (old == j) break;
                }
                s = (s + 1) & mask;
            }
            if (NUMERIC) {
                const T t = x * bv[q];
                vals[s] = vals[s] + t;
            }
        }
        team_sync<TS>();
    }
    if (!NUMERIC) {
        if (lane == 0) a.cnt[i + 1] = *cnt;
        team_sync<TS>();
        return;
    }
    // bitonic sort of the slots by key (the empty ones last)
    for (size_t kk = 2; kk <= S; kk <<= 1)
        for (size_t jj = kk >> 1; jj > 0; jj >>= 1) {
            for (size_t idx = lane; idx < S; idx += TS) {
                const size_t other = idx ^ jj;
                if (other > idx) {
                    const int32_t ka = keys[idx], kb = keys[other];
                    if ((ka > kb) == ((idx & kk) == 0)) {
                        keys[idx] = kb;
                        keys[other] = ka;
                        const T va = vals[idx];
                        vals[idx] = vals[other];
                        vals[other] = va;
                    }
                }
            }
            team_sync<TS>();
        }
    const long long base = a.crp[i], count = a.crp[i + 1] - base;
    T              *cv = static_cast<T *>(a.cva);
    for (long long t = lane; t < count && t < (long long)S; t += TS) {
        a.cci[base + t] = keys[t];
        cv[base + t] = vals[t];
    }
    team_sync<TS>();
}

// group rows: kLanes lanes per row, kThreads / kLanes rows per workgroup at a time, a table of kGroupSlots slots each
template <typename T, bool NUMERIC>
__global__ void __launch_bounds__(kThreads) group_kernel(Args a)
{
    constexpr int kTeams = kThreads / kLanes;
    __shared__ T       vals[kTeams][kGroupSlots];
    __shared__ int32_t keys[kTeams][kGroupSlots];
    __shared__ int     cnt[kTeams];
    const int          team = threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
    const long long    count = a.status[kStGroup];
    for (long long r = blockIdx.x * (long long)kTeams + team; r < count; r += (long long)gridDim.x * kTeams)
        row_in_table<T, NUMERIC, kLanes>(a, a.rows[r], lane, keys[team], vals[team], 6, &cnt[team]);
}

extern __shared__ __attribute__((aligned(16))) uint8_t spgemm_smem[];

// block rows: a workgroup per row at a time; the table has at least twice the row's products, at most kBlockSlots slots
template <typename T, bool NUMERIC>
__global__ void __launch_bounds__(kThreads) block_kernel(Args a)
{
    __shared__ int  cnt;
    T              *vals = reinterpret_cast<T *>(spgemm_smem);
    int32_t        *keys = reinterpret_cast<int32_t *>(spgemm_smem + sizeof(T) * (size_t)kBlockSlots);
    const long long first = a.status[kStGroup], count = a.status[kStBlock];
    for (long long r = blockIdx.x; r < count; r += gridDim.x) {
        const long long i = a.rows[first + r];
        int             log2s = ceil_log2(2ull * (unsigned long long)a.products[i]);
        log2s = log2s < 6 ? 6 : log2s > 13 ? 13 : log2s;
        row_in_table<T, NUMERIC, kThreads>(a, i, threadIdx.x, keys, vals, log2s, &cnt);
    }
}

// spill rows: a workgroup per row at a time, its table in the arena
template <typename T, bool NUMERIC>
__global__ void __launch_bounds__(kThreads) spill_kernel(Args a)
{
    __shared__ int  cnt;
    const size_t    cap = (size_t)1 << a.spill_log2;
    uint8_t        *mine = static_cast<uint8_t *>(a.arena) + (size_t)blockIdx.x * cap * (sizeof(T) + sizeof(int32_t));
    T              *vals = reinterpret_cast<T *>(mine);
    int32_t        *keys = reinterpret_cast<int32_t *>(mine + sizeof(T) * cap);
    const long long first = a.status[kStGroup] + a.status[kStBlock], count = a.status[kStSpill];
    for (long long r = blockIdx.x; r < count; r += gridDim.x) {
        const long long i = a.rows[first + r];
        long long       d = a.products[i];          // the row's distinct columns are at most this
        d = d < a.n ? d : a.n;
        d = d < a.nnzb ? d : a.nnzb;
        int log2s = ceil_log2(2ull * (unsigned long long)d);
        log2s = log2s < 6 ? 6 : log2s > a.spill_log2 ? a.spill_log2 : log2s;
        row_in_table<T, NUMERIC, kThreads>(a, i, threadIdx.x, keys, vals, log2s, &cnt);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
uint32_t grid_for(int64_t items, int64_t per_block, int64_t cap)
{
    const int64_t g = (items + per_block - 1) / per_block;
    return (uint32_t)std::max<int64_t>(1, std::min<int64_t>(g, cap));
}

// (on every launch: the attribute belongs to the current device's copy of the kernel, and the call is cheap)
template <typename T>
int set_block_lds(bool numeric)
{
    const int bytes = (int)((sizeof(T) + sizeof(int32_t)) * (size_t)kBlockSlots);
    if (numeric) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&block_kernel<T, true>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    else HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&block_kernel<T, false>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return CVR_OK;
}

Args args_of(const cvr_spgemm *g, const void *ava, const void *bva)
{
    Args a{};
    a.arp = g->d_arp;
    a.brp = g->d_brp;
    a.aci = g->d_aci - g->a_j0;
    a.bci = g->d_bci - g->b_j0;
    a.ava = ava;
    a.bva = bva;
    a.products = g->d_products;
    a.rows = g->d_rows;
    a.status = g->d_status;
    a.crp = g->d_crp;
    a.cnt = g->d_cnt;
    a.cci = g->d_cci;
    a.cva = g->d_cva;
    a.arena = g->d_arena;
    a.n = g->n;
    a.nnzb = g->nnzb;
    a.spill_log2 = g->spill_log2;
    return a;
}

// the kernels of the classes in `which` (1: group, 2: block, 4: spill); counts == nullptr: the classes' sizes are not known on the host yet
enum { kGroup = 1, kBlock = 2, kSpill = 4 };
template <typename T, bool NUMERIC>
int launch_classes(const cvr_spgemm *g, const Args &a, const long long *counts, int which, hipStream_t st)
{
    if (g->m == 0) return CVR_OK;
    if ((which & kGroup) && (!counts || counts[kStGroup] > 0)) {
        const int64_t rows = counts ? counts[kStGroup] : g->m;
        hipLaunchKernelGGL((group_kernel<T, NUMERIC>), dim3(grid_for(rows, kThreads / kLanes, 4096)), dim3(kThreads), 0, st, a);
    }
    if ((which & kBlock) && (!counts || counts[kStBlock] > 0)) {
        if (const int rc = set_block_lds<T>(NUMERIC)) return rc;
        const int64_t rows = counts ? counts[kStBlock] : g->m;
        const size_t  lds = (sizeof(T) + sizeof(int32_t)) * (size_t)kBlockSlots;
        hipLaunchKernelGGL((block_kernel<T, NUMERIC>), dim3(grid_for(rows, 1, 512)), dim3(kThreads), lds, st, a);
    }
    if ((which & kSpill) && (!counts || counts[kStSpill] > 0) && g->spill_wgs > 0) {
        const int64_t rows = counts ? counts[kStSpill] : g->m;
        hipLaunchKernelGGL((spill_kernel<T, NUMERIC>), dim3(grid_for(rows, 1, g->spill_wgs)), dim3(kThreads), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

int device_alloc(void **out, size_t bytes, const char *what)
{
    *out = nullptr;
    if (hipMalloc(out, bytes ? bytes : 16) != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        return fail(CVR_ERR_NOMEM, "cvr_spgemm_create: out of device memory for %s (%zu bytes)", what, bytes);
    }
    return CVR_OK;
}

// one view: checked as cvr_create checks a CSR (host arrays: check_view, cvr_spgemm_host's own; device arrays: the two kernels cvr_create uses, each
// with a small read-back), row pointers and columns copied into the object; *j0 / *j1 = row_ptr[0] / row_ptr[nrows]
int stage_view(const cvr_csr_view *v, long long **d_rp, int32_t **d_ci, int64_t *j0, int64_t *j1, hipStream_t st)
{
    *j0 = *j1 = 0;
    const hipMemcpyKind kind = v->arrays_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (!v->arrays_on_device) {
        if (const int rc = check_view(v)) return rc;
        if (v->nrows > 0) {
            *j0 = v->row_ptr[0];
            *j1 = v->row_ptr[v->nrows];
        }
    } else {
        if (v->ncols >= (int64_t)0x7fffffff) return fail(CVR_ERR_INVALID, "ncols (%lld) must stay below 2^31 - 1", (long long)v->ncols);
        if (v->nrows > 0 && !v->row_ptr) return fail(CVR_ERR_INVALID, "row_ptr is null");
        if (const int rc = check_rows_device(v->row_ptr, v->nrows, j0, j1)) return rc;
        if (*j1 > *j0 && (!v->col_idx || !v->vals)) return fail(CVR_ERR_INVALID, "col_idx / vals is null");
        if (const int rc = check_columns_device(v->col_idx, *j0, *j1, v->ncols)) return rc;
    }
    if (const int rc = device_alloc(reinterpret_cast<void **>(d_rp), sizeof(long long) * (size_t)(v->nrows + 1), "row_ptr")) return rc;
    if (const int rc = device_alloc(reinterpret_cast<void **>(d_ci), sizeof(int32_t) * (size_t)(*j1 - *j0), "col_idx")) return rc;
    if (v->nrows > 0) HIP_TRY(hipMemcpyAsync(*d_rp, v->row_ptr, sizeof(long long) * (size_t)(v->nrows + 1), kind, st));
    else HIP_TRY(hipMemsetAsync(*d_rp, 0, sizeof(long long), st));
    if (*j1 > *j0) HIP_TRY(hipMemcpyAsync(*d_ci, v->col_idx + *j0, sizeof(int32_t) * (size_t)(*j1 - *j0), kind, st));
    return CVR_OK;
}

void read_limits(cvr_spgemm *g)
{
    g->group_limit = kGroupLimit;
    g->block_limit = kBlockLimit;
    if (const char *e = cvr::debug_env("spgemm_limits")) {          // lowers the limits: a few hundred entries reach the block and the spill class
        char           *end = nullptr;
        const long long a = strtoll(e, &end, 10), b = end && *end == ':' ? strtoll(end + 1, nullptr, 10) : 0;
        if (a >= 1) g->group_limit = std::min<long long>(a, kGroupLimit);
        if (b >= 1) g->block_limit = std::min<long long>(b, kBlockLimit);
        g->block_limit = std::max(g->block_limit, g->group_limit);
    }
}

int build(cvr_spgemm *g, const cvr_csr_view *a, const cvr_csr_view *b, hipStream_t st)
{
    const double t0 = now_s();
    const size_t vsz = g->is_f32 ? 4 : 8;
    if (const int rc = stage_view(a, &g->d_arp, &g->d_aci, &g->a_j0, &g->a_j1, st)) return rc;
    if (const int rc = stage_view(b, &g->d_brp, &g->d_bci, &g->b_j0, &g->b_j1, st)) return rc;
    g->nnzb = g->b_j1 - g->b_j0;
    // the values: the caller's device arrays, or copies for the length of this call
    struct Tmp {
        void *p = nullptr;
        ~Tmp() { if (p) (void)hipFree(p); }
    } ta, tb;
    const void *ava = a->vals, *bva = b->vals;
    if (!a->arrays_on_device) {
        if (const int rc = device_alloc(&ta.p, vsz * (size_t)(g->a_j1 - g->a_j0), "A's values")) return rc;
        if (g->a_j1 > g->a_j0) HIP_TRY(hipMemcpyAsync(ta.p, static_cast<const uint8_t *>(a->vals) + vsz * (size_t)g->a_j0, vsz * (size_t)(g->a_j1 - g->a_j0), hipMemcpyHostToDevice, st));
        ava = static_cast<const uint8_t *>(ta.p) - vsz * (size_t)g->a_j0;
    }
    if (!b->arrays_on_device) {
        if (const int rc = device_alloc(&tb.p, vsz * (size_t)g->nnzb, "B's values")) return rc;
        if (g->nnzb > 0) HIP_TRY(hipMemcpyAsync(tb.p, static_cast<const uint8_t *>(b->vals) + vsz * (size_t)g->b_j0, vsz * (size_t)g->nnzb, hipMemcpyHostToDevice, st));
        bva = static_cast<const uint8_t *>(tb.p) - vsz * (size_t)g->b_j0;
    }
    const int64_t m = g->m;
    if (const int rc = device_alloc(reinterpret_cast<void **>(&g->d_products), sizeof(long long) * (size_t)m, "the products")) return rc;
    if (const int rc = device_alloc(reinterpret_cast<void **>(&g->d_rows), sizeof(long long) * (size_t)m, "the row lists")) return rc;
    if (const int rc = device_alloc(reinterpret_cast<void **>(&g->d_status), sizeof(g->status), "the status words")) return rc;
    if (const int rc = device_alloc(reinterpret_cast<void **>(&g->d_crp), sizeof(long long) * (size_t)(m + 1), "C's row_ptr")) return rc;
    if (const int rc = device_alloc(reinterpret_cast<void **>(&g->d_cnt), sizeof(long long) * (size_t)(m + 1), "the rows' counts")) return rc;
    g->status[kStBad] = kNoRow;
    HIP_TRY(hipMemcpyAsync(g->d_status, g->status, sizeof(g->status), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(g->d_crp, 0, sizeof(long long) * (size_t)(m + 1), st));
    HIP_TRY(hipMemsetAsync(g->d_cnt, 0, sizeof(long long) * (size_t)(m + 1), st));
    Args args = args_of(g, ava, bva);
    if (g->k > 0) hipLaunchKernelGGL(sorted_kernel, dim3(grid_for(g->k, kThreads, 4096)), dim3(kThreads), 0, st, (const long long *)g->d_brp, args.bci, (long long)g->k, g->d_status);
    if (m > 0) {
        hipLaunchKernelGGL(bound_kernel, dim3(grid_for(m, kThreads, 4096)), dim3(kThreads), 0, st, (const long long *)g->d_arp, args.aci, (const long long *)g->d_brp, (long long)m, g->d_products);
        hipLaunchKernelGGL(bin_kernel, dim3(1), dim3(kWide), 0, st, (const long long *)g->d_products, (long long)m, (long long)g->group_limit, (long long)g->block_limit, g->d_rows, g->d_status);
        HIP_TRY(hipGetLastError());
        if (g->nnzb > 0 && g->a_j1 > g->a_j0) {
            if (const int rc = g->is_f32 ? launch_classes<float, false>(g, args, nullptr, kGroup | kBlock, st) : launch_classes<double, false>(g, args, nullptr, kGroup | kBlock, st)) return rc;
            hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kWide), 0, st, (const long long *)g->d_cnt, g->d_crp, (long long)m, g->d_status);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(g->status, g->d_status, sizeof(g->status), hipMemcpyDeviceToHost, st));          // the one read-back
    HIP_TRY(hipStreamSynchronize(st));
    if (g->status[kStBad] != kNoRow) return fail_unsorted("cvr_spgemm_create", g->status[kStBad]);
    if (g->status[kStSpill] > 0) {
        // Rows spill: only now is the arena of their tables allocated -- a table holds twice the most distinct columns the largest row can have, as
        // many tables as fit 256 MiB (at most 256, at least one) -- and their symbolic kernel, the scan and a second read-back follow
        const int64_t most = std::max<int64_t>(1, std::min<int64_t>(g->status[kStMax], std::min<int64_t>(g->n, g->nnzb)));
        int           lg = 6;
        while (((int64_t)1 << lg) < 2 * most) lg++;
        if (lg > 31) return fail(CVR_ERR_NOMEM, "cvr_spgemm_create: a row of %lld products needs a table of 2^%d slots", (long long)g->status[kStMax], lg);
        g->spill_log2 = lg;
        const size_t table = ((size_t)1 << lg) * (vsz + sizeof(int32_t));
        g->spill_wgs = (int32_t)std::max<size_t>(1, std::min<size_t>((size_t)std::min<int64_t>(256, g->status[kStSpill]), ((size_t)256 << 20) / table));
        if (const int rc = device_alloc(&g->d_arena, table * (size_t)g->spill_wgs, "the spill arena")) return rc;
        args = args_of(g, ava, bva);
        if (const int rc = g->is_f32 ? launch_classes<float, false>(g, args, g->status, kSpill, st) : launch_classes<double, false>(g, args, g->status, kSpill, st)) return rc;
        hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kWide), 0, st, (const long long *)g->d_cnt, g->d_crp, (long long)m, g->d_status);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(g->status, g->d_status, sizeof(g->status), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    (void)hipFree(g->d_cnt);
    g->d_cnt = nullptr;
    g->nnz = g->status[kStNnz];
    g->symbolic_s = now_s() - t0;
    const double t1 = now_s();
    if (const int rc = device_alloc(reinterpret_cast<void **>(&g->d_cci), sizeof(int32_t) * (size_t)g->nnz, "C's col_idx")) return rc;
    if (const int rc = device_alloc(&g->d_cva, vsz * (size_t)g->nnz, "C's values")) return rc;
    args = args_of(g, ava, bva);
    if (g->nnz > 0)
        if (const int rc = g->is_f32 ? launch_classes<float, true>(g, args, g->status, kGroup | kBlock | kSpill, st) : launch_classes<double, true>(g, args, g->status, kGroup | kBlock | kSpill, st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));          // (the copies of host values are released behind this)
    g->numeric_s = now_s() - t1;
    return CVR_OK;
}

void release(cvr_spgemm *g)
{
    for (void *p : {(void *)g->d_arp, (void *)g->d_brp, (void *)g->d_aci, (void *)g->d_bci, (void *)g->d_products, (void *)g->d_rows, (void *)g->d_status, (void *)g->d_cnt, (void *)g->d_crp, (void *)g->d_cci,
                    g->d_cva, g->d_arena})
        if (p) (void)hipFree(p);
    delete g;
}

}  // namespace

extern "C" {

int cvr_spgemm_create(cvr_spgemm **out, const cvr_csr_view *a, const cvr_csr_view *b, int32_t device, void *stream)
{
    if (!out || !a || !b) return fail(CVR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (const int rc = check_pair(a, b, "cvr_spgemm_create")) return rc;
    if ((a->arrays_on_device != 0) != (b->arrays_on_device != 0)) return fail(CVR_ERR_INVALID, "cvr_spgemm_create: A and B must both be host arrays or both be arrays of device %d", device);
    if (device < 0 || device >= cvr_device_count()) return fail(CVR_ERR_NO_DEVICE, "device %d of %d", device, cvr_device_count());
    cvr::debug_refresh();
    Range range("cvr_spgemm_create");
    HIP_TRY(hipSetDevice(device));
    cvr_spgemm *g = new (std::nothrow) cvr_spgemm;
    if (!g) return fail(CVR_ERR_NOMEM, "out of host memory");
    g->device = device;
    g->is_f32 = a->is_f32 ? 1 : 0;
    g->m = a->nrows;
    g->k = a->ncols;
    g->n = b->ncols;
    read_limits(g);
    if (const int rc = build(g, a, b, (hipStream_t)stream)) {
        (void)hipStreamSynchronize((hipStream_t)stream);
        release(g);
        return rc;
    }
    *out = g;
    return CVR_OK;
}

int cvr_spgemm_get_info(const cvr_spgemm *g, cvr_spgemm_info_t *info)
{
    if (!g || !info) return fail(CVR_ERR_INVALID, "null argument");
    memset(info, 0, sizeof(*info));
    info->nrows = g->m;
    info->ncols = g->n;
    info->inner = g->k;
    info->nnz = g->nnz;
    info->products = g->status[kStProducts];
    info->max_row_products = g->status[kStMax];
    info->rows_empty = g->status[kStEmpty];
    info->rows_group = g->status[kStGroup];
    info->rows_block = g->status[kStBlock];
    info->rows_spill = g->status[kStSpill];
    info->group_limit = g->group_limit;
    info->block_limit = g->block_limit;
    info->is_f32 = g->is_f32;
    info->lanes_per_row = kLanes;
    info->symbolic_s = g->symbolic_s;
    info->numeric_s = g->numeric_s;
    return CVR_OK;
}

int cvr_spgemm_csr_device(const cvr_spgemm *g, cvr_csr_view *c)
{
    if (!g || !c) return fail(CVR_ERR_INVALID, "null argument");
    memset(c, 0, sizeof(*c));
    c->nrows = g->m;
    c->ncols = g->n;
    c->row_ptr = reinterpret_cast<const int64_t *>(g->d_crp);
    c->col_idx = g->d_cci;
    c->vals = g->d_cva;
    c->is_f32 = g->is_f32;
    c->arrays_on_device = 1;
    return CVR_OK;
}

int cvr_spgemm_export(const cvr_spgemm *g, int64_t *row_ptr, int32_t *col_idx, void *vals)
{
    if (!g) return fail(CVR_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipDeviceSynchronize());          // (a numeric re-run may be in flight on any stream)
    if (row_ptr) HIP_TRY(hipMemcpy(row_ptr, g->d_crp, sizeof(int64_t) * (size_t)(g->m + 1), hipMemcpyDeviceToHost));
    if (col_idx && g->nnz > 0) HIP_TRY(hipMemcpy(col_idx, g->d_cci, sizeof(int32_t) * (size_t)g->nnz, hipMemcpyDeviceToHost));
    if (vals && g->nnz > 0) HIP_TRY(hipMemcpy(vals, g->d_cva, (g->is_f32 ? 4 : 8) * (size_t)g->nnz, hipMemcpyDeviceToHost));
    return CVR_OK;
}

int cvr_spgemm_numeric_device(cvr_spgemm *g, const void *a_vals_dev, const void *b_vals_dev, void *stream)
{
    if (!g) return fail(CVR_ERR_INVALID, "null argument");
    if ((g->a_j1 > g->a_j0 && !a_vals_dev) || (g->nnzb > 0 && !b_vals_dev)) return fail(CVR_ERR_INVALID, "cvr_spgemm_numeric_device: null value array");
    if (g->nnz == 0) return CVR_OK;
    Range range("cvr_spgemm_numeric_device");
    HIP_TRY(hipSetDevice(g->device));
    const Args args = args_of(g, a_vals_dev, b_vals_dev);
    return g->is_f32 ? launch_classes<float, true>(g, args, g->status, kGroup | kBlock | kSpill, (hipStream_t)stream) : launch_classes<double, true>(g, args, g->status, kGroup | kBlock | kSpill, (hipStream_t)stream);
}

int cvr_spgemm_destroy(cvr_spgemm *g)
{
    if (!g) return CVR_OK;
    (void)hipSetDevice(g->device);
    (void)hipDeviceSynchronize();
    release(g);
    return CVR_OK;
}

}  // extern "C"
