// cvr_ilu0.hip -- the ILU(0) preconditioner, the third kind of cvr_precond (include/cvr_amd.h: cvr_precond_ilu0, cvr_precond_ilu0_info,
// cvr_precond_ilu0_export, cvr_ilu0_levels_host; cvr_precond_ilu0_jacobi, cvr_precond_ilu0_jacobi_info: the Jacobi-swept apply, below).  A ~ L U on A's own pattern, L unit lower and U upper triangular; z = U^-1 L^-1 r is two sparse
// triangular solves, each scheduled by levels: a row's level is one more than the largest level among the rows it reads, so the rows of a level are
// independent and the levels run in order.
//   Analysis, on the host, once, O(nnz): the checks (square, columns strictly increasing, a diagonal in every row), the level of every row in L
//     (from row 0 on, over the entries left of the diagonal) and in U (from the last row back, over the entries right of it), the rows ordered by
//     (level, row), and per sweep the launch plan: a level of at least `wide_threshold` rows is a launch of its own over all its rows
//     (sweep_wide_kernel); a run of consecutive narrower levels is ONE launch of ONE workgroup that walks them in order with __syncthreads() between
//     them (sweep_merged_kernel).  No kernel waits on another workgroup: no flag, no spinning, no cooperative grid.
//   Factorisation, on the device, on L's plan (row i needs exactly the rows its left-of-diagonal columns name), on an fp64 copy of the values, one
//     thread per row: for k < i of the row in column order a_ik = a_ik / a_kk, then a_ij = a_ij - a_ik a_kj for the j > k of row k that row i has (a
//     merge of two ascending rows).  Every operation is rounded on its own, every a_ij has one update order; rounded once to T at the end.  The lowest
//     row whose pivot is zero or not finite comes back in a device word (atomicMin).
//   Apply: G = lanes_per_row lanes per row (a power of two, 1 .. 64, groups inside a wavefront).  Lane l adds double(f_ij) * double(v_j) over the
//     row's entries l, l + G, .. of the sweep's triangle from +0, the lanes are combined by the xor butterfly G/2 .. 1, then
//     y_i = T(double(r_i) - s) in L's sweep and z_i = T((double(y_i) - s) / double(u_ii)) in U's.  y is a buffer of the object.
//   In the merged kernels the vector being solved for is read and written in the same launch by different wavefronts of the workgroup: those loads
//   are agent-scope atomic loads (they bypass the CU's vector L1), never const __restrict__; the stores are complete before the barrier.
// The same device function forms a row in both kernels, so the bits do not depend on the plan.
//   The Jacobi-swept object (cvr_precond_ilu0_jacobi, Ilu0::sweeps = s >= 1): the same analysis, factors and row sum (row_sum), but each exact
//   sweep is replaced by s Jacobi sweeps on its triangular system, 2 s launches per apply whatever the levels.  A launch (jacobi_sweep_kernel) covers
//   all n rows in natural order through a row-ordered slot array (cvr_ilu0_slots.h), reads one buffer and writes another -- never in place -- so the
//   read side was written by an earlier launch: plain const __restrict__ loads, no barrier, nothing waits on another workgroup.
//     L: y(0) = r, read in place;  y(k)_i = T(double(r_i) - S_i(y(k-1))), k = 1 .. s, alternating between two buffers of the object;
//        the last L launch also writes z(0)_i = T(double(y(s)_i) / double(u_ii)) for the row it has just formed.
//     U: z(k)_i = T((double(y(s)_i) - S'_i(z(k-1))) / double(u_ii)), k = 1 .. s, alternating between the caller's z and a third buffer of the object,
//        z(k) in the caller's z when s - k is even: z(s) lands there for odd and even s.
//   ilu0_apply is the one place that switches on `sweeps`; the solvers see kind 2 and nothing else.
// (The reference has no solver and no preconditioner: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_cg_kernels.h"
#include "cvr_precond.h"
#include "cvr_ilu0_slots.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace cvrh {
namespace krylov {

struct Ilu0Launch {
    int32_t lvl0, nlvl;          // the levels it covers
    int32_t slot0, nslots;       // ... and their rows in the sweep's order
    bool    merged;
};

struct Ilu0Sweep {
    Ilu0Slot               *d_slots = nullptr;          // n, by (level, row)
    int32_t                *d_lptr = nullptr;           // levels + 1: where each level begins in d_slots
    int32_t                 levels = 0, max_width = 0;
    std::vector<Ilu0Launch> plan;
};

struct Ilu0 {
    int64_t   nnz = 0;
    int32_t   G = 1, wide = 0;
    int32_t  *d_ci = nullptr;
    void     *d_f = nullptr;          // nnz values of T in the CSR's positions: L strictly below the diagonal, U from the diagonal up
    void     *d_y = nullptr;          // n values of T
    Ilu0Sweep lo, up;
    // the Jacobi-swept object only (sweeps >= 1; 0: the exact object, which has none of these)
    int32_t   sweeps = 0;
    Ilu0Slot *d_rows_lo = nullptr, *d_rows_up = nullptr;          // n each, in natural row order
    void     *d_y2 = nullptr, *d_w = nullptr;                     // n values of T each: y's second buffer (sweeps >= 2), z's other buffer
};

}  // namespace krylov
}  // namespace cvrh

namespace {

constexpr int     kMergedThreads = 1024;          // the one workgroup of a merged launch
constexpr int32_t kDefaultWide = 512;             // measured with tools/ilu_probe.py
constexpr int32_t kNoRow = 0x7fffffff;

// ---- the device half

// a value another wavefront of this workgroup may have stored in this launch: from L2, not from the CU's vector L1
__device__ __forceinline__ double load_coherent(const double *p)
{
    return __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ float load_coherent(const float *p)
{
    return __builtin_bit_cast(float, __hip_atomic_load(reinterpret_cast<const unsigned int *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
template <bool COH, typename V>
__device__ __forceinline__ V load_solved(const V *p)
{
    if constexpr (COH) return load_coherent(p);
    else return *p;
}

// the same in every thread of the launch
__device__ __forceinline__ bool gate_closed(const Ilu0Gate &g)
{
    for (int i = 0; i < g.nstop; i++)
        if (g.stop[i]) return true;
    if (g.owed) {
        const int q = g.owed[0], at = g.owed[1];
        if (q <= 0 || at <= g.lo || at > g.hi) return true;
    }
    return false;
}

// The sum of one row of a triangle over v by the G lanes of its group (lane l of them; every lane of the wavefront comes here, `active` or not: the
// butterfly is the whole wavefront's): the same value in all G lanes.  The exact and the Jacobi sweeps both form their rows with it.
template <bool COH, typename T, typename V>
__device__ __forceinline__ double row_sum(bool active, const Ilu0Slot &s, int l, int G, const int32_t *__restrict__ ci, const T *__restrict__ f, const V *v)
{
    double acc = 0;
    if (active)
        for (int e = l; e < s.cnt; e += G) {
            const long long q = s.beg + e;
            acc += (double)f[q] * (double)load_solved<COH>(v + ci[q]);
        }
    for (int o = G >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    return acc;
}

// One row of an exact sweep.  v: the vector being solved for (y in L's sweep, z in U's), rhs: r or y.
template <typename T, typename R, bool UPPER, bool COH>
__device__ __forceinline__ void sweep_row(bool active, const Ilu0Slot &s, int l, int G, const int32_t *__restrict__ ci, const T *__restrict__ f, const R *rhs, T *v)
{
    const double acc = row_sum<COH>(active, s, l, G, ci, f, (const T *)v);
    if (active && l == 0) {
        double t = (double)rhs[s.row] - acc;
        if constexpr (UPPER) t = t / (double)f[s.beg - 1];
        v[s.row] = (T)t;
    }
}

// a level of its own: slots slot0 .. slot0 + nslots - 1, G lanes each
template <typename T, typename R, bool UPPER>
__global__ __launch_bounds__(kThreads) void sweep_wide_kernel(const Ilu0Slot *__restrict__ slots, int slot0, int nslots, int G, const int32_t *__restrict__ ci,
                                                              const T *__restrict__ f, const R *rhs, T *v, Ilu0Gate gate)
{
    if (gate_closed(gate)) return;
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long k = t / G;
    const bool      active = k < nslots;
    Ilu0Slot        s{0, 0, 0};
    if (active) s = slots[slot0 + k];
    sweep_row<T, R, UPPER, false>(active, s, (int)(t - k * G), G, ci, f, rhs, v);
}

// a run of narrow levels lvl0 .. lvl0 + nlvl - 1 by one workgroup, a barrier behind each level.  Every loop bound is the workgroup's.
template <typename T, typename R, bool UPPER>
__global__ __launch_bounds__(kMergedThreads) void sweep_merged_kernel(const Ilu0Slot *__restrict__ slots, const int32_t *__restrict__ lptr, int lvl0, int nlvl, int G,
                                                                      const int32_t *__restrict__ ci, const T *__restrict__ f, const R *rhs, T *v, Ilu0Gate gate)
{
    if (gate_closed(gate)) return;
    const int per = kMergedThreads / G, k = threadIdx.x / G, l = threadIdx.x - k * G;
    for (int lv = lvl0; lv < lvl0 + nlvl; lv++) {
        const int a = lptr[lv], b = lptr[lv + 1];
        for (int base = a; base < b; base += per) {
            const bool active = base + k < b;
            Ilu0Slot   s{0, 0, 0};
            if (active) s = slots[base + k];
            sweep_row<T, R, UPPER, true>(active, s, l, G, ci, f, rhs, v);
        }
        __syncthreads();          // (with its fence: the level's stores are complete before any wavefront reads them)
    }
}

// One Jacobi sweep over all n rows in natural order (slots[i] is row i), G lanes a row: out_i from `in` of the launch before, never in place.
//   L (UPPER false): out_i = T(double(rhs_i) - S_i(in)); rhs is r, and so is `in` in the first sweep (V = R).  Z0: the last L sweep, which also writes
//     z0_i = T(double(out_i) / double(u_ii)), the diagonal lying behind the row's part of L.
//   U (UPPER true):  out_i = T((double(rhs_i) - S'_i(in)) / double(u_ii)); rhs is y(s).
// `in` and `rhs` were written before this launch and are only read (they may be the same array); out and z0 are other arrays.
template <typename T, typename V, typename R, bool UPPER, bool Z0>
__global__ __launch_bounds__(kThreads) void jacobi_sweep_kernel(const Ilu0Slot *__restrict__ slots, long long n, int G, const int32_t *__restrict__ ci, const T *__restrict__ f,
                                                                const R *rhs, const V *in, T *__restrict__ out, T *__restrict__ z0, Ilu0Gate gate)
{
    if (gate_closed(gate)) return;
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long i = t / G;
    const int       l = (int)(t - i * G);
    const bool      active = i < n;
    Ilu0Slot        s{0, 0, 0};
    if (active) s = slots[i];
    const double acc = row_sum<false>(active, s, l, G, ci, f, in);
    if (active && l == 0) {
        double v = (double)rhs[i] - acc;
        if constexpr (UPPER) v = v / (double)f[s.beg - 1];
        const T y = (T)v;
        out[i] = y;
        if constexpr (Z0) z0[i] = (T)((double)y / (double)f[s.beg + s.cnt]);
    }
}

// Row i of the factorisation, one thread: a holds the fp64 values in the CSR's positions
template <bool COH>
__device__ __forceinline__ void factor_row(int i, const int64_t *__restrict__ rp, const int64_t *__restrict__ dpos, const int32_t *__restrict__ ci, double *a, int32_t *bad)
{
    const long long b = rp[i], d = dpos[i], e = rp[i + 1];
    for (long long q = b; q < d; q++) {
        const int       k = ci[q];
        const long long dk = dpos[k], ek = rp[k + 1];
        const double    aik = a[q] / load_solved<COH>(a + dk);
        a[q] = aik;
        long long pi = q + 1;
        for (long long pk = dk + 1; pk < ek && pi < e; pk++) {
            const int j = ci[pk];
            while (pi < e && ci[pi] < j) pi++;
            if (pi < e && ci[pi] == j) a[pi] = a[pi] - aik * load_solved<COH>(a + pk);
        }
    }
    const double piv = a[d];
    if (!usable(piv)) atomicMin(bad, i);
}

__global__ __launch_bounds__(kThreads) void factor_wide_kernel(const Ilu0Slot *__restrict__ slots, int slot0, int nslots, const int64_t *__restrict__ rp,
                                                               const int64_t *__restrict__ dpos, const int32_t *__restrict__ ci, double *a, int32_t *bad)
{
    const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (k < nslots) factor_row<false>(slots[slot0 + k].row, rp, dpos, ci, a, bad);
}

__global__ __launch_bounds__(kMergedThreads) void factor_merged_kernel(const Ilu0Slot *__restrict__ slots, const int32_t *__restrict__ lptr, int lvl0, int nlvl,
                                                                       const int64_t *__restrict__ rp, const int64_t *__restrict__ dpos, const int32_t *__restrict__ ci,
                                                                       double *a, int32_t *bad)
{
    for (int lv = lvl0; lv < lvl0 + nlvl; lv++) {
        const int lo = lptr[lv], hi = lptr[lv + 1];
        for (int k = lo + (int)threadIdx.x; k < hi; k += kMergedThreads) factor_row<true>(slots[k].row, rp, dpos, ci, a, bad);
        __syncthreads();
    }
}

// the fp64 copy, and the factors rounded once to T
template <typename T>
__global__ __launch_bounds__(kThreads) void widen_kernel(const T *__restrict__ va, double *__restrict__ a, long long nnz)
{
    for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < nnz; q += (long long)kBlocks * kThreads) a[q] = (double)va[q];
}
template <typename T>
__global__ __launch_bounds__(kThreads) void round_kernel(const double *__restrict__ a, T *__restrict__ f, long long nnz)
{
    for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < nnz; q += (long long)kBlocks * kThreads) f[q] = (T)a[q];
}

// GMRES's x from M^-1 u, behind the sweeps and under their gate: x_i = T(double(x_i) + double(zu_i)).  AL: x, the caller's array, is 16-byte aligned.
template <typename T, bool AL>
__global__ __launch_bounds__(kThreads) void ilu0_xadd_kernel(T *__restrict__ x, const T *__restrict__ zu, long long n, Ilu0Gate gate)
{
    if (gate_closed(gate)) return;
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T xv[kPack<T>], zv[kPack<T>];
        load_pack<T, AL>(x, e, (int)cnt, xv);
        load_pack<T, true>(zu, e, (int)cnt, zv);
#pragma unroll
        for (int l = 0; l < kPack<T>; l++) xv[l] = (T)((double)xv[l] + (double)zv[l]);
        store_pack<T, AL>(x, e, (int)cnt, xv);
    }
}

// ---- the host half

// one sweep enqueued by its plan
template <typename T, typename R, bool UPPER>
int enqueue_sweep(const Ilu0 *u, const Ilu0Sweep &sw, const R *rhs, T *v, const Ilu0Gate &gate, hipStream_t st)
{
    const T *f = static_cast<const T *>(u->d_f);
    for (const Ilu0Launch &ln : sw.plan) {
        if (ln.merged) {
            hipLaunchKernelGGL((sweep_merged_kernel<T, R, UPPER>), dim3(1), dim3(kMergedThreads), 0, st, (const Ilu0Slot *)sw.d_slots, (const int32_t *)sw.d_lptr, (int)ln.lvl0, (int)ln.nlvl,
                               (int)u->G, (const int32_t *)u->d_ci, f, rhs, v, gate);
        } else {
            const long long groups = ((long long)ln.nslots * u->G + kThreads - 1) / kThreads;
            hipLaunchKernelGGL((sweep_wide_kernel<T, R, UPPER>), dim3((unsigned)groups), dim3(kThreads), 0, st, (const Ilu0Slot *)sw.d_slots, (int)ln.slot0, (int)ln.nslots, (int)u->G,
                               (const int32_t *)u->d_ci, f, rhs, v, gate);
        }
    }
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

// one Jacobi sweep enqueued: all n rows, G lanes each
template <typename T, typename V, typename R, bool UPPER, bool Z0>
void enqueue_jacobi(const Ilu0 *u, long long n, const R *rhs, const V *in, T *out, T *z0, const Ilu0Gate &gate, hipStream_t st)
{
    const long long groups = (n * u->G + kThreads - 1) / kThreads;
    hipLaunchKernelGGL((jacobi_sweep_kernel<T, V, R, UPPER, Z0>), dim3((unsigned)groups), dim3(kThreads), 0, st, (const Ilu0Slot *)(UPPER ? u->d_rows_up : u->d_rows_lo), n, (int)u->G,
                       (const int32_t *)u->d_ci, static_cast<const T *>(u->d_f), rhs, in, out, z0, gate);
}

// The swept apply: 2 * sweeps launches.  y(k) lies in the object's y buffer k & 1, z(k) in the caller's z when sweeps - k is even, else in w.
template <typename T, typename R>
int jacobi_apply(const Ilu0 *u, long long n, const R *r, T *z, const Ilu0Gate &gate, hipStream_t st)
{
    const int s = u->sweeps;
    T        *yb[2] = {static_cast<T *>(u->d_y2), static_cast<T *>(u->d_y)}, *w = static_cast<T *>(u->d_w);
    const auto zbuf = [&](int k) { return (s - k) % 2 == 0 ? z : w; };
    if (s == 1) enqueue_jacobi<T, R, R, false, true>(u, n, r, r, yb[1], zbuf(0), gate, st);
    else {
        enqueue_jacobi<T, R, R, false, false>(u, n, r, r, yb[1], (T *)nullptr, gate, st);
        for (int k = 2; k < s; k++) enqueue_jacobi<T, T, R, false, false>(u, n, r, (const T *)yb[(k - 1) & 1], yb[k & 1], (T *)nullptr, gate, st);
        enqueue_jacobi<T, T, R, false, true>(u, n, r, (const T *)yb[(s - 1) & 1], yb[s & 1], zbuf(0), gate, st);
    }
    for (int k = 1; k <= s; k++) enqueue_jacobi<T, T, T, true, false>(u, n, (const T *)yb[s & 1], (const T *)zbuf(k - 1), zbuf(k), (T *)nullptr, gate, st);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

// The structure checks and the two level arrays (n values each); dpos (n, may be null): where each row's diagonal lies.  O(nnz).
int analyse(int64_t n, const int64_t *rp, const int32_t *ci, const char *entry, int32_t *lvl_lo, int32_t *lvl_up, int64_t *dpos, int32_t *n_lo, int32_t *n_up)
{
    int32_t nl = 0, nu = 0;
    for (int64_t i = 0; i < n; i++) {
        int64_t d = -1, prev = -1;
        int32_t lv = 0;
        for (int64_t q = rp[i]; q < rp[i + 1]; q++) {
            const int64_t c = ci[q];
            if (c <= prev) return fail(CVR_ERR_INVALID, "%s: row %lld: the columns are not strictly increasing (%lld behind %lld)", entry, (long long)i, (long long)c, (long long)prev);
            prev = c;
            if (c == i) d = q;
            else if (c < i) lv = std::max(lv, lvl_lo[c] + 1);
        }
        if (d < 0) return fail(CVR_ERR_INVALID, "%s: row %lld has no diagonal entry", entry, (long long)i);
        if (dpos) dpos[i] = d;
        lvl_lo[i] = lv;
        nl = std::max(nl, lv + 1);
    }
    for (int64_t i = n - 1; i >= 0; i--) {
        int32_t lv = 0;
        for (int64_t q = rp[i + 1] - 1; q >= rp[i] && ci[q] > i; q--) lv = std::max(lv, lvl_up[ci[q]] + 1);
        lvl_up[i] = lv;
        nu = std::max(nu, lv + 1);
    }
    *n_lo = nl;
    *n_up = nu;
    return CVR_OK;
}

// the rows by (level, row) and the launch plan of one sweep
void plan_sweep(int64_t n, const int32_t *lvl, int32_t levels, int32_t wide, std::vector<int32_t> &order, std::vector<int32_t> &lptr, Ilu0Sweep &sw)
{
    lptr.assign((size_t)levels + 1, 0);
    for (int64_t i = 0; i < n; i++) lptr[(size_t)lvl[i] + 1]++;
    for (int32_t l = 0; l < levels; l++) lptr[(size_t)l + 1] += lptr[(size_t)l];
    order.assign((size_t)n, 0);
    std::vector<int32_t> at(lptr.begin(), lptr.end() - 1);
    for (int64_t i = 0; i < n; i++) order[(size_t)at[(size_t)lvl[i]]++] = (int32_t)i;          // ascending rows within a level
    sw.levels = levels;
    sw.max_width = 0;
    sw.plan.clear();
    for (int32_t l = 0; l < levels; l++) {
        const int32_t w = lptr[(size_t)l + 1] - lptr[(size_t)l];
        sw.max_width = std::max(sw.max_width, w);
        if (w >= wide) sw.plan.push_back({l, 1, lptr[(size_t)l], w, false});
        else if (!sw.plan.empty() && sw.plan.back().merged && sw.plan.back().lvl0 + sw.plan.back().nlvl == l) {
            sw.plan.back().nlvl++;
            sw.plan.back().nslots += w;
        } else sw.plan.push_back({l, 1, lptr[(size_t)l], w, true});
    }
}

// G: the power of two from the mean number of entries of a row in one triangle, ceil((nnz - n) / (2 n)), up; 1 .. 64
int32_t lanes_of(int64_t n, int64_t nnz)
{
    const int64_t mean = n > 0 ? (nnz - n + 2 * n - 1) / (2 * n) : 0;
    int32_t       G = 1;
    while (G < mean && G < 64) G <<= 1;
    return G;
}

constexpr const char *kEntry = "cvr_precond_ilu0";

int upload_sweep(int64_t n, const int64_t *rp, const int64_t *dpos, const std::vector<int32_t> &order, const std::vector<int32_t> &lptr, bool upper, Ilu0Sweep &sw, hipStream_t st,
                 std::vector<Ilu0Slot> &slots)
{
    slots.resize((size_t)n);
    for (int64_t k = 0; k < n; k++) {
        const int32_t i = order[(size_t)k];
        if (upper) slots[(size_t)k] = {dpos[i] + 1, (int32_t)(rp[i + 1] - dpos[i] - 1), i};
        else slots[(size_t)k] = {rp[i], (int32_t)(dpos[i] - rp[i]), i};
    }
    if (const int rc = device_alloc(kEntry, reinterpret_cast<void **>(&sw.d_slots), sizeof(Ilu0Slot) * (size_t)n, "a sweep's rows")) return rc;
    if (const int rc = device_alloc(kEntry, reinterpret_cast<void **>(&sw.d_lptr), sizeof(int32_t) * lptr.size(), "a sweep's levels")) return rc;
    HIP_TRY(hipMemcpyAsync(sw.d_slots, slots.data(), sizeof(Ilu0Slot) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(sw.d_lptr, lptr.data(), sizeof(int32_t) * lptr.size(), hipMemcpyHostToDevice, st));
    return CVR_OK;
}

template <typename T>
int factorise(const cvr_precond *p, const void *va_dev, const int64_t *d_rp, const int64_t *d_dpos, double *d_a, int32_t *d_bad, hipStream_t st)
{
    const Ilu0 *u = p->ilu;
    launch(widen_kernel<T>, st, static_cast<const T *>(va_dev), d_a, (long long)u->nnz);
    for (const Ilu0Launch &ln : u->lo.plan) {
        if (ln.merged)
            hipLaunchKernelGGL(factor_merged_kernel, dim3(1), dim3(kMergedThreads), 0, st, (const Ilu0Slot *)u->lo.d_slots, (const int32_t *)u->lo.d_lptr, (int)ln.lvl0, (int)ln.nlvl, d_rp,
                               d_dpos, (const int32_t *)u->d_ci, d_a, d_bad);
        else
            hipLaunchKernelGGL(factor_wide_kernel, dim3((unsigned)((ln.nslots + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const Ilu0Slot *)u->lo.d_slots, (int)ln.slot0,
                               (int)ln.nslots, d_rp, d_dpos, (const int32_t *)u->d_ci, d_a, d_bad);
    }
    launch(round_kernel<T>, st, (const double *)d_a, static_cast<T *>(u->d_f), (long long)u->nnz);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

int build(cvr_precond *p, const cvr_csr_view *csr, hipStream_t st)
{
    HostCsr h;
    if (const int rc = stage_host(kEntry, csr, h, false, st)) return rc;
    const int64_t n = p->n;
    if (n == 0) return CVR_OK;
    Ilu0         *u = p->ilu;
    const int64_t nnz = h.rp[n];
    const size_t  vsz = p->is_f32 ? 4 : 8;
    u->nnz = nnz;

    std::vector<int32_t>  lvl_lo, lvl_up, order, lptr;
    std::vector<int64_t>  dpos;
    std::vector<Ilu0Slot> slots_lo, slots_up, rows_lo, rows_up;
    try {
        lvl_lo.assign((size_t)n, 0);
        lvl_up.assign((size_t)n, 0);
        dpos.assign((size_t)n, 0);
        int32_t nlo = 0, nup = 0;
        if (const int rc = analyse(n, h.rp, h.ci, "cvr_precond_ilu0", lvl_lo.data(), lvl_up.data(), dpos.data(), &nlo, &nup)) return rc;
        u->G = lanes_of(n, nnz);
        if (const char *e = cvr::debug_env("ilu_lanes")) {          // (an experiment: tools/ilu_probe.py)
            const long long g = atoll(e);
            if (g >= 1 && g <= 64 && (g & (g - 1)) == 0) u->G = (int32_t)g;
        }
        u->wide = kDefaultWide;
        if (const char *e = cvr::debug_env("ilu_wide")) {
            const long long w = atoll(e);
            if (w >= 1) u->wide = (int32_t)std::min<long long>(w, 0x7fffffff);
        }
        plan_sweep(n, lvl_lo.data(), nlo, u->wide, order, lptr, u->lo);
        if (const int rc = upload_sweep(n, h.rp, dpos.data(), order, lptr, false, u->lo, st, slots_lo)) return rc;
        plan_sweep(n, lvl_up.data(), nup, u->wide, order, lptr, u->up);
        if (const int rc = upload_sweep(n, h.rp, dpos.data(), order, lptr, true, u->up, st, slots_up)) return rc;
        if (u->sweeps > 0) {          // the Jacobi sweeps walk the rows in natural order
            ilu0_row_slots(n, h.rp, dpos.data(), false, rows_lo);
            ilu0_row_slots(n, h.rp, dpos.data(), true, rows_up);
        }
    } catch (const std::bad_alloc &) {
        return fail(CVR_ERR_NOMEM, "cvr_precond_ilu0: out of host memory for the analysis (%lld rows)", (long long)n);
    }

    if (const int rc = device_alloc(kEntry, reinterpret_cast<void **>(&u->d_ci), sizeof(int32_t) * (size_t)nnz, "col_idx")) return rc;
    if (const int rc = device_alloc(kEntry, &u->d_f, vsz * (size_t)nnz, "the factors")) return rc;
    if (const int rc = device_alloc(kEntry, &u->d_y, vsz * (size_t)n, "y")) return rc;
    if (u->sweeps > 0) {
        if (const int rc = device_alloc(kEntry, reinterpret_cast<void **>(&u->d_rows_lo), sizeof(Ilu0Slot) * (size_t)n, "L's rows in natural order")) return rc;
        if (const int rc = device_alloc(kEntry, reinterpret_cast<void **>(&u->d_rows_up), sizeof(Ilu0Slot) * (size_t)n, "U's rows in natural order")) return rc;
        if (u->sweeps > 1)
            if (const int rc = device_alloc(kEntry, &u->d_y2, vsz * (size_t)n, "y's second buffer")) return rc;
        if (const int rc = device_alloc(kEntry, &u->d_w, vsz * (size_t)n, "z's second buffer")) return rc;
        HIP_TRY(hipMemcpyAsync(u->d_rows_lo, rows_lo.data(), sizeof(Ilu0Slot) * (size_t)n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(u->d_rows_up, rows_up.data(), sizeof(Ilu0Slot) * (size_t)n, hipMemcpyHostToDevice, st));
        if (u->d_y2) HIP_TRY(hipMemsetAsync(u->d_y2, 0, vsz * (size_t)n, st));
        HIP_TRY(hipMemsetAsync(u->d_w, 0, vsz * (size_t)n, st));
    }
    Scratch s;
    void   *d_rp = nullptr, *d_dpos = nullptr, *d_a = nullptr, *d_bad = nullptr, *d_va = nullptr;
    if (const int rc = scratch_alloc(kEntry, s, &d_rp, sizeof(int64_t) * (size_t)(n + 1), "row_ptr")) return rc;
    if (const int rc = scratch_alloc(kEntry, s, &d_dpos, sizeof(int64_t) * (size_t)n, "the diagonal's positions")) return rc;
    if (const int rc = scratch_alloc(kEntry, s, &d_a, sizeof(double) * (size_t)nnz, "the fp64 copy")) return rc;
    if (const int rc = scratch_alloc(kEntry, s, &d_bad, sizeof(int32_t), "the pivot word")) return rc;
    const void *va = csr->vals;
    if (!csr->arrays_on_device) {
        if (const int rc = scratch_alloc(kEntry, s, &d_va, vsz * (size_t)nnz, "vals")) return rc;
        HIP_TRY(hipMemcpyAsync(d_va, csr->vals, vsz * (size_t)nnz, hipMemcpyHostToDevice, st));
        va = d_va;
    }
    int32_t bad = kNoRow;
    HIP_TRY(hipMemcpyAsync(u->d_ci, h.ci, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_rp, h.rp, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_dpos, dpos.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_bad, &bad, sizeof(bad), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(u->d_y, 0, vsz * (size_t)n, st));
    const int rc = p->is_f32 ? factorise<float>(p, va, static_cast<const int64_t *>(d_rp), static_cast<const int64_t *>(d_dpos), static_cast<double *>(d_a), static_cast<int32_t *>(d_bad), st)
                             : factorise<double>(p, va, static_cast<const int64_t *>(d_rp), static_cast<const int64_t *>(d_dpos), static_cast<double *>(d_a), static_cast<int32_t *>(d_bad), st);
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));          // (the host vectors and the scratch are released behind this)
    if (bad != kNoRow) return fail(CVR_ERR_STATE, "cvr_precond_ilu0: the pivot of row %d is zero or not finite", bad);
    return CVR_OK;
}

}  // namespace

namespace cvrh {
namespace krylov {

template <typename T, typename R>
int ilu0_apply(const cvr_precond *pc, const R *r, T *z, const Ilu0Gate &gate, hipStream_t st)
{
    const Ilu0 *u = pc->ilu;
    if (!u || pc->n == 0) return CVR_OK;
    if (u->sweeps > 0) return jacobi_apply<T, R>(u, (long long)pc->n, r, z, gate, st);
    T *y = static_cast<T *>(u->d_y);
    if (const int rc = enqueue_sweep<T, R, false>(u, u->lo, r, y, gate, st)) return rc;
    return enqueue_sweep<T, T, true>(u, u->up, (const T *)y, z, gate, st);
}
template int ilu0_apply<float, float>(const cvr_precond *, const float *, float *, const Ilu0Gate &, hipStream_t);
template int ilu0_apply<float, double>(const cvr_precond *, const double *, float *, const Ilu0Gate &, hipStream_t);
template int ilu0_apply<double, double>(const cvr_precond *, const double *, double *, const Ilu0Gate &, hipStream_t);

template <typename T>
int ilu0_add_to_x(T *x, const T *zu, long long n, const Ilu0Gate &gate, bool al, hipStream_t st)
{
    with_flags([&](auto AL) { launch(ilu0_xadd_kernel<T, AL>, st, x, zu, n, gate); }, al);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}
template int ilu0_add_to_x<float>(float *, const float *, long long, const Ilu0Gate &, bool, hipStream_t);
template int ilu0_add_to_x<double>(double *, const double *, long long, const Ilu0Gate &, bool, hipStream_t);

namespace {

int ilu0_apply_any(const cvr_precond *p, const void *r, void *z, hipStream_t st)          // by the object's type, no gate
{
    if (p->is_f32) return ilu0_apply<float, float>(p, static_cast<const float *>(r), static_cast<float *>(z), Ilu0Gate{}, st);
    return ilu0_apply<double, double>(p, static_cast<const double *>(r), static_cast<double *>(z), Ilu0Gate{}, st);
}

// the sweeps into z, then one kernel on the solvers' grid with the partial sums and, at the start, p = z
template <typename T>
int ilu0_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *)
{
    const CgCell *c = static_cast<const CgCell *>(cell);
    Ilu0Gate      gate;
    if (!start) {
        gate.stop = &c->stop;
        gate.nstop = 1;
    }
    if (const int rc = ilu0_apply<T, T>(pc, r, z, gate, st)) return rc;
    with_flags([&](auto START) { launch(precond_rz_kernel<T, START, false>, st, r, (const T *)z, (T *)nullptr, p, (long long)pc->n, part_rz, c); }, start);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

void ilu0_release(cvr_precond *p)
{
    Ilu0 *u = p->ilu;
    if (!u) return;
    for (void *buf : {(void *)u->d_ci, u->d_f, u->d_y, (void *)u->lo.d_slots, (void *)u->lo.d_lptr, (void *)u->up.d_slots, (void *)u->up.d_lptr, (void *)u->d_rows_lo,
                      (void *)u->d_rows_up, u->d_y2, u->d_w})
        if (buf) (void)hipFree(buf);
    delete u;
    p->ilu = nullptr;
}

}  // namespace

PrecondOps kIlu0Ops = {kPrecondIlu0, "ILU(0)", ilu0_apply_any, ilu0_release, ilu0_cg_apply<float>, ilu0_cg_apply<double>};

}  // namespace krylov
}  // namespace cvrh

namespace {

// both constructors behind their own argument checks; sweeps = 0: the exact object
int construct(cvr_precond **out, const cvr_csr_view *csr, int32_t sweeps, int32_t device, void *stream, const char *entry)
{
    *out = nullptr;
    if (csr->nrows != csr->ncols) return fail(CVR_ERR_INVALID, "ILU(0) needs a square matrix (%lld x %lld)", (long long)csr->nrows, (long long)csr->ncols);
    if (csr->nrows < 0) return fail(CVR_ERR_INVALID, "null or negative-size CSR view");
    if (device < 0 || device >= cvr_device_count()) return fail(CVR_ERR_NO_DEVICE, "device %d of %d", device, cvr_device_count());
    cvr::debug_refresh();
    Range range(entry);
    HIP_TRY(hipSetDevice(device));
    cvr_precond *p = new (std::nothrow) cvr_precond;
    Ilu0        *u = new (std::nothrow) Ilu0;
    if (!p || !u) {
        delete p;
        delete u;
        return fail(CVR_ERR_NOMEM, "out of host memory");
    }
    p->kind = kPrecondIlu0;
    p->ops = &kIlu0Ops;
    p->device = device;
    p->n = csr->nrows;
    p->bs = 0;
    p->is_f32 = csr->is_f32 ? 1 : 0;
    p->ilu = u;
    u->G = 1;
    u->wide = kDefaultWide;
    u->sweeps = sweeps;
    if (const int rc = build(p, csr, (hipStream_t)stream)) return abandon(p, rc);
    *out = p;
    return CVR_OK;
}

}  // namespace

extern "C" {

int cvr_precond_ilu0(cvr_precond **out, const cvr_csr_view *csr, int32_t device, void *stream)
{
    if (!out || !csr) return fail(CVR_ERR_INVALID, "null argument");
    return construct(out, csr, 0, device, stream, "cvr_precond_ilu0");
}

int cvr_precond_ilu0_jacobi(cvr_precond **out, const cvr_csr_view *csr, int32_t sweeps, int32_t device, void *stream)
{
    if (!out || !csr) return fail(CVR_ERR_INVALID, "null argument");
    *out = nullptr;
    if (sweeps < 1 || sweeps > CVR_ILU0_MAX_SWEEPS) return fail(CVR_ERR_INVALID, "cvr_precond_ilu0_jacobi: sweeps = %d, not in 1 .. %d", sweeps, CVR_ILU0_MAX_SWEEPS);
    return construct(out, csr, sweeps, device, stream, "cvr_precond_ilu0_jacobi");
}

int cvr_precond_ilu0_jacobi_info(const cvr_precond *p, cvr_ilu0_jacobi_info *info)
{
    if (!p || !info) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondIlu0 || !p->ilu) return fail(CVR_ERR_INVALID, "cvr_precond_ilu0_jacobi_info: the preconditioner is of kind %d, not an ILU(0) object (kind %d)", p->kind, kPrecondIlu0);
    const Ilu0 *u = p->ilu;
    if (u->sweeps < 1) return fail(CVR_ERR_INVALID, "cvr_precond_ilu0_jacobi_info: the object is an exact ILU(0) object (cvr_precond_ilu0), not one of cvr_precond_ilu0_jacobi");
    memset(info, 0, sizeof(*info));
    info->n = p->n;
    info->nnz = u->nnz;
    info->sweeps = u->sweeps;
    info->launches_per_apply = p->n > 0 ? 2 * u->sweeps : 0;
    info->lanes_per_row = u->G;
    info->levels_lower = u->lo.levels;
    info->levels_upper = u->up.levels;
    info->is_f32 = p->is_f32;
    return CVR_OK;
}

int cvr_precond_ilu0_info(const cvr_precond *p, cvr_ilu0_info *info)
{
    if (!p || !info) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondIlu0 || !p->ilu) return fail(CVR_ERR_INVALID, "cvr_precond_ilu0_info: the preconditioner is of kind %d, not an ILU(0) object (kind %d)", p->kind, kPrecondIlu0);
    const Ilu0 *u = p->ilu;
    memset(info, 0, sizeof(*info));
    info->n = p->n;
    info->nnz = u->nnz;
    info->levels_lower = u->lo.levels;
    info->levels_upper = u->up.levels;
    info->launches_lower = (int32_t)u->lo.plan.size();
    info->launches_upper = (int32_t)u->up.plan.size();
    if (u->sweeps > 0) info->launches_lower = info->launches_upper = p->n > 0 ? u->sweeps : 0;          // (a Jacobi-swept object: what an apply enqueues)
    info->max_level_width = std::max(u->lo.max_width, u->up.max_width);
    info->lanes_per_row = u->G;
    info->wide_threshold = u->wide;
    info->is_f32 = p->is_f32;
    return CVR_OK;
}

int cvr_precond_ilu0_export(const cvr_precond *p, void *vals_host)
{
    if (!p || !vals_host) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondIlu0 || !p->ilu) return fail(CVR_ERR_INVALID, "cvr_precond_ilu0_export: the preconditioner is of kind %d, not an ILU(0) object (kind %d)", p->kind, kPrecondIlu0);
    if (p->ilu->nnz == 0) return CVR_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpy(vals_host, p->ilu->d_f, (p->is_f32 ? 4 : 8) * (size_t)p->ilu->nnz, hipMemcpyDeviceToHost));
    return CVR_OK;
}

int cvr_ilu0_levels_host(const cvr_csr_view *csr, int32_t *lower_level, int32_t *upper_level, int32_t *n_lower, int32_t *n_upper)
{
    if (!csr || !n_lower || !n_upper) return fail(CVR_ERR_INVALID, "null argument");
    if (csr->nrows > 0 && (!lower_level || !upper_level)) return fail(CVR_ERR_INVALID, "null argument");
    if (csr->arrays_on_device) return fail(CVR_ERR_INVALID, "cvr_ilu0_levels_host: the arrays must be host arrays");
    if (csr->nrows != csr->ncols) return fail(CVR_ERR_INVALID, "ILU(0) needs a square matrix (%lld x %lld)", (long long)csr->nrows, (long long)csr->ncols);
    cvr_csr_view v = *csr;
    if (!v.vals) v.vals = v.col_idx;          // (not read here)
    if (const int rc = check_csr(&v, true)) return rc;
    *n_lower = *n_upper = 0;
    if (csr->nrows == 0) return CVR_OK;
    return analyse(csr->nrows, csr->row_ptr, csr->col_idx, "cvr_ilu0_levels_host", lower_level, upper_level, nullptr, n_lower, n_upper);
}

}  // extern "C"
