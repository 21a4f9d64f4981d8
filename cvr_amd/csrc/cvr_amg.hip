// cvr_amg.hip -- plain (unsmoothed) aggregation AMG, the fifth kind of cvr_precond (include/cvr_amd.h: cvr_precond_amg, cvr_precond_amg_info,
// cvr_precond_amg_export_level; the set-up, all of it on the host: cvr_amg_host.cpp).  The apply is one V-cycle that never leaves the SpMV path:
// every level's operator is a handle (level 0: the caller's, borrowed; the coarse levels: the object's own, from device arrays with the default
// options), the smoother is l1-Jacobi (one product and one element-wise kernel), the restriction a segmented sum over an aggregate-members CSR (one
// lane per aggregate, rows ascending: no atomics, one order), the prolongation a gather.  No triangular sweep, no level schedule, no dot product, no
// read-back, no kernel that waits on another workgroup.
//   Per level: r (n values), z (an SpMV input: element n stays 0 -- the kernels write elements 0 .. n - 1 only, and no product writes into a z),
//     q (an SpMV output), dinv, and above the coarsest level agg, mrp and mem.  No buffer is one product's output and another one's input, so
//     there is no pad slot to zero between products.
//   Apply: precond_copy_in_kernel (r_0 = r) | down: amg_first_kernel, [product, amg_smooth_kernel] x (sweeps - 1), product, amg_restrict_kernel | the
//     coarsest level: amg_dense_kernel (z = W r, one workgroup, a thread per row) or 2 * sweeps sweeps | up: amg_prolong_kernel, [product,
//     amg_smooth_kernel] x sweeps | precond_copy_out_kernel (z = z_0), or inside cvr_pcg_device precond_rz_kernel in its place (z = z_0 with the
//     partial sums of r . z and, at the start, p = z; nothing behind a stop): cvr_precond.h's.  The level kernels take a thread per element on a grid cut to the level's size; the
//     first and the last run on the solvers' grid.
// The smoothed kind (cvr_precond_amg_smoothed: the same object with Hierarchy::smoothed set) builds every level on the device inside the host
// set-up's loop (SmoothedBuild: amg_tentative_kernel, the device SpGEMM, amg_prolongator_kernel, transpose_csr, two more products), owns a handle of
// P_l and one of R_l per level and moves between levels by products: amg_residual_kernel and R_l's product in place of amg_restrict_kernel, P_l's
// product and amg_correct_kernel in place of amg_prolong_kernel.  Per level two more buffers: t (R_l's input, element n stays 0) and e (P_l's output).
// The device set-up (cvr_precond_amg_mis2: setup_mis2 below) builds the same smoothed object with no level loop on the host: the MIS(2) aggregation
// and the diagonal are kernels (cvr_amg_mis2.hip), steps 1 - 5 are SmoothedBuild::coarsen, every level's CSR, dinv, agg and P_l stay in device arrays
// of the object's own, and the exports copy from them when first asked (fetch_level, fetch_prolongator).  DESIGN.md 5.44.
// cvr_precond_amg_block (cvr_amg_block.hip) builds the same object through this file's constructor with Amg::width = K: the set-up is the one above,
// untouched; every handle of the object's own is created with cvr_options.nvec = K and every buffer holds K columns (cvr_amg_dev.h).  This file's
// cycle serves its single-vector calls on those buffers at ld = 1, behind amg_zero_pads_kernel; the K-wide cycle is cvr_amg_block.hip's.
// (The reference has no solver and no preconditioner: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
#include "cvr_krylov.h"
#include "cvr_cg_kernels.h"
#include "cvr_precond.h"
#include "cvr_amg_dev.h"
#include "cvr_amg_mis2.h"

using namespace cvrh;
using namespace cvrh::krylov;

namespace {

// ---- the device half

// z_i = T(dinv_i * r_i)
template <typename T>
__global__ __launch_bounds__(kThreads) void amg_first_kernel(const T *__restrict__ dinv, const T *__restrict__ r, T *__restrict__ z, long long n)
{
    CVR_AMG_ELEMENTS(i, n) z[i] = (T)((double)dinv[i] * (double)r[i]);
}

// behind q = A z: z_i = T(z_i + dinv_i * (r_i - q_i))
template <typename T>
__global__ __launch_bounds__(kThreads) void amg_smooth_kernel(const T *__restrict__ dinv, const T *__restrict__ r, const T *__restrict__ q, T *__restrict__ z, long long n)
{
    CVR_AMG_ELEMENTS(i, n) z[i] = (T)((double)z[i] + (double)dinv[i] * ((double)r[i] - (double)q[i]));
}

// behind q = A z: rc_I = T(+0 + (r_i - q_i) + ..) over the rows of aggregate I, ascending; a lane per aggregate
template <typename T>
__global__ __launch_bounds__(kThreads) void amg_restrict_kernel(const int64_t *__restrict__ mrp, const int32_t *__restrict__ mem, const T *__restrict__ r, const T *__restrict__ q,
                                                                T *__restrict__ rc, long long nc)
{
    CVR_AMG_ELEMENTS(I, nc) {
        double s = 0;
        for (long long m = mrp[I]; m < mrp[I + 1]; m++) {
            const int i = mem[m];
            s = s + ((double)r[i] - (double)q[i]);
        }
        rc[I] = (T)s;
    }
}

// z_i = T(z_i + scale * zc[agg_i])
template <typename T>
__global__ __launch_bounds__(kThreads) void amg_prolong_kernel(const int32_t *__restrict__ agg, const T *__restrict__ zc, T *__restrict__ z, long long n, double scale)
{
    CVR_AMG_ELEMENTS(i, n) z[i] = (T)((double)z[i] + scale * (double)zc[agg[i]]);
}

// ---- the smoothed kind
// behind q = A z: t_i = T(r_i - q_i), the input of R's product
template <typename T>
__global__ __launch_bounds__(kThreads) void amg_residual_kernel(const T *__restrict__ r, const T *__restrict__ q, T *__restrict__ t, long long n)
{
    CVR_AMG_ELEMENTS(i, n) t[i] = (T)((double)r[i] - (double)q[i]);
}

// behind e = P zc: z_i = T(z_i + scale * e_i)
template <typename T>
__global__ __launch_bounds__(kThreads) void amg_correct_kernel(const T *__restrict__ e, T *__restrict__ z, long long n, double scale)
{
    CVR_AMG_ELEMENTS(i, n) z[i] = (T)((double)z[i] + scale * (double)e[i]);
}

// the tentative prolongator as a CSR: row_ptr = 0 .. n, col_idx = agg, vals = 1
template <typename T>
__global__ __launch_bounds__(kThreads) void amg_tentative_kernel(const int32_t *__restrict__ agg, int64_t *__restrict__ rp, int32_t *__restrict__ ci, T *__restrict__ va, long long n)
{
    CVR_AMG_ELEMENTS(i, n + 1) {
        rp[i] = i;
        if (i < n) {
            ci[i] = agg[i];
            va[i] = T(1);
        }
    }
}

// P on the pattern of G = A T, a thread per row: w = omega * dinv_i; p_ij = T([j == agg_i] - w * g_ij)
template <typename T>
__global__ __launch_bounds__(kThreads) void amg_prolongator_kernel(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ g, const int32_t *__restrict__ agg,
                                                                   const T *__restrict__ dinv, double omega, T *__restrict__ p, long long n)
{
    CVR_AMG_ELEMENTS(i, n) {
        const double w = omega * (double)dinv[i];
        const int    own = agg[i];
        for (long long q = rp[i]; q < rp[i + 1]; q++) {
            const double wg = w * (double)g[q];
            p[q] = (T)((ci[q] == own ? 1.0 : 0.0) - wg);
        }
    }
}

// the directly solved coarsest level, n <= CVR_AMG_MAX_COARSE: z_i = T(t_0 + t_1 + ..), t_j = W_ij * r_j; W is symmetric bit for bit, so thread i
// reads W_ji, which neighbouring threads find side by side
template <typename T>
__global__ __launch_bounds__(CVR_AMG_MAX_COARSE) void amg_dense_kernel(const T *__restrict__ w, const T *__restrict__ r, T *__restrict__ z, int n)
{
    const int i = threadIdx.x;
    if (i >= n) return;
    double s = (double)w[i] * (double)r[0];
    for (int j = 1; j < n; j++) s = s + (double)w[(size_t)j * n + i] * (double)r[j];
    z[i] = (T)s;
}

// a block object's single-vector calls: the pad slots of the SpMV inputs at ld = 1 (cvr_amg_dev.h); at most 2 * CVR_AMG_MAX_LEVELS of them
template <typename T>
__global__ __launch_bounds__(64) void amg_zero_pads_kernel(T *const *__restrict__ pads, int count)
{
    if ((int)threadIdx.x < count) *pads[threadIdx.x] = (T)0;
}

// ---- the host half

constexpr const char *kEntry = "cvr_precond_amg";          // (as the allocation messages of both constructors begin)

// a level's CSR in device memory, uploaded from the host's copy into buffers that `s` owns
int upload_level(const amg::Level &l, int is_f32, Scratch &s, const char *rp_what, const char *ci_what, const char *va_what, cvr_csr_view *out)
{
    void *d_rp = nullptr, *d_ci = nullptr, *d_va = nullptr;
    if (const int rc = upload(kEntry, &d_rp, l.rp.data(), sizeof(int64_t) * l.rp.size(), rp_what)) return rc;
    s.bufs.push_back(d_rp);
    if (const int rc = upload(kEntry, &d_ci, l.ci.data(), sizeof(int32_t) * l.ci.size(), ci_what)) return rc;
    s.bufs.push_back(d_ci);
    if (const int rc = upload(kEntry, &d_va, l.va.data(), l.va.size(), va_what)) return rc;
    s.bufs.push_back(d_va);
    *out = cvr_csr_view{};
    out->nrows = out->ncols = l.n;
    out->row_ptr = static_cast<const int64_t *>(d_rp);
    out->col_idx = static_cast<const int32_t *>(d_ci);
    out->vals = d_va;
    out->is_f32 = is_f32;
    out->arrays_on_device = 1;
    return CVR_OK;
}

// The smoothed kind's levels on the device, one coarsening step per call from inside amg::setup's loop (the aggregation before it and the next
// level's diagonal behind it are the host's).  `cur` is the level's CSR in device memory: level 0 uploaded from the host's copy, a coarse level the
// product that made it, kept until the next step has read it.
struct SmoothedBuild {
    cvr_precond *p = nullptr;
    hipStream_t  st = nullptr;
    double       omega = 0;
    cvr_spgemm  *cur_owner = nullptr;
    Scratch      cur_bufs;
    cvr_csr_view cur{};
    SmoothedBuild() = default;
    SmoothedBuild(const SmoothedBuild &) = delete;
    SmoothedBuild &operator=(const SmoothedBuild &) = delete;
    ~SmoothedBuild()
    {
        if (cur_owner) (void)cvr_spgemm_destroy(cur_owner);
    }

    struct Product {          // a cvr_spgemm that lives for one step
        cvr_spgemm *g = nullptr;
        Product() = default;
        Product(const Product &) = delete;
        Product &operator=(const Product &) = delete;
        ~Product()
        {
            if (g) (void)cvr_spgemm_destroy(g);
        }
    };
    struct Transposed {
        TransposedCsr t;
        Transposed() = default;
        Transposed(const Transposed &) = delete;
        Transposed &operator=(const Transposed &) = delete;
        ~Transposed() { t.release(); }
    };

    // Steps 1 - 5 of one level whose dinv and agg lie in dl: what lives on behind them, until the caller has taken its copies
    struct Coarse {
        Product      G, AC;
        Scratch      s;          // T's arrays and P's values
        cvr_csr_view pv{}, acv{};
        void        *d_pva = nullptr;
        size_t       pnnz = 0;
        int64_t      cnnz = 0;
    };

    // ... and the two transfer handles; returns with the device idle
    template <typename T>
    static int coarsen(cvr_precond *p, AmgLevel &dl, const cvr_csr_view &cur, long long n, int64_t nc, double omega, hipStream_t st, Coarse &o)
    {
        const int is_f32 = p->is_f32;
        // 1. T
        Scratch &s = o.s;
        void    *d_trp = nullptr, *d_tci = nullptr, *d_tva = nullptr, *d_pva = nullptr;
        if (const int rc = device_alloc(kEntry, &d_trp, sizeof(int64_t) * (size_t)(n + 1), "the tentative prolongator")) return rc;
        s.bufs.push_back(d_trp);
        if (const int rc = device_alloc(kEntry, &d_tci, sizeof(int32_t) * (size_t)n, "the tentative prolongator")) return rc;
        s.bufs.push_back(d_tci);
        if (const int rc = device_alloc(kEntry, &d_tva, sizeof(T) * (size_t)n, "the tentative prolongator")) return rc;
        s.bufs.push_back(d_tva);
        launch_level(amg_tentative_kernel<T>, n + 1, st, static_cast<const int32_t *>(dl.d_agg), static_cast<int64_t *>(d_trp), static_cast<int32_t *>(d_tci), static_cast<T *>(d_tva), n);
        HIP_TRY(hipGetLastError());
        cvr_csr_view tv{};
        tv.nrows = n;
        tv.ncols = nc;
        tv.row_ptr = static_cast<const int64_t *>(d_trp);
        tv.col_idx = static_cast<const int32_t *>(d_tci);
        tv.vals = d_tva;
        tv.is_f32 = is_f32;
        tv.arrays_on_device = 1;
        // 2. G = A T (cvr_spgemm_create orders itself behind `st` and returns with it idle)
        Product      AP;
        cvr_csr_view gv{}, apv{};
        if (const int rc = cvr_spgemm_create(&o.G.g, &cur, &tv, p->device, st)) return rc;
        if (const int rc = cvr_spgemm_csr_device(o.G.g, &gv)) return rc;
        cvr_spgemm_info_t gi;
        if (const int rc = cvr_spgemm_get_info(o.G.g, &gi)) return rc;
        const size_t pnnz = (size_t)gi.nnz;
        // 3. P on G's pattern
        if (const int rc = device_alloc(kEntry, &d_pva, sizeof(T) * pnnz, "the prolongator's values")) return rc;
        s.bufs.push_back(d_pva);
        launch_level(amg_prolongator_kernel<T>, n, st, gv.row_ptr, gv.col_idx, static_cast<const T *>(gv.vals), static_cast<const int32_t *>(dl.d_agg), static_cast<const T *>(dl.d_dinv), omega,
                     static_cast<T *>(d_pva), n);
        HIP_TRY(hipGetLastError());
        cvr_csr_view pv = gv;
        pv.vals = d_pva;
        // 4. R = P^T (synchronises st)
        Transposed R;
        if (const int rc = transpose_csr(pv, 0, (int64_t)pnnz, false, st, &R.t)) return rc;
        cvr_csr_view rv{};
        rv.nrows = R.t.nrows;
        rv.ncols = R.t.ncols;
        rv.row_ptr = R.t.rp;
        rv.col_idx = R.t.ci;
        rv.vals = R.t.va;
        rv.is_f32 = is_f32;
        rv.arrays_on_device = 1;
        // 5. A_c = R (A P)
        if (const int rc = cvr_spgemm_create(&AP.g, &cur, &pv, p->device, st)) return rc;
        if (const int rc = cvr_spgemm_csr_device(AP.g, &apv)) return rc;
        if (const int rc = cvr_spgemm_create(&o.AC.g, &rv, &apv, p->device, st)) return rc;
        if (const int rc = cvr_spgemm_csr_device(o.AC.g, &o.acv)) return rc;
        cvr_spgemm_info_t ci;
        if (const int rc = cvr_spgemm_get_info(o.AC.g, &ci)) return rc;
        // the two transfer handles, from the device arrays
        if (const int rc = make_handle(&dl.hp, pv, p->device, 0, p->amg->width)) return rc;
        if (const int rc = make_handle(&dl.hr, rv, p->device, 0, p->amg->width)) return rc;
        HIP_TRY(hipDeviceSynchronize());          // (the handles' copies are complete before the step's arrays go)
        o.pv = pv;
        o.d_pva = d_pva;
        o.pnnz = pnnz;
        o.cnnz = ci.nnz;
        return CVR_OK;
    }

    template <typename T>
    int step(amg::Level &f, amg::Level &c, int32_t level)
    {
        Amg      *a = p->amg;
        AmgLevel &dl = a->lv[(size_t)level];          // (sized for CVR_AMG_MAX_LEVELS before the set-up)
        const int is_f32 = p->is_f32;
        if (level == 0) {
            if (const int rc = upload_level(f, is_f32, cur_bufs, "level 0's row_ptr", "level 0's col_idx", "level 0's values", &cur)) return rc;
        } else {
            dl.own = true;
            if (const int rc = make_handle(&dl.h, cur, p->device, 0, a->width)) return rc;
        }
        const long long n = f.n;
        if (const int rc = upload(kEntry, &dl.d_dinv, f.dinv.data(), f.dinv.size(), "dinv")) return rc;
        if (const int rc = upload(kEntry, &dl.d_agg, f.agg.data(), sizeof(int32_t) * f.agg.size(), "agg")) return rc;
        Coarse o;
        if (const int rc = coarsen<T>(p, dl, cur, n, f.nc, omega, st, o)) return rc;
        const size_t pnnz = o.pnnz;
        // the host's copies: P for the export, A_c for the next level's aggregation and the export
        f.pnnz = (int64_t)pnnz;
        f.prp.assign((size_t)n + 1, 0);
        f.pci.assign(pnnz, 0);
        f.pva.assign(sizeof(T) * pnnz, 0);
        HIP_TRY(hipMemcpy(f.prp.data(), o.pv.row_ptr, sizeof(int64_t) * f.prp.size(), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(f.pci.data(), o.pv.col_idx, sizeof(int32_t) * pnnz, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(f.pva.data(), o.d_pva, sizeof(T) * pnnz, hipMemcpyDeviceToHost));
        c.n = f.nc;
        c.nnz = o.cnnz;
        c.rp.assign((size_t)c.n + 1, 0);
        c.ci.assign((size_t)c.nnz, 0);
        c.va.assign(sizeof(T) * (size_t)c.nnz, 0);
        if (const int rc = cvr_spgemm_export(o.AC.g, c.rp.data(), c.ci.data(), c.va.data())) return rc;
        if (cur_owner) (void)cvr_spgemm_destroy(cur_owner);
        cur_owner = o.AC.g;
        o.AC.g = nullptr;
        Scratch().bufs.swap(cur_bufs.bufs);          // (level 0's upload goes with the temporary)
        cur = o.acv;
        return CVR_OK;
    }
};

size_t x_bytes_of(const cvr_handle *h, size_t cols) { return h->vsz * cols * (size_t)std::max<int64_t>(h->info.x_elems, h->info.ncols + 1); }

enum class Mode { kPlain = CVR_AMG_SETUP_PLAIN, kSmoothed = CVR_AMG_SETUP_SMOOTHED, kMis2 = CVR_AMG_SETUP_MIS2 };
const char *entry_of(Mode m) { return m == Mode::kMis2 ? "cvr_precond_amg_mis2" : m == Mode::kSmoothed ? "cvr_precond_amg_smoothed" : "cvr_precond_amg"; }

// row_ptr[i] -= base
__global__ __launch_bounds__(kThreads) void amg_rebase_kernel(int64_t *__restrict__ rp, long long n1, long long base)
{
    CVR_AMG_ELEMENTS(i, n1) rp[i] -= base;
}

cvr_csr_view level_view(const AmgLevel &dl, int64_t n, int is_f32)
{
    cvr_csr_view v{};
    v.nrows = v.ncols = n;
    v.row_ptr = static_cast<const int64_t *>(dl.d_arp);
    v.col_idx = static_cast<const int32_t *>(dl.d_aci);
    v.vals = dl.d_ava;
    v.is_f32 = is_f32;
    v.arrays_on_device = 1;
    return v;
}

// The device set-up's copy of a level or a prolongator in H, made when an export first asks for it
int fetch_level(const cvr_precond *p, int32_t level)
{
    Amg *a = p->amg;
    if (!a->on_demand || level < 0 || level >= (int32_t)a->H.lv.size()) return CVR_OK;          // (a level outside: the export's own error)
    amg::Level     &l = a->H.lv[(size_t)level];
    const AmgLevel &dl = a->lv[(size_t)level];
    const size_t    vsz = p->is_f32 ? 4 : 8;
    HIP_TRY(hipSetDevice(p->device));
    try {
        if (l.rp.empty()) {
            std::vector<int64_t> rp((size_t)l.n + 1, 0);
            std::vector<int32_t> ci((size_t)l.nnz, 0);
            std::vector<uint8_t> va(vsz * (size_t)l.nnz, 0);
            HIP_TRY(hipMemcpy(rp.data(), dl.d_arp, sizeof(int64_t) * rp.size(), hipMemcpyDeviceToHost));
            if (l.nnz > 0) {
                HIP_TRY(hipMemcpy(ci.data(), dl.d_aci, sizeof(int32_t) * ci.size(), hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(va.data(), dl.d_ava, va.size(), hipMemcpyDeviceToHost));
            }
            l.ci.swap(ci);
            l.va.swap(va);
            l.rp.swap(rp);
        }
        if (l.dinv.empty() && l.n > 0) {
            std::vector<uint8_t> dinv(vsz * (size_t)l.n, 0);
            HIP_TRY(hipMemcpy(dinv.data(), dl.d_dinv, dinv.size(), hipMemcpyDeviceToHost));
            l.dinv.swap(dinv);
        }
        if (l.agg.empty() && level + 1 < (int32_t)a->H.lv.size()) {
            std::vector<int32_t> agg((size_t)l.n, 0);
            HIP_TRY(hipMemcpy(agg.data(), dl.d_agg, sizeof(int32_t) * agg.size(), hipMemcpyDeviceToHost));
            l.agg.swap(agg);
        }
    } catch (const std::bad_alloc &) {
        return fail(CVR_ERR_NOMEM, "%s: out of host memory for level %d", kEntry, level);
    }
    return CVR_OK;
}

int fetch_prolongator(const cvr_precond *p, int32_t level)
{
    Amg *a = p->amg;
    if (!a->on_demand || level < 0 || level + 1 >= (int32_t)a->H.lv.size()) return CVR_OK;
    amg::Level     &l = a->H.lv[(size_t)level];
    const AmgLevel &dl = a->lv[(size_t)level];
    if (!l.prp.empty()) return CVR_OK;
    HIP_TRY(hipSetDevice(p->device));
    try {
        std::vector<int64_t> rp((size_t)l.n + 1, 0);
        std::vector<int32_t> ci((size_t)l.pnnz, 0);
        std::vector<uint8_t> va((p->is_f32 ? 4 : 8) * (size_t)l.pnnz, 0);
        HIP_TRY(hipMemcpy(rp.data(), dl.d_prp, sizeof(int64_t) * rp.size(), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ci.data(), dl.d_pci, sizeof(int32_t) * ci.size(), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(va.data(), dl.d_pva, va.size(), hipMemcpyDeviceToHost));
        l.pci.swap(ci);
        l.pva.swap(va);
        l.prp.swap(rp);
    } catch (const std::bad_alloc &) {
        return fail(CVR_ERR_NOMEM, "%s: out of host memory for the prolongator of level %d", kEntry, level);
    }
    return CVR_OK;
}

// bytes of device memory into a buffer of the object's own, enqueued on st
int device_copy(void **out, const void *src, size_t bytes, const char *what, hipStream_t st)
{
    if (const int rc = device_alloc(kEntry, out, bytes, what)) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(*out, src, bytes, hipMemcpyDeviceToDevice, st));
    return CVR_OK;
}

// cvr_precond_amg_mis2's set-up: the smoothed kind's level loop with nothing of it on the host.  Level 0 becomes arrays of the object's own (from
// host arrays, or from device arrays behind their checks); per level the diagonal kernel, the MIS(2) aggregation (cvr_amg_mis2.hip), steps 1 - 5
// (SmoothedBuild::coarsen) and device-to-device copies of P_l and A_(l+1) into arrays the object keeps for the next level and for the exports.
// The host waits on scalars and reads the coarsest level for the dense inverse.  *cur: the last level's CSR, for its handle.
template <typename T>
int setup_mis2(cvr_precond *p, const cvr_csr_view *csr, const cvr_amg_options *opt, double omega, hipStream_t st, cvr_csr_view *cur_out)
{
    Amg            *a = p->amg;
    const char     *entry = a->entry;
    amg::Hierarchy &H = a->H;
    const int       is_f32 = p->is_f32;
    const int64_t   n0 = p->n;
    int64_t         j0 = 0, j1 = 0;
    cvr::debug_refresh();
    if (csr->arrays_on_device) {          // (host arrays: checked before any device work, in construct)
        std::vector<int64_t> rp_host;
        if (const int rc = check_device_view(kEntry, csr, rp_host, st)) return rc;
        if (n0 > 0) j0 = rp_host.front(), j1 = rp_host.back();
        if (j1 > j0 && !csr->vals) return fail(CVR_ERR_INVALID, "vals is null");
        if (const int rc = mis2_check_structure_device(entry, *csr, rp_host, st)) return rc;
    } else if (n0 > 0) j0 = csr->row_ptr[0], j1 = csr->row_ptr[n0];
    if (n0 == 0) {          // one empty level, inverted directly: the host's set-up makes it
        int32_t bad_level = -1;
        int64_t bad_row = -1;
        const int64_t rp0 = 0;
        if (const int rc = amg::setup(H, 0, &rp0, nullptr, nullptr, is_f32, opt, entry, &bad_level, &bad_row, nullptr, amg::Aggregation::kMis2)) return rc;
        H.smoothed = 1;
        H.omega = omega;
        return CVR_OK;
    }
    try {
        H = amg::Hierarchy();
        H.lv.reserve(CVR_AMG_MAX_LEVELS);
        H.lv.emplace_back();
        a->lv.resize(CVR_AMG_MAX_LEVELS);
    } catch (const std::bad_alloc &) {
        return fail(CVR_ERR_NOMEM, "%s: out of host memory", entry);
    }
    H.opt = *opt;
    H.is_f32 = is_f32;
    H.smoothed = 1;
    H.omega = omega;
    H.mis2 = 1;
    a->on_demand = true;
    // level 0 in the object's own arrays, row_ptr[0] = 0
    {
        AmgLevel           &d0 = a->lv[0];
        const size_t        nnz = (size_t)(j1 - j0);
        const hipMemcpyKind kind = csr->arrays_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        if (const int rc = device_alloc(kEntry, &d0.d_arp, sizeof(int64_t) * (size_t)(n0 + 1), "level 0's row_ptr")) return rc;
        if (const int rc = device_alloc(kEntry, &d0.d_aci, sizeof(int32_t) * nnz, "level 0's col_idx")) return rc;
        if (const int rc = device_alloc(kEntry, &d0.d_ava, sizeof(T) * nnz, "level 0's values")) return rc;
        HIP_TRY(hipMemcpyAsync(d0.d_arp, csr->row_ptr, sizeof(int64_t) * (size_t)(n0 + 1), kind, st));
        if (nnz > 0) {
            HIP_TRY(hipMemcpyAsync(d0.d_aci, csr->col_idx + j0, sizeof(int32_t) * nnz, kind, st));
            HIP_TRY(hipMemcpyAsync(d0.d_ava, static_cast<const T *>(csr->vals) + j0, sizeof(T) * nnz, kind, st));
        }
        if (j0 != 0) launch_level(amg_rebase_kernel, n0 + 1, st, static_cast<int64_t *>(d0.d_arp), (long long)(n0 + 1), (long long)j0);
        HIP_TRY(hipGetLastError());
        H.lv[0].n = n0;
        H.lv[0].nnz = (int64_t)nnz;
    }
    cvr_csr_view cur = level_view(a->lv[0], n0, is_f32);
    for (;;) {
        const int32_t level = (int32_t)H.lv.size() - 1;
        amg::Level   &l = H.lv.back();
        AmgLevel     &dl = a->lv[(size_t)level];
        const int64_t n = l.n;
        Scratch       s;
        void         *d_diag = nullptr;
        int64_t       bad = -1;
        if (const int rc = device_alloc(kEntry, &dl.d_dinv, sizeof(T) * (size_t)n, "dinv")) return rc;
        if (const int rc = scratch_alloc(kEntry, s, &d_diag, sizeof(double) * (size_t)n, "the diagonal")) return rc;
        if (const int rc = mis2_diagonal_device(kEntry, cur, dl.d_dinv, static_cast<double *>(d_diag), &bad, st)) return rc;
        if (bad >= 0) return fail(CVR_ERR_STATE, "%s: level %d: the diagonal entry of row %lld is not finite or not > 0", entry, level, (long long)bad);
        if (n <= H.opt.coarse_size || (int32_t)H.lv.size() == H.opt.max_levels) break;
        int64_t nc = 0;
        int32_t rounds = 0;
        if (const int rc = device_alloc(kEntry, &dl.d_agg, sizeof(int32_t) * (size_t)n, "agg")) return rc;
        if (const int rc = mis2_aggregate_device(kEntry, cur, 0, l.nnz, static_cast<const double *>(d_diag), H.opt.strength, static_cast<int32_t *>(dl.d_agg), &nc, &rounds, st)) return rc;
        if ((double)nc > 0.8 * (double)n) {          // a stall: this level is the last
            (void)hipFree(dl.d_agg);
            dl.d_agg = nullptr;
            break;
        }
        l.nc = nc;
        H.rounds[level] = rounds;
        if (level > 0) {
            dl.own = true;
            if (const int rc = make_handle(&dl.h, cur, p->device, 0, a->width)) return rc;
        }
        SmoothedBuild::Coarse o;
        if (const int rc = SmoothedBuild::coarsen<T>(p, dl, cur, n, nc, omega, st, o)) return rc;
        AmgLevel &dn = a->lv[(size_t)level + 1];
        if (const int rc = device_copy(&dl.d_prp, o.pv.row_ptr, sizeof(int64_t) * (size_t)(n + 1), "a prolongator's row_ptr", st)) return rc;
        if (const int rc = device_copy(&dl.d_pci, o.pv.col_idx, sizeof(int32_t) * o.pnnz, "a prolongator's col_idx", st)) return rc;
        if (const int rc = device_copy(&dl.d_pva, o.d_pva, sizeof(T) * o.pnnz, "a prolongator's values", st)) return rc;
        if (const int rc = device_copy(&dn.d_arp, o.acv.row_ptr, sizeof(int64_t) * (size_t)(nc + 1), "a level's row_ptr", st)) return rc;
        if (const int rc = device_copy(&dn.d_aci, o.acv.col_idx, sizeof(int32_t) * (size_t)o.cnnz, "a level's col_idx", st)) return rc;
        if (const int rc = device_copy(&dn.d_ava, o.acv.vals, sizeof(T) * (size_t)o.cnnz, "a level's values", st)) return rc;
        HIP_TRY(hipStreamSynchronize(st));          // (the copies are complete before the step's arrays go)
        l.pnnz = (int64_t)o.pnnz;
        H.lv.emplace_back();          // (reserved: l stays where it is)
        H.lv.back().n = nc;
        H.lv.back().nnz = o.cnnz;
        cur = level_view(dn, nc, is_f32);
    }
    const int32_t last = (int32_t)H.lv.size() - 1;
    if (H.lv.back().n <= CVR_AMG_MAX_COARSE) {          // the coarsest level comes to the host for its inverse
        H.coarse_direct = 1;
        if (const int rc = fetch_level(p, last)) return rc;
        int64_t bad = -1;
        try {
            bad = amg::coarsest_inverse(H.lv.back(), is_f32, H.winv);
        } catch (const std::bad_alloc &) {
            return fail(CVR_ERR_NOMEM, "%s: out of host memory", entry);
        }
        if (bad >= 0) return fail(CVR_ERR_STATE, "%s: level %d: the pivot of row %lld of the coarsest matrix is not finite or not > 0", entry, last, (long long)bad);
    }
    *cur_out = cur;
    return CVR_OK;
}

int build(cvr_precond *p, cvr_handle *h, const cvr_csr_view *csr, const cvr_amg_options *opt, Mode mode, double omega, hipStream_t st)
{
    Amg          *a = p->amg;
    const bool    smoothed = mode != Mode::kPlain;
    const char   *entry = a->entry;
    const size_t  K = (size_t)std::max<int32_t>(a->width, 1);          // columns per buffer
    SmoothedBuild sb;
    if (mode == Mode::kMis2) {
        if (const int rc = p->is_f32 ? setup_mis2<float>(p, csr, opt, omega, st, &sb.cur) : setup_mis2<double>(p, csr, opt, omega, st, &sb.cur)) return rc;
    } else {
        HostCsr hc;
        if (const int rc = stage_host(kEntry, csr, hc, true, st)) return rc;
        if (csr->arrays_on_device)          // (host arrays: checked before any device work, in construct)
            if (const int rc = amg::check_structure(p->n, hc.rp, hc.ci, kEntry)) return rc;
        int32_t bad_level = -1;
        int64_t bad_row = -1;
        if (smoothed) {
            try {
                a->lv.resize(CVR_AMG_MAX_LEVELS);
            } catch (const std::bad_alloc &) {
                return fail(CVR_ERR_NOMEM, "%s: out of host memory", entry);
            }
            sb.p = p;
            sb.st = st;
            sb.omega = omega;
            const amg::Coarsen coarsen = [&](amg::Level &f, amg::Level &c, int32_t level) {
                return p->is_f32 ? sb.step<float>(f, c, level) : sb.step<double>(f, c, level);
            };
            if (const int rc = amg::setup(a->H, p->n, hc.rp, hc.ci, hc.va, p->is_f32, opt, entry, &bad_level, &bad_row, &coarsen)) return rc;
            a->H.smoothed = 1;
            a->H.omega = omega;
        } else if (const int rc = amg::setup(a->H, p->n, hc.rp, hc.ci, hc.va, p->is_f32, opt, entry, &bad_level, &bad_row)) return rc;
    }
    const amg::Hierarchy &H = a->H;
    const size_t          vsz = p->is_f32 ? 4 : 8, L = H.lv.size();
    a->products = amg::products_per_apply(H);
    if (p->n == 0) {
        a->lv.clear();
        return CVR_OK;
    }
    try {
        a->lv.resize(L);
    } catch (const std::bad_alloc &) {
        return fail(CVR_ERR_NOMEM, "%s: out of host memory", entry);
    }
    Scratch    s;
    const auto buffer = [&](void **out, size_t bytes, const char *what) {          // zeroed once, counted
        a->buffer_bytes += (int64_t)(bytes ? bytes : 1);
        return zeroed(kEntry, out, bytes, what);
    };
    for (size_t l = 0; l < L; l++) {
        const amg::Level &hl = H.lv[l];
        AmgLevel         &dl = a->lv[l];
        const bool        last = l + 1 == L;
        dl.n = hl.n;
        dl.nc = hl.nc;
        if (l == 0) dl.h = h;
        else if (smoothed) {
            if (last && !H.coarse_direct) {          // (the levels above it got theirs in their coarsening step)
                dl.own = true;
                if (const int rc = make_handle(&dl.h, sb.cur, p->device, 0, a->width)) return rc;
            }
        } else if (!(last && H.coarse_direct)) {
            dl.own = true;
            cvr_csr_view lv{};
            if (const int rc = upload_level(hl, p->is_f32, s, "a level's row_ptr", "a level's col_idx", "a level's values", &lv)) return rc;
            if (const int rc = make_handle(&dl.h, lv, p->device, 0, a->width)) return rc;
        }
        if (smoothed) {
            if (last && !dl.d_dinv)          // (the device set-up has left every level's there)
                if (const int rc = upload(kEntry, &dl.d_dinv, hl.dinv.data(), hl.dinv.size(), "dinv")) return rc;
            // r is R_(l-1)'s output, z is P_(l-1)'s input beside A_l's, t is R_l's input, e is P_l's output; zeroed: the pad slots stay 0
            const AmgLevel *up = l > 0 ? &a->lv[l - 1] : nullptr;
            size_t          rb = vsz * K * (size_t)std::max<int64_t>(hl.n, 1), zb = dl.h ? x_ext_bytes(dl.h, (int)K) : vsz * K * (size_t)(hl.n + 1);
            if (up) rb = std::max(rb, y_ext_bytes(up->hr, (int)K)), zb = std::max(zb, x_bytes_of(up->hp, K));
            if (const int rc = buffer(&dl.d_r, rb, "r")) return rc;
            if (const int rc = buffer(&dl.d_z, zb, "z")) return rc;
            if (const int rc = buffer(&dl.d_q, dl.h ? y_ext_bytes(dl.h, (int)K) : vsz, "q")) return rc;
            if (!last) {
                if (const int rc = buffer(&dl.d_t, x_bytes_of(dl.hr, K), "t")) return rc;
                if (const int rc = buffer(&dl.d_e, y_ext_bytes(dl.hp, (int)K), "e")) return rc;
            }
            continue;
        }
        if (const int rc = upload(kEntry, &dl.d_dinv, hl.dinv.data(), hl.dinv.size(), "dinv")) return rc;
        if (!last) {
            if (const int rc = upload(kEntry, &dl.d_agg, hl.agg.data(), sizeof(int32_t) * hl.agg.size(), "agg")) return rc;
            if (const int rc = upload(kEntry, &dl.d_mrp, hl.mrp.data(), sizeof(int64_t) * hl.mrp.size(), "the aggregates' row_ptr")) return rc;
            if (const int rc = upload(kEntry, &dl.d_mem, hl.mem.data(), sizeof(int32_t) * hl.mem.size(), "the aggregates' members")) return rc;
        }
        // r, z, q, zeroed: z[n] is the pad slot of an SpMV input and is never written again
        if (const int rc = buffer(&dl.d_r, vsz * K * (size_t)std::max<int64_t>(hl.n, 1), "r")) return rc;
        if (const int rc = buffer(&dl.d_z, dl.h ? x_ext_bytes(dl.h, (int)K) : vsz * K * (size_t)(hl.n + 1), "z")) return rc;
        if (const int rc = buffer(&dl.d_q, dl.h ? y_ext_bytes(dl.h, (int)K) : vsz, "q")) return rc;
    }
    if (a->width >= 2) {          // the pads of the single-vector calls: element n of every z and t (at ld = K a block call writes there)
        std::vector<void *> pads;
        try {
            for (size_t l = 0; l < L; l++) {
                pads.push_back(static_cast<uint8_t *>(a->lv[l].d_z) + vsz * (size_t)a->lv[l].n);
                if (a->lv[l].d_t) pads.push_back(static_cast<uint8_t *>(a->lv[l].d_t) + vsz * (size_t)a->lv[l].n);
            }
        } catch (const std::bad_alloc &) {
            return fail(CVR_ERR_NOMEM, "%s: out of host memory", entry);
        }
        a->npads = (int)pads.size();
        if (const int rc = upload(kEntry, &a->d_pads, pads.data(), sizeof(void *) * pads.size(), "the pad list")) return rc;
    }
    if (H.coarse_direct)
        if (const int rc = upload(kEntry, &a->d_winv, H.winv.data(), H.winv.size(), "the coarsest level's inverse")) return rc;
    HIP_TRY(hipDeviceSynchronize());          // (the handles' copies of the levels are complete before the scratch goes; the buffers are zeroed)
    return CVR_OK;
}

template <typename T>
int smooth_more(const AmgLevel &l, int times, hipStream_t st)
{
    for (int k = 0; k < times; k++) {
        HIP_TRY(run_spmv(l.h, l.d_z, l.d_q, st));
        launch_level(amg_smooth_kernel<T>, l.n, st, static_cast<const T *>(l.d_dinv), static_cast<const T *>(l.d_r), static_cast<const T *>(l.d_q), static_cast<T *>(l.d_z), (long long)l.n);
    }
    return CVR_OK;
}

// r_0 = r | the cycle: z_0 holds the result
template <typename T>
int enqueue_cycle(const cvr_precond *pc, const T *r, bool al, hipStream_t st)
{
    const Amg      *a = pc->amg;
    const size_t    L = a->lv.size();
    const int       sweeps = a->H.opt.sweeps;
    const long long n = pc->n;
    if (a->npads > 0) hipLaunchKernelGGL(amg_zero_pads_kernel<T>, dim3(1), dim3(64), 0, st, static_cast<T *const *>(a->d_pads), a->npads);
    with_flags([&](auto AL) { launch(precond_copy_in_kernel<T, AL>, st, r, static_cast<T *>(a->lv[0].d_r), n); }, al);
    HIP_TRY(hipGetLastError());
    for (size_t l = 0; l + 1 < L; l++) {
        const AmgLevel &f = a->lv[l], &c = a->lv[l + 1];
        launch_level(amg_first_kernel<T>, f.n, st, static_cast<const T *>(f.d_dinv), static_cast<const T *>(f.d_r), static_cast<T *>(f.d_z), (long long)f.n);
        if (const int rc = smooth_more<T>(f, sweeps - 1, st)) return rc;
        HIP_TRY(run_spmv(f.h, f.d_z, f.d_q, st));
        if (a->H.smoothed) {
            launch_level(amg_residual_kernel<T>, f.n, st, static_cast<const T *>(f.d_r), static_cast<const T *>(f.d_q), static_cast<T *>(f.d_t), (long long)f.n);
            HIP_TRY(run_spmv(f.hr, f.d_t, c.d_r, st));
        } else
        launch_level(amg_restrict_kernel<T>, f.nc, st, static_cast<const int64_t *>(f.d_mrp), static_cast<const int32_t *>(f.d_mem), static_cast<const T *>(f.d_r), static_cast<const T *>(f.d_q),
                     static_cast<T *>(c.d_r), (long long)f.nc);
    }
    const AmgLevel &last = a->lv[L - 1];
    if (a->H.coarse_direct)
        hipLaunchKernelGGL(amg_dense_kernel<T>, dim3(1), dim3(CVR_AMG_MAX_COARSE), 0, st, static_cast<const T *>(a->d_winv), static_cast<const T *>(last.d_r), static_cast<T *>(last.d_z), (int)last.n);
    else {
        launch_level(amg_first_kernel<T>, last.n, st, static_cast<const T *>(last.d_dinv), static_cast<const T *>(last.d_r), static_cast<T *>(last.d_z), (long long)last.n);
        if (const int rc = smooth_more<T>(last, 2 * sweeps - 1, st)) return rc;
    }
    for (size_t l = L - 1; l-- > 0;) {
        const AmgLevel &f = a->lv[l], &c = a->lv[l + 1];
        if (a->H.smoothed) {
            HIP_TRY(run_spmv(f.hp, c.d_z, f.d_e, st));
            launch_level(amg_correct_kernel<T>, f.n, st, static_cast<const T *>(f.d_e), static_cast<T *>(f.d_z), (long long)f.n, a->H.opt.coarse_scale);
        } else
            launch_level(amg_prolong_kernel<T>, f.n, st, static_cast<const int32_t *>(f.d_agg), static_cast<const T *>(c.d_z), static_cast<T *>(f.d_z), (long long)f.n, a->H.opt.coarse_scale);
        if (const int rc = smooth_more<T>(f, sweeps, st)) return rc;
    }
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

}  // namespace

namespace cvrh {
namespace krylov {

int amg_apply_any(const cvr_precond *p, const void *r, void *z, hipStream_t st)
{
    const Amg *a = p->amg;
    if (!a || p->n == 0) return CVR_OK;
    const bool      ral = ((uintptr_t)r & 15u) == 0, zal = ((uintptr_t)z & 15u) == 0;
    const long long n = p->n;
    if (p->is_f32) {
        if (const int rc = enqueue_cycle<float>(p, static_cast<const float *>(r), ral, st)) return rc;
        with_flags([&](auto AL) { launch(precond_copy_out_kernel<float, AL>, st, static_cast<const float *>(a->lv[0].d_z), static_cast<float *>(z), n); }, zal);
    } else {
        if (const int rc = enqueue_cycle<double>(p, static_cast<const double *>(r), ral, st)) return rc;
        with_flags([&](auto AL) { launch(precond_copy_out_kernel<double, AL>, st, static_cast<const double *>(a->lv[0].d_z), static_cast<double *>(z), n); }, zal);
    }
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}

template <typename T>
int amg_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *spmvs)
{
    const Amg *a = pc->amg;
    if (!a || pc->n == 0) return CVR_OK;
    if (const int rc = enqueue_cycle<T>(pc, r, true, st)) return rc;
    if (spmvs) *spmvs += a->products;
    with_flags([&](auto START) { launch(precond_rz_kernel<T, START, true>, st, r, static_cast<const T *>(a->lv[0].d_z), z, p, (long long)pc->n, part_rz, static_cast<const CgCell *>(cell)); }, start);
    HIP_TRY(hipGetLastError());
    return CVR_OK;
}
void amg_release(cvr_precond *p)
{
    Amg *a = p->amg;
    if (!a) return;
    for (AmgLevel &l : a->lv) {
        if (l.own && l.h) (void)cvr_destroy(l.h);
        if (l.hp) (void)cvr_destroy(l.hp);
        if (l.hr) (void)cvr_destroy(l.hr);
        for (void *buf : {l.d_dinv, l.d_agg, l.d_mrp, l.d_mem, l.d_r, l.d_z, l.d_q, l.d_t, l.d_e, l.d_arp, l.d_aci, l.d_ava, l.d_prp, l.d_pci, l.d_pva})
            if (buf) (void)hipFree(buf);
    }
    if (a->d_winv) (void)hipFree(a->d_winv);
    if (a->d_pads) (void)hipFree(a->d_pads);
    delete a;
    p->amg = nullptr;
}
template int amg_cg_apply<float>(const cvr_precond *, const float *, float *, float *, double *, const void *, bool, hipStream_t, int *);
template int amg_cg_apply<double>(const cvr_precond *, const double *, double *, double *, double *, const void *, bool, hipStream_t, int *);

PrecondOps kAmgOps = {kPrecondAmg, "AMG", amg_apply_any, amg_release, amg_cg_apply<float>, amg_cg_apply<double>};

}  // namespace krylov
}  // namespace cvrh

namespace cvrh {
namespace krylov {

// cvr_precond_amg, cvr_precond_amg_smoothed and cvr_precond_amg_mis2 (width = 0): one constructor, the smoothed kinds with their omega as given;
// cvr_precond_amg_block (width = K): the same behind its own checks of setup and nvec, with its name in the messages and the level-0 handle's checks
int amg_construct(cvr_precond **out, cvr_handle *h, const cvr_csr_view *csr, const cvr_amg_options *opt, int32_t setup, double omega, int32_t width, void *stream)
{
    const Mode  mode = (Mode)setup;
    const bool  smoothed = mode != Mode::kPlain;
    const char *entry = width > 0 ? "cvr_precond_amg_block" : entry_of(mode);
    if (!out || !h || !csr) return fail(CVR_ERR_INVALID, "null argument");
    *out = nullptr;
    cvr_amg_options o;
    cvr_amg_default_options(&o);
    if (opt) o = *opt;
    if (const int rc = amg::check_options(&o, entry)) return rc;
    if (smoothed)
        if (const int rc = amg::check_omega(omega, &omega, entry)) return rc;
    if (csr->nrows != csr->ncols) return fail(CVR_ERR_INVALID, "AMG needs a square matrix (%lld x %lld)", (long long)csr->nrows, (long long)csr->ncols);
    if (csr->nrows < 0) return fail(CVR_ERR_INVALID, "null or negative-size CSR view");
    if (csr->nrows >= (int64_t)0x7fffffff) return fail(CVR_ERR_INVALID, "%s: nrows (%lld) must stay below 2^31 - 1: the rows are the members of the aggregates", entry, (long long)csr->nrows);
    if (const int rc = check_square_preprocessed(h, entry, "an AMG preconditioner needs")) return rc;
    if (h->info.nrows != csr->nrows) return fail(CVR_ERR_INVALID, "%s: the view has nrows = %lld, the handle nrows = %lld", entry, (long long)csr->nrows, (long long)h->info.nrows);
    if ((csr->is_f32 != 0) != (h->vsz == 4)) return fail(CVR_ERR_INVALID, "%s: the view's type is %s, the handle's %s", entry, csr->is_f32 ? "fp32" : "fp64", h->vsz == 4 ? "fp32" : "fp64");
    if (width >= 2) {          // level 0's products are k-wide through the borrowed handle
        if (!cvr_spmm_supported(h))
            return fail(CVR_ERR_STATE, "%s: nvec = %d, but the handle's image is not the plain layout; create it with cvr_options.nvec >= 2 for level 0's k-wide products", entry, width);
        if ((uint64_t)(h->info.ncols + 1) * (uint64_t)width * h->vsz > 0xffffffffull)
            return fail(CVR_ERR_INVALID, "%s: a block of %lld rows of %d values exceeds the 4 GiB a buffer descriptor addresses", entry, (long long)(h->info.ncols + 1), width);
    }
    if (!csr->arrays_on_device) {
        if (const int rc = check_csr(csr, true)) return rc;
        if (const int rc = amg::check_structure(csr->nrows, csr->row_ptr, csr->col_idx, entry)) return rc;
    }
    Range range(entry);
    HIP_TRY(hipSetDevice(h->device));
    cvr_precond *p = new (std::nothrow) cvr_precond;
    Amg         *a = new (std::nothrow) Amg;
    if (!p || !a) {
        delete p;
        delete a;
        return fail(CVR_ERR_NOMEM, "out of host memory");
    }
    p->kind = kPrecondAmg;
    p->ops = width > 0 ? &kAmgBlockOps : &kAmgOps;
    p->multi_width = width;
    p->device = h->device;
    p->n = csr->nrows;
    p->bs = 0;
    p->is_f32 = csr->is_f32 ? 1 : 0;
    p->amg = a;
    a->entry = entry;
    a->width = width;
    a->setup = setup;
    if (const int rc = build(p, h, csr, &o, mode, omega, (hipStream_t)stream)) return abandon(p, rc);
    *out = p;
    return CVR_OK;
}

}  // namespace krylov
}  // namespace cvrh

extern "C" {

int cvr_precond_amg(cvr_precond **out, cvr_handle *h, const cvr_csr_view *csr, const cvr_amg_options *opt, void *stream)
{
    return amg_construct(out, h, csr, opt, CVR_AMG_SETUP_PLAIN, 0.0, 0, stream);
}

int cvr_precond_amg_smoothed(cvr_precond **out, cvr_handle *h, const cvr_csr_view *csr, const cvr_amg_options *opt, double omega, void *stream)
{
    return amg_construct(out, h, csr, opt, CVR_AMG_SETUP_SMOOTHED, omega, 0, stream);
}

int cvr_precond_amg_mis2(cvr_precond **out, cvr_handle *h, const cvr_csr_view *csr, const cvr_amg_options *opt, double omega, void *stream)
{
    return amg_construct(out, h, csr, opt, CVR_AMG_SETUP_MIS2, omega, 0, stream);
}

int cvr_precond_amg_mis2_info(const cvr_precond *p, cvr_amg_mis2_info *info)
{
    if (!p || !info) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondAmg || !p->amg) return fail(CVR_ERR_INVALID, "cvr_precond_amg_mis2_info: the preconditioner is of kind %d, not an AMG object (kind %d)", p->kind, kPrecondAmg);
    amg::fill_mis2_info(p->amg->H, info);
    return CVR_OK;
}

int cvr_precond_amg_smoothed_info(const cvr_precond *p, cvr_amg_smoothed_info *info)
{
    if (!p || !info) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondAmg || !p->amg) return fail(CVR_ERR_INVALID, "cvr_precond_amg_smoothed_info: the preconditioner is of kind %d, not an AMG object (kind %d)", p->kind, kPrecondAmg);
    amg::fill_smoothed_info(p->amg->H, info);
    return CVR_OK;
}

int cvr_precond_amg_export_prolongator(const cvr_precond *p, int32_t level, int64_t *row_ptr, int32_t *col_idx, void *vals)
{
    if (!p) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondAmg || !p->amg) return fail(CVR_ERR_INVALID, "cvr_precond_amg_export_prolongator: the preconditioner is of kind %d, not an AMG object (kind %d)", p->kind, kPrecondAmg);
    if (const int rc = fetch_prolongator(p, level)) return rc;
    return amg::export_prolongator(p->amg->H, level, row_ptr, col_idx, vals, "cvr_precond_amg_export_prolongator");
}

int cvr_precond_amg_info(const cvr_precond *p, cvr_amg_info *info)
{
    if (!p || !info) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondAmg || !p->amg) return fail(CVR_ERR_INVALID, "cvr_precond_amg_info: the preconditioner is of kind %d, not an AMG object (kind %d)", p->kind, kPrecondAmg);
    amg::fill_info(p->amg->H, info);
    return CVR_OK;
}

int cvr_precond_amg_export_level(const cvr_precond *p, int32_t level, int64_t *row_ptr, int32_t *col_idx, void *vals, void *dinv, int32_t *agg, void *winv)
{
    if (!p) return fail(CVR_ERR_INVALID, "null argument");
    if (p->kind != kPrecondAmg || !p->amg) return fail(CVR_ERR_INVALID, "cvr_precond_amg_export_level: the preconditioner is of kind %d, not an AMG object (kind %d)", p->kind, kPrecondAmg);
    if (const int rc = fetch_level(p, level)) return rc;
    return amg::export_level(p->amg->H, level, row_ptr, col_idx, vals, dinv, agg, winv, "cvr_precond_amg_export_level");
}

}  // extern "C"
