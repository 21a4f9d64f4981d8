// cvr_precond.h -- the preconditioner object as the solvers see it, shared by the files that hold the objects (cvr_precond.hip: block-Jacobi,
// cvr_chebyshev.hip: the Chebyshev kind, cvr_pcg_multi.hip: the k-wide block-Jacobi apply) and the solvers that take one (cvr_cg.hip, cvr_cg_multi.hip,
// cvr_bicgstab.hip, cvr_gmres.hip, cvr_fgmres.hip): the struct with its kind and its table of operations (PrecondOps: one per kind, defined in the kind's file; the
// entry points all kinds share and the CG solver call through it, and nothing branches on the kind but BiCGSTAB and GMRES for ILU(0)'s gated sweeps),
// the block-Jacobi apply of one packet (every solver forms z = W r by this code, so the same r gives the same bits in all of them), the copy and
// r . z kernels the kinds share, the checks every preconditioned entry point makes, and the helpers the constructors build with.  How W is built and
// laid out: cvr_precond.hip's head.  The Chebyshev kind: cvr_chebyshev.hip's head.  The ILU(0) kind (two level-scheduled triangular sweeps, launches
// of their own in every solver): cvr_ilu0.hip's head.  The FSAI kind (two products on the SpMV path through two handles of the object's own):
// cvr_fsai.hip's head.  The AMG kind (one V-cycle: a handle per level, l1-Jacobi sweeps, a segmented sum down and a gather up): cvr_amg.hip's head; its K-wide cycle: cvr_amg_block.hip's.  The multicolour SGS kind (two sweeps of one launch per colour of a graph colouring): cvr_mcsgs.hip's head.
// Where a new kind plugs in: DESIGN.md 5.43.
#pragma once
#include "cvr_krylov.h"

constexpr int32_t kPrecondBlockJacobi = 0, kPrecondChebyshev = 1, kPrecondIlu0 = 2, kPrecondFsai = 3, kPrecondAmg = 4, kPrecondMcSgs = 5;          // cvr_precond::kind

#define CVR_HIDDEN __attribute__((visibility("hidden")))          // calls and data between the library's own files

namespace cvrh {
namespace krylov {
struct Chebyshev;     // cvr_chebyshev.hip: the borrowed handle, the polynomial and the three buffers
struct Ilu0;          // cvr_ilu0.hip: the factors, the two schedules and the launch plans
struct Fsai;          // cvr_fsai.hip: W's pattern, Wa and Wb, the two handles and the three buffers
struct Amg;           // cvr_amg_dev.h: the hierarchy, a handle and three buffers per level
struct McSgs;         // cvr_mcsgs.hip: the colouring, the two parts in perm order, the diagonal and one buffer

// What a kind does behind the entry points all kinds share.
//   apply     z = M r enqueued on `st`, by the object's type (the checks are cvr_precond_apply_device's)
//   release   frees the kind's device memory and its struct (cvr_precond_destroy has set the device and deletes the object itself)
//   cg_apply  "z = M r inside a CG solve", enqueued on `st`: z and the partial sums of r . z into part_rz (set 1 of cg_direction_kernel<T, true>);
//             start: before the state cell exists, p = z as well; otherwise nothing is written once the cell (a CgCell) holds a stop.  r, z and p are
//             the solver's buffers; *spmvs grows by the products enqueued; the solver's T is the object's type (check_precond_pair)
//   apply_multi  Z = M R for a row-major block of nvec columns (cvr_precond_apply_multi_device behind its checks; n == 0 included)
//   cgm_apply    cg_apply for the blocks of batched CG (ld = nvec each): Z = M R and per column the partial sums of r . z into that column's set 1
//                of `part`; lv: the solver's blocks take 16-byte packets; cells: the columns' CgCells; start: P = Z as well, else a column whose
//                cell holds a stop is not written
//   The last three are null where a kind has no block form: the two multi entry points decline such an object (decline_multi).
struct PrecondOps {
    int32_t     kind;
    const char *name;          // as the error texts spell it
    int (*apply)(const cvr_precond *, const void *r, void *z, hipStream_t st);
    void (*release)(cvr_precond *);
    int (*cg_apply_f32)(const cvr_precond *, const float *r, float *z, float *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *spmvs);
    int (*cg_apply_f64)(const cvr_precond *, const double *r, double *z, double *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *spmvs);
    int (*apply_multi)(const cvr_precond *, const void *R, int64_t ldr, void *Z, int64_t ldz, int32_t nvec, hipStream_t st) = nullptr;
    int (*cgm_apply_f32)(const cvr_precond *, const float *R, float *Z, float *P, long long n, int nvec, bool lv, double *part, const void *cells, bool start, hipStream_t st,
                         int *spmvs) = nullptr;
    int (*cgm_apply_f64)(const cvr_precond *, const double *R, double *Z, double *P, long long n, int nvec, bool lv, double *part, const void *cells, bool start, hipStream_t st,
                         int *spmvs) = nullptr;
};
// each in its kind's file; written nowhere (not declared const: a const table would be compiled for the device too, where its functions do not exist)
CVR_HIDDEN extern PrecondOps kBlockJacobiOps, kChebyshevOps, kIlu0Ops, kFsaiOps, kAmgOps, kMcSgsOps;
}
}

// What all kinds have, the block-Jacobi fields the solvers' kernels read directly (0 and null in the other kinds) and the other kinds' own structs
// (the one `kind` names is set)
struct cvr_precond {
    int      device = 0;
    int64_t  n = 0, nblocks = 0, identity_blocks = 0;
    int32_t  bs = 1, is_f32 = 0;
    void    *d_w = nullptr;          // nblocks * bs * bs values of T, every block transposed
    int32_t  kind = kPrecondBlockJacobi;
    int32_t  multi_width = 0;          // an object built for blocks of at most this many columns (cvr_precond_amg_block); 0: whatever the entry point takes
    const cvrh::krylov::PrecondOps *ops = nullptr;          // the kind's table: every constructor sets it beside `kind`
    cvrh::krylov::Chebyshev        *cheb = nullptr;
    cvrh::krylov::Ilu0             *ilu = nullptr;
    cvrh::krylov::Fsai             *fsai = nullptr;
    cvrh::krylov::Amg              *amg = nullptr;
    cvrh::krylov::McSgs            *mcsgs = nullptr;
};

namespace cvrh {
namespace krylov {
namespace {

// The fp64 sums of the packet at e (cnt of its values exist; the others 0): s_i = t_0 + t_1 + .., t_j = double(W[i][j]) * double(r[k bs + j]), left to
// right over the columns of block k that exist.  R: the type of r -- T in the apply, double where GMRES forms x from its fp64 combination.
template <typename T, typename R>
__device__ __forceinline__ void apply_sums(const T *__restrict__ wt, int bs, const R *__restrict__ r, long long n, long long e, int cnt, double (&sv)[kPack<T>])
{
    long long k = e / bs;
    int       il = (int)(e - k * bs);
#pragma unroll
    for (int jj = 0; jj < kPack<T>; jj++) {
        sv[jj] = 0;
        if (jj < cnt) {
            const long long r0 = k * bs;
            const int       m = n - r0 < bs ? (int)(n - r0) : bs;
            const T        *w = wt + r0 * bs + il;
            double          s = (double)w[0] * (double)r[r0];
            for (int j = 1; j < m; j++) s += (double)w[(long long)j * bs] * (double)r[r0 + j];
            sv[jj] = s;
            if (++il == bs) { il = 0; k++; }
        }
    }
}

// z of the packet at e: z_i = T(s_i)
template <typename T>
__device__ __forceinline__ void apply_pack(const T *__restrict__ wt, int bs, const T *__restrict__ r, long long n, long long e, int cnt, T (&zv)[kPack<T>])
{
    double sv[kPack<T>];
    apply_sums<T, T>(wt, bs, r, n, e, cnt, sv);
#pragma unroll
    for (int jj = 0; jj < kPack<T>; jj++) zv[jj] = (T)sv[jj];
}

// What the kinds whose apply ends in a buffer of the object's (FSAI, AMG) put around it: in = r before it, AL: r, the caller's array, is 16-byte
// aligned ...
template <typename T, bool AL>
__global__ __launch_bounds__(kThreads) void precond_copy_in_kernel(const T *__restrict__ r, T *__restrict__ in, long long n)
{
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T v[kPack<T>];
        load_pack<T, AL>(r, e, (int)cnt, v);
        store_pack<T, true>(in, e, (int)cnt, v);
    }
}

// ... and z = zo behind it.  AL: z, the caller's array, is 16-byte aligned
template <typename T, bool AL>
__global__ __launch_bounds__(kThreads) void precond_copy_out_kernel(const T *__restrict__ zo, T *__restrict__ z, long long n)
{
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T v[kPack<T>];
        load_pack<T, true>(zo, e, (int)cnt, v);
        store_pack<T, AL>(z, e, (int)cnt, v);
    }
}

// The same inside cvr_pcg_device: the partial sums of r . z (the term double(r_i) * double(z_i) added in the thread that owns element i in element
// order: pcg_apply_kernel's) and, at the START, p = z; behind a stop nothing is written.  COPY: z = zo as well (FSAI, AMG); without it the apply has
// written the solver's z itself, which is read in place as zo, and the argument z is not used (ILU(0)).
template <typename T, bool START, bool COPY>
__global__ __launch_bounds__(kThreads) void precond_rz_kernel(const T *__restrict__ r, const T *__restrict__ zo, T *__restrict__ z, T *__restrict__ p, long long n,
                                                              double *__restrict__ out, const CgCell *__restrict__ cell)
{
    __shared__ double sh[1][kWaves];
    if constexpr (!START)
        if (cell->stop) return;          // (no workgroup of this kernel sets it)
    double acc[1] = {0};
    CVR_KRYLOV_PACKETS(T, e, cnt) {
        T rv[kPack<T>], zv[kPack<T>];
        load_pack<T, true>(r, e, (int)cnt, rv);
        load_pack<T, true>(zo, e, (int)cnt, zv);
#pragma unroll
        for (int j = 0; j < kPack<T>; j++) if (j < cnt) acc[0] += (double)rv[j] * (double)zv[j];
        if constexpr (COPY) store_pack<T, true>(z, e, (int)cnt, zv);
        if constexpr (START) store_pack<T, true>(p, e, (int)cnt, zv);
    }
    store_partials<1>(acc, out, sh);
}

// what the preconditioned entry points check before any device work and before the handle is looked at, behind their solver's own checks
// (`entry`: "cvr_pcg", "cvr_pbicgstab", ...)
inline int check_precond_args(const cvr_precond *p, const cvr_cg_options *opt, const char *entry)
{
    if (!p) return fail(CVR_ERR_INVALID, "null argument");
    if (opt->minv_dev) return fail(CVR_ERR_INVALID, "%s: minv_dev is set beside a preconditioner object: one preconditioner per call", entry);
    return CVR_OK;
}

// ... and what they ask of the pair, behind check_square_preprocessed
inline int check_precond_pair(const cvr_handle *h, const cvr_precond *p, const char *entry)
{
    if (p->n != h->info.nrows) return fail(CVR_ERR_INVALID, "%s: the preconditioner has n = %lld, the handle nrows = %lld", entry, (long long)p->n, (long long)h->info.nrows);
    if ((p->is_f32 != 0) != (h->vsz == 4))
        return fail(CVR_ERR_INVALID, "%s: the preconditioner's type is %s, the handle's %s", entry, p->is_f32 ? "fp32" : "fp64", h->vsz == 4 ? "fp32" : "fp64");
    if (p->device != h->device) return fail(CVR_ERR_INVALID, "%s: the preconditioner lies on device %d, the handle on device %d", entry, p->device, h->device);
    return CVR_OK;
}

// ... and, behind both, the entry point that takes block-Jacobi objects only (cvr_precond_export)
inline int decline_not_block_jacobi(const cvr_precond *p, const char *entry)
{
    return fail(CVR_ERR_STATE, "%s: the preconditioner is of kind %d (%s): this entry point takes block-Jacobi objects (kind %d) only", entry, p->kind, p->ops->name, kPrecondBlockJacobi);
}
inline int check_block_jacobi(const cvr_precond *p, const char *entry)
{
    if (p->kind != kPrecondBlockJacobi) return decline_not_block_jacobi(p, entry);
    return CVR_OK;
}

// ... or the objects whose table has the block form: an object without it is declined in the words above (block-Jacobi was the first kind with one,
// and the words are pinned), an object built for fewer columns than the call's is CVR_ERR_INVALID
inline int check_multi(const cvr_precond *p, int32_t nvec, const char *entry)
{
    if (!p->ops->apply_multi || !p->ops->cgm_apply_f32 || !p->ops->cgm_apply_f64) return decline_not_block_jacobi(p, entry);
    if (p->multi_width > 0 && nvec > p->multi_width)
        return fail(CVR_ERR_INVALID, "%s: nvec = %d, but the preconditioner was built for blocks of at most %d columns (cvr_precond_amg_block's nvec)", entry, nvec, p->multi_width);
    return CVR_OK;
}

// ... or block-Jacobi and ILU(0) objects: BiCGSTAB and GMRES, which apply M^-1 to one vector at a time
inline int check_block_jacobi_or_ilu0(const cvr_precond *p, const char *entry)
{
    if (p->kind != kPrecondBlockJacobi && p->kind != kPrecondIlu0)
        return fail(CVR_ERR_STATE, "%s: the preconditioner is of kind %d (%s): this entry point takes block-Jacobi and ILU(0) objects (kinds %d and %d) only", entry, p->kind,
                    p->ops->name, kPrecondBlockJacobi, kPrecondIlu0);
    return CVR_OK;
}

}  // namespace

// the CG solver's call of an object's apply: the kind's cg_apply of the solver's type
template <typename T>
static int precond_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *spmvs)
{
    if constexpr (sizeof(T) == 4) return pc->ops->cg_apply_f32(pc, r, z, p, part_rz, cell, start, st, spmvs);
    else return pc->ops->cg_apply_f64(pc, r, z, p, part_rz, cell, start, st, spmvs);
}
// ... and batched CG's: the kind's cgm_apply (behind check_multi)
template <typename T>
static int precond_cgm_apply(const cvr_precond *pc, const T *R, T *Z, T *P, long long n, int nvec, bool lv, double *part, const void *cells, bool start, hipStream_t st, int *spmvs)
{
    if constexpr (sizeof(T) == 4) return pc->ops->cgm_apply_f32(pc, R, Z, P, n, nvec, lv, part, cells, start, st, spmvs);
    else return pc->ops->cgm_apply_f64(pc, R, Z, P, n, nvec, lv, part, cells, start, st, spmvs);
}

// cvr_chebyshev.hip: kChebyshevOps' apply and release.  (The two have been names the library exports since they were cvr_precond.hip's calls into
// that file, and stay so: the list of exported names does not change.)
int  chebyshev_apply(const cvr_precond *p, const void *r, void *z, hipStream_t st);
void chebyshev_release(cvr_precond *p);

// cvr_ilu0.hip: z = U^-1 L^-1 r of an ILU(0) object enqueued on `st` as launches of its own (launches_lower + launches_upper of them, nothing
// else), for the solvers that apply M^-1 to one vector at a time and for cvr_precond_apply_device.  R: the type of r -- T, or double where GMRES
// hands over its fp64 combination.  A sweep kernel returns at its top, having written nothing, when the gate says so: a state cell that holds a
// stop (`stop`: nstop adjacent words, any of them set), or GMRES's guard of the x-forming kernels (`owed`: the words owed and owed_at of its cell;
// the sweep runs only when owed > 0 and lo < owed_at <= hi).  Both null: it always runs.  r must not be the object's own buffer, nor z.
struct Ilu0Gate {
    const int32_t *stop = nullptr;
    int32_t        nstop = 0;
    const int32_t *owed = nullptr;
    int32_t        lo = 0, hi = 0;
};
template <typename T, typename R> CVR_HIDDEN int ilu0_apply(const cvr_precond *pc, const R *r, T *z, const Ilu0Gate &gate, hipStream_t st);
// ... and what GMRES does with M^-1 u: x_i = T(double(x_i) + double(zu_i)) under the gate (one launch on the solvers' grid); al: x is 16-byte aligned
template <typename T> CVR_HIDDEN int ilu0_add_to_x(T *x, const T *zu, long long n, const Ilu0Gate &gate, bool al, hipStream_t st);

// cvr_pcg_multi.hip: kBlockJacobiOps' apply_multi and cgm_apply (Z = W R; the products counted: none)
CVR_HIDDEN int block_jacobi_apply_multi(const cvr_precond *p, const void *R, int64_t ldr, void *Z, int64_t ldz, int32_t nvec, hipStream_t st);
template <typename T>
CVR_HIDDEN int block_jacobi_cgm_apply(const cvr_precond *pc, const T *R, T *Z, T *P, long long n, int nvec, bool lv, double *part, const void *cells, bool start, hipStream_t st, int *spmvs);

// ---- what the constructors build with (cvr_precond.hip).  `entry`: the constructor's name as its messages begin

// hipMalloc of at least one byte: "<entry>: no device memory for <what> (<bytes> bytes)" (CVR_ERR_NOMEM) or "<entry>: hipMalloc of <what>: .."
CVR_HIDDEN int device_alloc(const char *entry, void **out, size_t bytes, const char *what);
// ... with the host's bytes in it, or zeroed (both complete on return)
CVR_HIDDEN int upload(const char *entry, void **out, const void *src, size_t bytes, const char *what);
CVR_HIDDEN int zeroed(const char *entry, void **out, size_t bytes, const char *what);

// device memory that lives for the build only
struct CVR_HIDDEN Scratch {
    std::vector<void *> bufs;
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch()
    {
        for (void *p : bufs)
            if (p) (void)hipFree(p);
    }
};
CVR_HIDDEN int scratch_alloc(const char *entry, Scratch &s, void **out, size_t bytes, const char *what);

// A view of device arrays checked as cvr_create checks one: the row pointers come to the host once (rp_host; copied on `st` and waited for, so what
// the caller enqueued on that stream to produce the arrays is complete before anything reads them), the columns are checked where they lie
CVR_HIDDEN int check_device_view(const char *entry, const cvr_csr_view *c, std::vector<int64_t> &rp_host, hipStream_t st);

// The view with row_ptr and col_idx (with_values: and vals) on the host for an analysis there: the caller's own arrays, checked by check_csr, or
// copies of device arrays behind check_device_view (with_values: the entries row_ptr[0] .. row_ptr[n] - 1 in their places, else 0 .. row_ptr[n] - 1)
struct CVR_HIDDEN HostCsr {
    const int64_t       *rp = nullptr;
    const int32_t       *ci = nullptr;
    const void          *va = nullptr;
    std::vector<int64_t> rp_own;
    std::vector<int32_t> ci_own;
    std::vector<uint8_t> va_own;
};
CVR_HIDDEN int stage_host(const char *entry, const cvr_csr_view *c, HostCsr &h, bool with_values, hipStream_t st);

// a handle of an object's own: cvr_create + cvr_preprocess of a view of device arrays with the default options on the object's device; nvec >= 2:
// with cvr_options.nvec = nvec, the plain layout
CVR_HIDDEN int make_handle(cvr_handle **out, const cvr_csr_view &device_view, int device, int transpose, int nvec = 1);

// The end of a constructor whose build failed with `rc`: destroys the half-made object and returns rc with the build's message still in place
// (cvr_destroy of a half-made handle may write one of its own)
CVR_HIDDEN int abandon(cvr_precond *p, int rc);
}  // namespace krylov
}  // namespace cvrh
