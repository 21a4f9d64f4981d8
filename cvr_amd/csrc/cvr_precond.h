// cvr_precond.h -- the preconditioner object as the solvers see it, shared by the files that hold the objects (cvr_precond.hip: block-Jacobi,
// cvr_chebyshev.hip: the Chebyshev kind, cvr_pcg_multi.hip: the k-wide block-Jacobi apply) and the solvers that take one (cvr_cg.hip, cvr_cg_multi.hip,
// cvr_bicgstab.hip, cvr_gmres.hip): the struct with its kind, the block-Jacobi apply of one packet (every solver forms z = W r by this code, so the same
// r gives the same bits in all of them), the checks every preconditioned entry point makes, and the host calls by which the CG solvers enqueue an
// object's apply.  How W is built and laid out: cvr_precond.hip's head.  The Chebyshev kind: cvr_chebyshev.hip's head.  The ILU(0) kind (two
// level-scheduled triangular sweeps, launches of their own in every solver): cvr_ilu0.hip's head.  The FSAI kind (two products on the SpMV path through
// two handles of the object's own): cvr_fsai.hip's head.  The AMG kind (one V-cycle: a handle per level, l1-Jacobi sweeps, a segmented sum down and a
// gather up): cvr_amg.hip's head.
#pragma once
#include "cvr_krylov.h"

constexpr int32_t kPrecondBlockJacobi = 0, kPrecondChebyshev = 1, kPrecondIlu0 = 2, kPrecondFsai = 3, kPrecondAmg = 4;          // cvr_precond::kind

namespace cvrh {
namespace krylov {
struct Ilu0;          // cvr_ilu0.hip: the factors, the two schedules and the launch plans
struct Fsai;          // cvr_fsai.hip: W's pattern, Wa and Wb, the two handles and the three buffers
struct Amg;           // cvr_amg.hip: the hierarchy, a handle and three buffers per level
}
}

struct cvr_precond {
    int      device = 0;
    int64_t  n = 0, nblocks = 0, identity_blocks = 0;
    int32_t  bs = 1, is_f32 = 0;
    void    *d_w = nullptr;          // nblocks * bs * bs values of T, every block transposed
    int32_t  kind = kPrecondBlockJacobi;
    // kind == kPrecondChebyshev (bs, nblocks and identity_blocks are 0, d_w is null): the borrowed handle, the polynomial, the object's three buffers
    cvr_handle *h = nullptr;
    int32_t     degree = 0;
    double      lmin = 0, lmax = 0, a[CVR_CHEBYSHEV_MAX_DEGREE] = {}, b[CVR_CHEBYSHEV_MAX_DEGREE] = {};
    void       *d_zi = nullptr, *d_q = nullptr, *d_d = nullptr;          // z between the steps (x_ext values, element ncols stays 0), q = A z (y_ext), d (n)
    // kind == kPrecondIlu0 (bs, nblocks and identity_blocks are 0, d_w is null)
    cvrh::krylov::Ilu0 *ilu = nullptr;
    // kind == kPrecondFsai (bs, nblocks and identity_blocks are 0, d_w is null)
    cvrh::krylov::Fsai *fsai = nullptr;
    // kind == kPrecondAmg (bs, nblocks and identity_blocks are 0, d_w is null)
    cvrh::krylov::Amg *amg = nullptr;
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

// ... and, behind both, the entry points that take block-Jacobi objects only
inline int check_block_jacobi(const cvr_precond *p, const char *entry)
{
    if (p->kind == kPrecondAmg)
        return fail(CVR_ERR_STATE, "%s: the preconditioner is of kind %d (AMG): this entry point takes block-Jacobi objects (kind %d) only", entry, p->kind, kPrecondBlockJacobi);
    if (p->kind == kPrecondFsai)
        return fail(CVR_ERR_STATE, "%s: the preconditioner is of kind %d (FSAI): this entry point takes block-Jacobi objects (kind %d) only", entry, p->kind, kPrecondBlockJacobi);
    if (p->kind == kPrecondIlu0)
        return fail(CVR_ERR_STATE, "%s: the preconditioner is of kind %d (ILU(0)): this entry point takes block-Jacobi objects (kind %d) only", entry, p->kind, kPrecondBlockJacobi);
    if (p->kind != kPrecondBlockJacobi)
        return fail(CVR_ERR_STATE, "%s: the preconditioner is of kind %d (Chebyshev): this entry point takes block-Jacobi objects (kind %d) only", entry, p->kind, kPrecondBlockJacobi);
    return CVR_OK;
}

// ... or block-Jacobi and ILU(0) objects: BiCGSTAB and GMRES, which apply M^-1 to one vector at a time
inline int check_block_jacobi_or_ilu0(const cvr_precond *p, const char *entry)
{
    if (p->kind == kPrecondAmg)
        return fail(CVR_ERR_STATE, "%s: the preconditioner is of kind %d (AMG): this entry point takes block-Jacobi and ILU(0) objects (kinds %d and %d) only", entry, p->kind,
                    kPrecondBlockJacobi, kPrecondIlu0);
    if (p->kind == kPrecondFsai)
        return fail(CVR_ERR_STATE, "%s: the preconditioner is of kind %d (FSAI): this entry point takes block-Jacobi and ILU(0) objects (kinds %d and %d) only", entry, p->kind,
                    kPrecondBlockJacobi, kPrecondIlu0);
    if (p->kind != kPrecondBlockJacobi && p->kind != kPrecondIlu0)
        return fail(CVR_ERR_STATE, "%s: the preconditioner is of kind %d (Chebyshev): this entry point takes block-Jacobi and ILU(0) objects (kinds %d and %d) only", entry, p->kind,
                    kPrecondBlockJacobi, kPrecondIlu0);
    return CVR_OK;
}

}  // namespace

// cvr_chebyshev.hip: the Chebyshev kind behind cvr_precond_apply_device (the checks are the caller's) and cvr_precond_destroy
int  chebyshev_apply(const cvr_precond *p, const void *r, void *z, hipStream_t st);
void chebyshev_release(cvr_precond *p);

// "z = M r inside a CG solve", enqueued on `st`: z and the partial sums of r . z into part_rz (set 1 of cg_direction_kernel<T, true>); start: before
// the state cell exists, p = z as well; otherwise nothing is written once the cell (a CgCell) holds a stop.  r, z and p are the solver's buffers.
// *spmvs grows by the products enqueued.  One definition per kind (cvr_precond.hip: pcg_apply_kernel, cvr_chebyshev.hip: the polynomial's steps), for
// float and double; the solver's T is the object's type (check_precond_pair).
// (Hidden: calls between the library's own files.  chebyshev_apply and chebyshev_release above stay visible as they were, so that the list of names
// the library exports only loses the function that went away.)
template <typename T> __attribute__((visibility("hidden"))) int block_jacobi_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st);
template <typename T> __attribute__((visibility("hidden"))) int chebyshev_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *spmvs);
// cvr_ilu0.hip: the sweeps into z, then one kernel on the solvers' grid with the partial sums and, at the start, p = z
template <typename T> __attribute__((visibility("hidden"))) int ilu0_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st);
// cvr_fsai.hip: xin = r, the two products, then one kernel on the solvers' grid with z, the partial sums and, at the start, p = z
template <typename T> __attribute__((visibility("hidden"))) int fsai_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *spmvs);
// cvr_amg.hip: r_0 = r, the cycle, then one kernel on the solvers' grid with z, the partial sums and, at the start, p = z
template <typename T> __attribute__((visibility("hidden"))) int amg_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *spmvs);
template <typename T>
static int precond_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *spmvs)
{
    if (pc->kind == kPrecondAmg) return amg_cg_apply<T>(pc, r, z, p, part_rz, cell, start, st, spmvs);
    if (pc->kind == kPrecondFsai) return fsai_cg_apply<T>(pc, r, z, p, part_rz, cell, start, st, spmvs);
    if (pc->kind == kPrecondIlu0) return ilu0_cg_apply<T>(pc, r, z, p, part_rz, cell, start, st);
    if (pc->kind == kPrecondChebyshev) return chebyshev_cg_apply<T>(pc, r, z, p, part_rz, cell, start, st, spmvs);
    return block_jacobi_cg_apply<T>(pc, r, z, p, part_rz, cell, start, st);
}

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
template <typename T, typename R> __attribute__((visibility("hidden"))) int ilu0_apply(const cvr_precond *pc, const R *r, T *z, const Ilu0Gate &gate, hipStream_t st);
// ... and what GMRES does with M^-1 u: x_i = T(double(x_i) + double(zu_i)) under the gate (one launch on the solvers' grid); al: x is 16-byte aligned
template <typename T> __attribute__((visibility("hidden"))) int ilu0_add_to_x(T *x, const T *zu, long long n, const Ilu0Gate &gate, bool al, hipStream_t st);
__attribute__((visibility("hidden"))) int  ilu0_apply_any(const cvr_precond *p, const void *r, void *z, hipStream_t st);          // by the object's type, no gate
__attribute__((visibility("hidden"))) void ilu0_release(cvr_precond *p);
// cvr_fsai.hip: the FSAI kind behind cvr_precond_apply_device (the checks are the caller's; by the object's type) and cvr_precond_destroy
__attribute__((visibility("hidden"))) int  fsai_apply_any(const cvr_precond *p, const void *r, void *z, hipStream_t st);
__attribute__((visibility("hidden"))) void fsai_release(cvr_precond *p);
// cvr_amg.hip: the same for the AMG kind
__attribute__((visibility("hidden"))) int  amg_apply_any(const cvr_precond *p, const void *r, void *z, hipStream_t st);
__attribute__((visibility("hidden"))) void amg_release(cvr_precond *p);

// cvr_pcg_multi.hip: the same for the blocks of batched CG (block-Jacobi only), Z = W R and per column the partial sums of r . z into that column's
// set 1 of `part`; lv: the library's blocks take 16-byte packets.  cells: the columns' CgCells
template <typename T>
__attribute__((visibility("hidden"))) hipError_t block_jacobi_cgm_apply(const cvr_precond *pc, const T *R, T *Z, T *P, long long n, int nvec, bool lv, double *part, const void *cells, bool start, hipStream_t st);
}  // namespace krylov
}  // namespace cvrh
