// cvr_amg_dev.h -- the AMG object's device half as the two files that run its cycle see it: cvr_amg.hip (the constructors, the set-ups, the
// single-vector cycle) and cvr_amg_block.hip (cvr_precond_amg_block: the K-wide cycle).  What the buffers hold and who writes them: cvr_amg.hip's head.
#pragma once
#include "cvr_precond.h"
#include "cvr_amg.h"

// the elements of a thread of a level kernel: a grid-stride loop, whatever grid the level was given
#define CVR_AMG_ELEMENTS(i, n) for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < (n); i += (long long)gridDim.x * kThreads)

namespace cvrh {
namespace krylov {

// a level kernel's launch: a thread per element (or row) on a grid cut to the level's size
template <typename... P, typename... A>
static void launch_level(void (*kernel)(P...), long long n, hipStream_t st, A... args)
{
    const long long blocks = std::min<long long>((n + kThreads - 1) / kThreads, kBlocks);
    hipLaunchKernelGGL(kernel, dim3((unsigned)std::max<long long>(blocks, 1)), dim3(kThreads), 0, st, args...);
}

struct AmgLevel {
    int64_t     n = 0, nc = 0;
    cvr_handle *h = nullptr;          // level 0: borrowed; a directly solved coarsest level: none
    bool        own = false;
    void       *d_dinv = nullptr, *d_agg = nullptr, *d_mrp = nullptr, *d_mem = nullptr;
    void       *d_r = nullptr, *d_z = nullptr, *d_q = nullptr;
    cvr_handle *hp = nullptr, *hr = nullptr;          // the smoothed kind above the coarsest level: the object's handles of P_l and R_l ...
    void       *d_t = nullptr, *d_e = nullptr;        // ... R_l's input and P_l's output
    void       *d_arp = nullptr, *d_aci = nullptr, *d_ava = nullptr;          // the device set-up (cvr_precond_amg_mis2): the level's CSR (row_ptr[0] = 0) ...
    void       *d_prp = nullptr, *d_pci = nullptr, *d_pva = nullptr;          // ... and P_l's above the coarsest level, kept for the exports
};

struct Amg {
    amg::Hierarchy        H;          // the host's copy: what the info and the export return
    bool                  on_demand = false;          // the device set-up: a level's arrays come to H when an export first asks (fetch_level, fetch_prolongator)
    std::vector<AmgLevel> lv;
    void                 *d_winv = nullptr;
    int                   products = 0;          // of one apply
    // cvr_precond_amg_block (width > 0): every handle of the object's own has the plain layout of cvr_options.nvec = width, every buffer is a
    // row-major block of `width` columns (ld = width; the pad row of an SpMV input lies at row n and is never written).  A single-vector call reads
    // the same buffers at ld = 1, where the pad is element n: d_pads lists those npads elements and the call zeroes them first.
    const char           *entry = "cvr_precond_amg";          // as the constructor's messages begin
    int32_t               width = 0, setup = 0;
    int64_t               buffer_bytes = 0;
    void                 *d_pads = nullptr;
    int                   npads = 0;
};

// cvr_amg.hip: the one constructor behind cvr_precond_amg, _smoothed, _mis2 (width = 0) and cvr_precond_amg_block (width = K >= 1; setup: CVR_AMG_SETUP_*)
CVR_HIDDEN int amg_construct(cvr_precond **out, cvr_handle *h, const cvr_csr_view *csr, const cvr_amg_options *opt, int32_t setup, double omega, int32_t width, void *stream);
// cvr_amg_block.hip: a block object's table (kind 4, with apply_multi and cgm_apply)
CVR_HIDDEN extern PrecondOps kAmgBlockOps;
// cvr_amg.hip: kAmgOps' functions, which a block object's table shares
CVR_HIDDEN int  amg_apply_any(const cvr_precond *p, const void *r, void *z, hipStream_t st);
CVR_HIDDEN void amg_release(cvr_precond *p);
template <typename T> CVR_HIDDEN int amg_cg_apply(const cvr_precond *pc, const T *r, T *z, T *p, double *part_rz, const void *cell, bool start, hipStream_t st, int *spmvs);

}  // namespace krylov
}  // namespace cvrh
