/* include/cvr_amd.h -- C ABI of libcvr_amd.so: CVR-format SpMV for MI355X (gfx950), wave64.
 *
 * This is the drop-in boundary for the ONE hot path of puckbee/CVR (/root/reference/spmv.cpp):
 *
 *   reference interface (C++ linkage, void, caller-owned arrays)        replaced by
 *   ------------------------------------------------------------------  ---------------------------
 *   readMatrix(char*, double**, int**, int**, int*, int*, int*)         cvr_mm_read / cvr_mm_free
 *       spmv.cpp:311-535, call site spmv.cpp:1771
 *   fill(double*, int)  (x = 1.0)   spmv.cpp:556-563, call :1788        cvr_fill_x
 *   pre_processing(int Nthrds, ..19 args..)                             cvr_create + cvr_preprocess
 *       spmv.cpp:565-1014, call site spmv.cpp:1857
 *   spmv_compute_kernel(..21 args.., double* h_vec, int Ntimes)         cvr_spmv (host x,y, timed) /
 *       spmv.cpp:1016-1667, call site spmv.cpp:1882                     cvr_spmv_device (async)
 *   the CSR self-check loop + verdict  spmv.cpp:1843-1850, 1916-1938    cvr_csr_spmv_host, cvr_verdict
 *   (nothing: frees are commented out, spmv.cpp:1889-1907)              cvr_destroy
 *
 * Conventions: plain C, POD structs, opaque handle, every entry point returns an int
 * status (0 = ok, <0 = error class) and never exits or throws; the message of the last error of the
 * calling thread is cvr_last_error().  The handle owns all device memory; the caller owns the host
 * CSR / x / y buffers and may free them as soon as the call that received them returns.
 * Calls on one handle must be serialised by the caller; different handles are independent.
 *
 * There is no CPU fallback behind this ABI: without a HIP device every compute entry point returns
 * CVR_ERR_NO_DEVICE.
 */
#ifndef CVR_AMD_H
#define CVR_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVR_OK              0
#define CVR_ERR_INVALID    -1   /* bad argument / malformed CSR                       */
#define CVR_ERR_NO_DEVICE  -2   /* no HIP device, or device index out of range        */
#define CVR_ERR_HIP        -3   /* a HIP runtime call failed (text in cvr_last_error) */
#define CVR_ERR_IO         -4   /* loader: cannot open / not a coordinate matrix      */
#define CVR_ERR_NOMEM      -5
#define CVR_ERR_STATE      -6   /* call out of order (spmv before preprocess ...)     */
#define CVR_ERR_INTERNAL   -7   /* device converter self-check failed                 */

typedef struct cvr_handle cvr_handle;

/* Host CSR as the library reads it.  The arrays are taken LITERALLY: row r owns elements
 * row_ptr[r] .. row_ptr[r+1]-1, and col_idx indexes x directly.  The reference loader's 1-based
 * arrays (numRows+2 row pointers, columns 1..numCols) are therefore passed as a
 * matrix of numRows+1 rows and numCols+1 columns, and its "tail = nItems-1" quirk (Q9) excludes the
 * same last element the reference's CSR loop excludes. */
typedef struct {
    int64_t        nrows;
    int64_t        ncols;     /* x has ncols entries, y has nrows entries                      */
    const int64_t *row_ptr;   /* [nrows+1], non-decreasing, row_ptr[0] >= 0                    */
    const int32_t *col_idx;   /* [row_ptr[nrows]], each in [0, ncols)                          */
    const void    *vals;      /* double[] or float[] by is_f32                                 */
    int32_t        is_f32;    /* 0: fp64 values, x, y    1: fp32 values, x, y (fp32 accumulate) */
    int32_t        arrays_on_device;   /* 0: the three arrays are host memory; 1: device memory of cvr_options.device (a GPU-
                                 * resident caller): all three are checked and copied device to device; from 200 000 rows on
                                 * row_ptr never comes to the host (checked by a kernel, planned where it is), below that it
                                 * comes back once (8 B per row); the struct's size is unchanged (former padding)          */
} cvr_csr_view;

typedef struct {
    int32_t device;            /* HIP device ordinal                                           */
    int32_t steps_per_chunk;   /* S: lane-stream length of one chunk, multiple of 4; 0 = auto  */
    int64_t split_threshold;   /* rows with more remaining nnz than this may be cut at a chunk */
                               /* boundary; 0 = default (16*S; interleaved column panels: 32*S) */
    int32_t xcd_swizzle;       /* 1 (default when <0): contiguous chunk ranges per XCD; 0 off; */
                               /* 2: also consecutive chunks per CU (measured within +-2 %);   */
                               /* 3..6: runs of 2 / 4 / 8 / 16 workgroups dealt over the XCDs  */
                               /* (measured: no gain over 1)                                   */
    int32_t x_window;          /* values of x each workgroup stages in LDS with coalesced loads */
                               /* and serves its gathers from (cut to what fits the 160 KiB of */
                               /* LDS beside the row-sum stage); 0 = off (<0 = default = off)  */
    int32_t waves_per_block;   /* wavefronts (= consecutive chunks) per SpMV workgroup, 1..16; 0 = default (1).  More than */
                               /* one pays only with x_window: the chunks of a workgroup share the staged window          */
    int32_t col_panels;        /* column panels (each with its slice of x L2-resident, partial sums combined by a second
                                  kernel): 1 = off, <0 = auto (only when x is several times the L2), else the count   */
    int32_t value_dict;        /* value dictionary: one byte per slot instead of the value when the matrix has at most
                                  256 distinct values (pattern matrices); <0 = auto (default), 0 = off                */
    int32_t col_phases;        /* column phases: every chunk feeds its rows' non-zeros column range by column range (P equal
                                  ranges), so that chunks running at the same time gather from the same slice of x and that
                                  slice stays in the L2s; the sums of a row's pieces are added up in LDS, every row is still
                                  written once.  For matrices whose chunks are all resident at once and whose x is larger
                                  than an L2 (web-Google: 7.3 MB); needs ascending columns inside every row.  0 / 1 = off,
                                  <0 = auto (default)                                                                     */
    int32_t hub_table;         /* hub table: the columns with the most non-zeros (at most this many; what fits the LDS) get
                                  their x values compacted before every SpMV and staged in LDS by every workgroup (8 chunks),
                                  their gathers become ds_reads.  For power-law matrices whose x does not fit an L2.
                                  0 = off, <0 = auto (default): on when those columns hold >= 50 % of the non-zeros        */
    int32_t narrow_cols;       /* 16-bit column offsets per chunk when every chunk spans fewer than 32 767 columns (banded
                                  matrices; plain layout without value dictionary): 10 instead of 12 bytes per fp64 slot.
                                  0 = off, <0 = auto (default)                                                             */
    int32_t hub_reorder;       /* with a hub table: re-order the whole of x by column popularity before every SpMV (every column
                                  index of the image is the column's rank), so that the popular columns share cache lines.
                                  0 = off, 1 = on, <0 = auto (default): when x is at least 24 MB; never inside column panels   */
    int32_t row_tags16;        /* column phases: the chunk's row of every piece in a 16-bit tag of its own (2 more bytes per slot)
                                  instead of above the column index in the piece's last column word: lifts the limit of
                                  2^(31 - bits of ncols) rows per chunk.  0 = off, 1 = on, <0 = auto (default): when the
                                  chunks the layout wants hold more rows than the column word has room for                  */
    int32_t row_bands;         /* reserved (the 2-D form of round 3 -- row bands, each a resident launch -- was measured and not adopted:
                                  DESIGN.md 5.9).  Leave at the default (<0) or 1; values > 1 are refused with CVR_ERR_INVALID             */
    int32_t piece_max;         /* column phases: (row, phase) segments are cut into pieces of at most this many elements (at the
                                  multiples of it from the chunk's first element), so that no lane sits on one long row's
                                  segment while the others move on to the next column ranges.  A power of two (others are rounded
                                  down).  0 = whole segments,
                                  <0 = auto (default): 8 when the chunks are long enough for a lane to fall a phase behind     */
    int32_t interleave;        /* interleaved chunks: a chunk's non-zeros are dealt to the 64 lanes in COLUMN order (element e of the chunk's
                                  column-sorted list at step e / 64, lane e % 64) instead of one row per lane, so that a gather instruction
                                  reads 64 column-sorted neighbours and lanes share 128-byte lines of x; every slot carries its row, the
                                  rows' sums are accumulated in LDS (four chunks of up to 5 051 rows per workgroup).  For matrices whose x
                                  is far larger than an L2 and whose columns are scattered.  0 = off, 1 = on,
                                  <0 = auto (default): for column panels that run one per XCD and get no hub tables                       */
    int32_t gang;              /* gang chunks (interleaved images only): the chunks of a workgroup are sorted by column TOGETHER and the workgroup's
                                  wavefronts walk the common list in turn (units of two groups), adding into the chunks' accumulators in the list's
                                  order -- a token in LDS passes from unit to unit, so the sums are those of the CSR loop whatever the wavefronts'
                                  timing (bitwise reproducible) -- : four times the non-zeros share the lines of x a gather instruction touches.
                                  0 = off, 1 = on, <0 = auto (default): for interleaved column panels of four wavefronts per workgroup          */
    int32_t nvec;              /* vectors the caller multiplies this matrix by at once (cvr_spmm_device).  0 / 1 (default): the layout rules as
                                  above.  >= 2: the plain layout -- one chunk per workgroup, no window, column phases, column panels, hub table,
                                  re-ordering, interleaved or gang chunks (value dictionary and narrow columns by their own rules) --, the one whose
                                  kernel has a k-wide form; an explicit setting of any of those options beyond off is refused (CVR_ERR_INVALID) */
    int32_t mutable_values;    /* 1: the handle keeps, for every slot of its image, the CSR position its value came from (a u32 per slot: 4 *
                                  cvr_info.nslots device bytes beside the image), so that cvr_update_values_device can write new values of the same
                                  sparsity pattern without converting again.  The value dictionary is then off (value_dict < 0 turns it off, an explicit
                                  value_dict > 0 is refused with CVR_ERR_INVALID), and row_ptr[nrows] must stay below 2^32 - 1 (CVR_ERR_INVALID).
                                  Every other option and rule works as without it.  0 (default): nothing of this; the former reserved[0]     */
    int32_t transpose;         /* 1: cvr_create builds the handle of A^T from the CSR of A it is given (host or device arrays, checked as ever): the CSR T
                                  of A^T -- row j = A's elements of column j in ascending CSR position (duplicates kept in their order), column index =
                                  A's row -- is made on the device by a stable sort and exists only there; the handle is then bit for bit the cvr_create
                                  of T as device arrays with the same options (image, cvr_info but its times, every result).  cvr_info.nrows = A's ncols,
                                  ncols = A's nrows: x holds nrows(A) + 1 values, y ncols(A).  With mutable_values the handle's map points into A's CSR
                                  positions: cvr_update_values* take the array indexed like A's vals.  A's nrows must stay below 2^31 - 1 and
                                  row_ptr[nrows] below 2^32 (CVR_ERR_INVALID before any device work); cvr_create_multi refuses it.  0 (default): A itself.
                                  Other values: CVR_ERR_INVALID.  The former reserved[1]: no reserved word is left in this struct                   */
} cvr_options;
/* Automatic layout: with steps_per_chunk = 0, waves_per_block = 0, x_window < 0 and col_phases < 0 (the defaults) cvr_create
 * looks at the uploaded CSR on the device (are the rows sorted by column? which share of the non-zeros lies near the
 * diagonal?) and, for matrices whose chunks can all be resident at once, picks 6-8 chunks per workgroup sharing a 64-KiB LDS
 * window of x and/or column phases; everything else keeps one chunk per workgroup.  CVR_DEBUG=no_auto_layout in the environment
 * or any explicit value of those four options switches it off.
 * The one profiling knob is not part of this struct: CVR_DEBUG_COL_MASK in the environment (folds the gather onto a 2^k-entry table:
 * wrong results, timing only) is read by cvr_create. */

typedef struct {
    int32_t iters;
    double  mean_s, min_s, max_s;   /* per-SpMV seconds over `iters` timed launches (HIP events): the SpMV alone (compute only)  */
    double  total_s;                /* events around the whole back-to-back loop                      */
    double  h2d_s, d2h_s;           /* host<->device copies of x and y (outside mean_s)               */
    double  median_s;               /* median of the per-SpMV times                                   */
    /* rows sharded over several GPUs (cvr_spmv_multi): one step = every shard's SpMV + the all-gather of y; the slowest device
     * counts.  On one GPU there is no exchange: step_* repeat the compute figures and gather_mean_s is 0. */
    double  step_mean_s, step_min_s, step_median_s, step_max_s;
    double  gather_mean_s;          /* step_mean_s - mean_s: what the exchange adds                   */
} cvr_timing;

typedef struct {
    int64_t nrows, ncols, nnz;
    int32_t is_f32, steps_per_chunk;
    int64_t nchunks;
    int64_t nslots;            /* nchunks * 64 * S  (nnz + one pad slot per empty row + chunk tails) */
    int64_t nshared;           /* rows cut over several chunks (fix-up list length)                   */
    int64_t image_bytes;       /* device bytes of the CVR image incl. descriptors                     */
    int64_t yext_elems;        /* y_ext = [y | dump | 2 carry slots per chunk]                        */
    int64_t x_elems;           /* ncols + 1 : x_ext[ncols] must be 0 (pad slot)                       */
    double  plan_s, upload_s, convert_s;  /* planner (+ panel rule; preprocess_fused: the whole chain up to the converter's end), H2D of the CSR
                                           * (cvr_options.transpose: + the transpose of A on the device, A's upload included),
                                           * device time of segment table + conversion (preprocess_fused: from the planner's first kernel) */
    int32_t col_panels;        /* 1, or the number of column panels the matrix was cut into                          */
    int32_t value_dict;        /* 0, or the number of dictionary entries (distinct values + the pad slots' 0)         */
    int32_t col_phases;        /* 1, or the number of column phases                                                    */
    int32_t waves_per_block;   /* wavefronts (chunks) per SpMV workgroup                                                */
    int32_t x_window;          /* values of x every workgroup stages in LDS (0 = none)                                  */
    int32_t lds_bytes;         /* dynamic LDS of one SpMV workgroup                                                     */
    int64_t nsegments;         /* column phases: (row, phase) segments over all chunks (0 otherwise)                    */
    int64_t chunk_row_cap;     /* column phases: most rows the planner gives a chunk (their sums live in LDS); 0 = none */
    double  near_diagonal_share;   /* automatic layout: share of the non-zeros within a quarter window of the diagonal (0 if not probed) */
    int32_t hub_entries;           /* hub table: columns staged in LDS (0 = none)                                          */
    int32_t narrow_cols;           /* 1: the image stores 16-bit column offsets (narrow chunks)                             */
    int32_t hub_reorder;           /* 1: the image's column indices are popularity ranks, x is re-ordered before every SpMV  */
    int32_t row_tags16;            /* 1: the image carries 16-bit row tags (column phases with long chunks / wide matrices)   */
    double  hub_share;             /* share of the non-zeros in the hub columns that were (or could have been) chosen      */
    double  hub_select_s;          /* the device pass that counted and ranked the columns (0 if not run)                  */
    double  probe_s;               /* automatic layout: the device pass over the CSR (sortedness, near-diagonal share), 0 if not run */
    double  dict_s;                /* the value-dictionary detection pass over the uploaded values (part of upload_s) */
    double  preprocess_wall_s;     /* host wall time of cvr_preprocess: convert_s (device events) + its temporary allocations and the final sync */
    int32_t row_bands;             /* 1, or the number of row bands (resident launches per SpMV)                                           */
    int32_t piece_max;             /* column phases: longest piece of a lane stream (0 = whole (row, phase) segments)                     */
    int32_t spmv_launches;         /* launches of the SpMV kernel one SpMV is made of: 1 (also with column panels that run one per XCD at a
                                      time: all rounds of eight share one grid), or one per panel when each panel runs over the whole chip;
                                      combine / fix-up / hub kernels not counted                                                            */
    int32_t preprocess_fused;      /* 1: cvr_create ran analysis, chunk plan, segment table and conversion as one submission (resident
                                    * layouts, cvr_fused.hip: plan_s covers all of it, the first cvr_preprocess has nothing left to do) */
    int32_t interleave;            /* 1: the image's chunks are interleaved (cvr_options.interleave)                                      */
    int32_t gang;                  /* > 0: gang chunks (cvr_options.gang) -- the wavefronts of a workgroup that walk one common list            */
} cvr_info;

void        cvr_default_options(cvr_options *opt);
const char *cvr_last_error(void);
const char *cvr_version(void);
int         cvr_device_count(void);                     /* 0 when there is no usable HIP device */

/* ---- the handle: one matrix (or one row shard of it) on one GPU ------------------------------ */
/* Validates the CSR, uploads it, looks at it on the device to choose the layout, plans the chunks (on the device from
 * 200 000 rows on, else on the host: the same plan).  (pre_processing's setup half: chunk partition + row search,
 * spmv.cpp:584-694.)  For a single image in the resident layout the tracker loop follows in the same submission of kernels
 * (cvr_info.preprocess_fused): the handle comes back converted, and cvr_preprocess only releases the CSR and reports the times. */
int cvr_create(cvr_handle **out, const cvr_csr_view *csr, const cvr_options *opt);
/* CSR -> CVR64 on the device (the tracker loop, spmv.cpp:711-1000); `seconds` = what the reference
 * prints at spmv.cpp:1009.  Frees the device copy of the CSR unless keep_csr != 0. */
int cvr_preprocess(cvr_handle *h, int keep_csr, double *seconds);
int cvr_get_info(const cvr_handle *h, cvr_info *info);
int cvr_destroy(cvr_handle *h);

/* y = A x.  x_host: ncols values, y_host: nrows values (type by is_f32).  One untimed warm-up launch,
 * then `iters` timed launches; y of the last one is copied back.  (spmv.cpp:1016-1667; unlike the
 * reference, spmv.cpp:1026-1033, nothing the result needs is left outside the timed region.) */
int cvr_spmv(cvr_handle *h, const void *x_host, void *y_host, int iters, cvr_timing *timing);

/* Asynchronous single SpMV on caller-provided device buffers and stream (a hipStream_t passed as
 * void*; NULL is HIP's null stream, cvr_stream(h) is the handle's own).  x_dev must hold info.x_elems values with
 * x_dev[ncols] == 0; y_dev must hold info.yext_elems values (the first nrows are y; the rest is
 * scratch: carry slots of rows cut over chunks).  Rows without
 * non-zeros are written as 0 on every call; y needs no zeroing.  The call makes the handle's device current.  A handle with
 * column panels (info.col_panels > 1) keeps the panels' partial sums in one buffer of its own: launches of such a handle on
 * different streams are ordered one after the other by the library (an event recorded on the stream it leaves when a launch
 * comes on another one; the stream of the earlier launches must still exist then, or the library waits for the device), so they
 * do not overlap.  Launches on one stream are ordered by that stream alone. */
int cvr_spmv_device(cvr_handle *h, const void *x_dev, void *y_dev, void *stream);
/* the same, `n` launches back to back (the Ntimes loop of spmv.cpp:1024 without a host round trip per launch) */
int cvr_spmv_device_repeat(cvr_handle *h, const void *x_dev, void *y_dev, void *stream, int n);

/* Several vectors at once: Y = A X for nvec vectors in one pass over the image (its stream, descriptors and `target` are read once
 * for all of them, and every gather fetches the nvec values of a column that lie side by side).  X_dev: info.x_elems rows of ldx values
 * (row-major; row c holds x_0[c] .. x_{nvec-1}[c]), the first nvec values of row ncols must be 0.  Y_dev: info.yext_elems rows of ldy
 * values; the first nrows rows are Y, the rest is scratch (carry slots of cut rows, per vector).  Values at positions >= nvec of a row
 * of Y are not written, values at positions >= nvec of a row of X are not used.  ldx >= nvec, ldy >= nvec; any alignment of the
 * element type; (ncols + 1) * ldx values must stay within 4 GiB.  Blocks of up to 8 vectors per launch, all on `stream` (NULL = HIP's
 * null stream); makes the handle's device current.  Every column j of Y is bit for bit what cvr_spmv_device computes for X[:, j].
 * Handles whose image is not the plain layout (create them with cvr_options.nvec >= 2) take only nvec = 1 with ldx = ldy = 1, which
 * is cvr_spmv_device; anything else is CVR_ERR_STATE.  Null pointers, nvec < 1, ld < nvec: CVR_ERR_INVALID before any device work. */
int cvr_spmm_device(cvr_handle *h, const void *X_dev, int64_t ldx, void *Y_dev, int64_t ldy, int32_t nvec, void *stream);
/* host X (ncols x nvec, row-major, ld = nvec) and Y (nrows x nvec): copies, one untimed warm-up, `iters` timed launches, as cvr_spmv */
int cvr_spmm(cvr_handle *h, const void *X_host, void *Y_host, int32_t nvec, int iters, cvr_timing *timing);
/* 1: the handle's image runs cvr_spmm_device for any nvec; 0: it only takes nvec = 1 with ldx = ldy = 1 (any layout) */
int cvr_spmm_supported(const cvr_handle *h);
/* y = alpha * A x + beta * y on the device: cvr_spmv_device with the scaling done where each row is written (the SpMV kernel's write-out,
 * the fix-up of rows cut over chunks, the combine pass of column panels): no pass of its own, one read of old y.  Buffers as for
 * cvr_spmv_device: x_dev holds info.x_elems values with x_dev[ncols] == 0; y_dev holds info.yext_elems values, the first nrows are y (input
 * when beta != 0, always output), the rest is scratch.  Arithmetic in the handle's type T: alpha and beta are rounded to T first, then
 * y[i] = (alpha * s_i) + (beta * y_old[i]) with each product and the sum rounded on their own (no fused multiply-add), where s_i is bit for
 * bit the y[i] of cvr_spmv_device for the same x (+0 for rows without non-zeros).  beta == 0: y is not read (NaN or Inf there have no
 * effect) and y[i] = alpha * s_i.  alpha == 0: neither the matrix nor x is read (x may be NULL), y[i] = beta * y_old[i], or +0 when beta is
 * 0 too.  Asynchronous on `stream` (NULL = HIP's null stream), capturable in a HIP graph and ordered with other launches as
 * cvr_spmv_device is.  Every single-GPU handle.  Errors: null handle or y, or null x with alpha != 0: CVR_ERR_INVALID before any device
 * work; a handle before cvr_preprocess: CVR_ERR_STATE. */
int cvr_spmv_scaled_device(cvr_handle *h, double alpha, const void *x_dev, double beta, void *y_dev, void *stream);
/* the same with host x (ncols values) and y (nrows values, in and out); synchronous, one launch, no timing loop */
int cvr_spmv_scaled(cvr_handle *h, double alpha, const void *x_host, double beta, void *y_host);
/* New values for a handle created with cvr_options.mutable_values = 1: the same sparsity pattern, other values.  vals_dev is a device array
 * of the handle's device (double or float by is_f32), indexed exactly like the cvr_csr_view.vals the handle was created from: element i is
 * the value of CSR position i, 0 <= i < row_ptr[nrows].  One kernel writes them into the image (value block of every group, through the
 * handle's position map); every SpMV, SpMM and power-iteration step after it computes with them.  Values are copied bit for bit (NaN, Inf,
 * -0.0 and explicit zeros included, none checked).  Asynchronous on `stream` (NULL = HIP's null stream) and capturable in a HIP graph, like
 * cvr_spmv_device; ordered like the handle's SpMV launches: when the launch before went to another stream the update waits for it, and a
 * launch on a third stream waits for the update.  vals_dev may be reused once the update has run on `stream`.
 * Errors (all checked before any device work): null handle or array CVR_ERR_INVALID; a handle created without mutable_values, one not yet
 * through cvr_preprocess, or one that kept its device CSR (cvr_preprocess with keep_csr != 0: a later cvr_preprocess would convert the
 * creation values again; refreshing the kept CSR is not offered) CVR_ERR_STATE. */
int cvr_update_values_device(cvr_handle *h, const void *vals_dev, void *stream);
/* the same from host memory: copied on the handle's stream, returns when the image holds the new values */
int cvr_update_values(cvr_handle *h, const void *vals_host);
/* 1: cvr_update_values* accept this handle (mutable_values, preprocessed, no kept CSR); 0 otherwise */
int cvr_update_values_supported(const cvr_handle *h);
/* The column-panel count cvr_create chooses for col_panels = -1 (host only, no device needed): 1 unless x is >= 24 MB
 * -- or >= 12 MB and the matrix is too large for the resident layout (more slots or rows than its workgroups hold in one pass) --
 * and the estimated share of x gathers missing a 4-MiB L2 (*l2_miss_estimate, sampled over eight windows of 65 536
 * rows) exceeds 0.17; then one panel per 1.8 MB of missing x, counted in rounds of eight (one panel per XCD at a time: eight up
 * to 27 MB of x, then 8 * ceil(x / 20.8 MB)); doubled once for thin lists (fewer than two non-zeros of a workgroup's list per
 * 128-byte line of a panel's slice of x, and fewer than 0.15 (row, panel) pairs per non-zero).  cvr_create differs from this host
 * rule in what it measures on the device: hub tables (popular columns) widen or drop the panels, unevenly filled panels are
 * doubled, and from 8 MB of x on a matrix whose non-zeros are not near the diagonal is asked the panel question as well.
 * Returns the count (>= 1) or a negative error. */
int cvr_auto_panels(const cvr_csr_view *csr, double *l2_miss_estimate);

/* Optional tuning of steps_per_chunk by measurement: builds the matrix with S = 8, 12, ... 64 on the device, times the
 * SpMV of each (about 1.5 ms of launches per candidate) and returns the fastest; the caller then passes it as
 * cvr_options.steps_per_chunk to cvr_create.  The default rule (steps_per_chunk = 0) needs no tuning on matrices
 * that fill the GPU many times over; on small ones (a row shard of web-Google on one of 8 GPUs) which chunk counts run
 * fastest depends on how the workgroups fall onto the CUs, and measuring beats the rule by 10-20 %.
 * Host arrays are uploaded once and every candidate is built from the device copy; *tuning_s counts as preprocessing time. */
int cvr_tune_steps(const cvr_csr_view *csr, const cvr_options *opt, int32_t *best_steps, double *best_spmv_s, double *tuning_s);
/* The same over the whole layout: besides S = 8 .. 64 with one chunk per workgroup it measures, for matrices small enough,
 * the resident layout (8 or 4 chunks per workgroup, every workgroup on its own CU at once) with and without a 64-KiB LDS
 * window of x and with and without column phases, and returns the fastest set of options in *best (pass it to cvr_create). */
int cvr_tune(const cvr_csr_view *csr, const cvr_options *opt, cvr_options *best, double *best_spmv_s, double *tuning_s);

/* ---- one call = all GPUs of the process ------------------------------------------------------------------
 * In the reference ONE call drives all threads (pre_processing spmv.cpp:1857 -> omp parallel num_threads at :577;
 * spmv_compute_kernel :1882 -> :1034).  The multi-device handle is that for GPUs: it cuts the rows into one contiguous block
 * per device with balanced predicted time (cvr_row_partition_cost: non-zeros plus a cost per row; binary search on row_ptr, the reference's per-thread trick of
 * spmv.cpp:631-667, but at row boundaries, so no row spans devices and nothing is reduced across them), builds one shard
 * handle per device (x replicated), owns the device vectors, the communicators (ncclCommInitAll) and the all-gather of y.
 * A device may be listed several times (CVR_DEVICES=0,0,0 on a one-GPU box): sharding, handles and gather layout stay,
 * device-to-device copies stand in for RCCL, which needs distinct devices. */
typedef struct cvr_multi cvr_multi;
/* bounds[nparts + 1]: rows [bounds[p], bounds[p+1]) go to part p; returns the largest part's row count (>= 0) or < 0 on error.
 * Host only, no device needed.  The one partition rule of this library (the host program, bench.py and cvr_amd/shard.py use it). */
int64_t cvr_row_partition(int64_t nrows, const int64_t *row_ptr, int32_t nparts, int64_t *bounds);
/* The same cut on predicted TIME instead of non-zeros: a row costs its non-zeros plus row_cost_milli / 1000 of a non-zero (its hand-out,
 * its accumulator, its store: a fit over the eight row shards of R-MAT-26, whose kernels ran 851 .. 1 074 us at equal non-zeros --
 * t = 6.33 ns per 1 000 non-zeros + 7.7 ns per 1 000 rows, i.e. 1.22 non-zeros per row; profiles/r03_rank_emulation_rmat26.json).
 * bounds[p] = the first row r with 1000 * nnz(rows before r) + row_cost_milli * r >= 1000 * floor(nnz * p / nparts) + floor(nrows * row_cost_milli * p / nparts).  row_cost_milli = 0 is cvr_row_partition (the
 * reference balances non-zeros only, spmv.cpp:584-627); CVR_ROW_COST_MILLI_DEFAULT is what cvr_create_multi, spmv.cvr and bench.py use
 * (spmv.cvr: CVR_PARTITION=nnz in the environment keeps the reference's rule). */
#define CVR_ROW_COST_MILLI_DEFAULT 1250
int64_t cvr_row_partition_cost(int64_t nrows, const int64_t *row_ptr, int32_t nparts, int32_t row_cost_milli, int64_t *bounds);
/* csr: host arrays of the whole matrix; opt: as for cvr_create (opt->device is ignored; opt->transpose != 0 is refused with CVR_ERR_INVALID
 * before any device work: row shards of A^T would be column shards of A); devices[ndevices]: HIP ordinals */
int cvr_create_multi(cvr_multi **out, const cvr_csr_view *csr, const cvr_options *opt, const int32_t *devices, int32_t ndevices);
int cvr_preprocess_multi(cvr_multi *m, int keep_csr, double *seconds);      /* seconds: the slowest shard's conversion + planning */
/* y = A x through host buffers: x is replicated to every device, every shard computes its rows, the y slices are all-gathered
 * (every device ends up with the whole y), y comes back from the first device's gathered copy.  `iters` timed steps
 * compute-only, then `iters` with the gather (timing->mean_s ... and timing->step_*). */
int cvr_spmv_multi(cvr_multi *m, const void *x_host, void *y_host, int iters, cvr_timing *timing);
int cvr_multi_shards(const cvr_multi *m);                                    /* number of shards (= ndevices) */
int cvr_multi_info(const cvr_multi *m, int32_t shard, cvr_info *info, int64_t *row_begin, int64_t *row_end, int32_t *device);
int cvr_multi_uses_rccl(const cvr_multi *m);                                 /* 1: ncclAllGather; 0: device-to-device copies (or one shard) */
/* shard handles that exist already (loaded from image caches, or built by the caller): adopted by a multi handle, which then owns
 * them; bounds[n + 1], devices[n]; handle g holds rows [bounds[g], bounds[g+1]) and is preprocessed */
int cvr_multi_from_handles(cvr_multi **out, cvr_handle **shards, const int64_t *bounds, const int32_t *devices, int32_t n);
cvr_handle *cvr_multi_handle(cvr_multi *m, int32_t shard);                   /* shard's handle (owned by m), e.g. for cvr_save_image */
int cvr_destroy_multi(cvr_multi *m);

/* ---- rows sharded over GPUs, one process per GPU: the exchange step ------------------------------------
 * The reference's threads share one y in host memory (spmv.cpp:1280-1282, 1640-1649); with one row shard per GPU
 * (contiguous rows, cut at row boundaries, x replicated) the shards' y slices are all-gathered over RCCL / xGMI.
 * RCCL is loaded on first use (dlopen; the instance already in the process, e.g. PyTorch's, is preferred), so
 * single-GPU users never pay for it. */
typedef struct cvr_comm cvr_comm;
#define CVR_COMM_ID_BYTES 128
/* rank 0 calls this and hands the 128 bytes to every rank by its own means (file, socket, torch.distributed) */
int cvr_comm_unique_id(void *id128);
/* collective over all ranks; `device` is this rank's GPU */
int cvr_comm_create(cvr_comm **comm, const void *id128, int nranks, int rank, int device);
int cvr_comm_destroy(cvr_comm *comm);
/* What RCCL itself says about the communicator -- ncclCommCount, ncclCommUserRank, ncclGetVersion (-1 where the loaded library lacks the call):
 * a record of a multi-GPU run can show that the collective saw N ranks.  Any pointer may be NULL. */
int cvr_comm_info(cvr_comm *comm, int *nranks, int *rank, int *rccl_version);
/* one all-gather of `count` values per rank (type by is_f32) on `stream`: recv_dev holds nranks * count values */
int cvr_comm_all_gather(cvr_comm *comm, const void *send_dev, void *recv_dev, int64_t count, int is_f32, void *stream);
/* `n` sharded SpMVs of the fixed-x loop (spmv.cpp:1024), each followed by the all-gather of this rank's y slice
 * (the first max_rows values of y; every rank passes the same max_rows >= its row count).  Step k computes into
 * y_dev[k & 1] and gathers into yall_dev[k & 1] (nranks * max_rows values).  overlap = 0: SpMV and gather follow
 * each other on `stream` (two enqueues per step; the cheapest for the host).  overlap = 1: the gather runs on the
 * communicator's own stream, so the gather of step k overlaps the SpMV of step k + 1, and buffers are reused only
 * after the gather that used them has finished (two events per step: worth it when the gather outlasts the
 * SpMV by more than their cost).  Every rank must pass the same n and overlap.  On return `stream` is ordered after
 * every gather; *last_buf = index of the buffers holding the last step.  y_dev[i] must hold
 * max(info.yext_elems, max_rows) values.  No host synchronisation. */
int cvr_spmv_gather_repeat(cvr_handle *h, cvr_comm *comm, const void *x_dev, void *const y_dev[2], void *const yall_dev[2],
                           int64_t max_rows, int n, int overlap, void *stream, int *last_buf);

/* The iterative caller (power iteration): x <- A x / ||A x||, `iters` times, everything on the device and on `stream`
 * with no host round trip inside the loop; dot products use a fixed reduction tree, so results are bitwise reproducible.
 * x_dev: info.x_elems values, in: the start vector (any non-zero), out: the normalised iterate; x_dev[ncols] stays 0.
 * *lambda = x_k . (A x_k) / x_k . x_k of the last iteration (Rayleigh quotient).  Inside the loop a step's dot products and
 * the scaling of the next x are one pass over the vectors: x is scaled by the norm of the step before (||x|| stays between
 * 1/lambda and lambda), the last iterate is normalised exactly.  comm = NULL: one GPU, the handle holds the whole
 * square matrix.  comm != NULL: the handle holds this rank's row block of a square matrix of ncols rows, bounds[nranks+1]
 * are the row offsets of all blocks, and every iteration all-gathers y over RCCL and rebuilds the replicated x from
 * it -- the one setting where the exchange step is on the critical path.  On one GPU with an image of the resident layout (column
 * phases, no row cut over chunks) the step's dot products and the next iterate come out of the SpMV kernel's write-out: one launch per
 * iteration (web-Google shape: 26 us per iteration, SpMV alone 21).  Synchronises `stream` before returning.
 * (The reference has no such loop: its Ntimes loop, spmv.cpp:1024, recomputes one y.)
 *
 * Arithmetic, T = the handle's type, n = ncols, every operation rounded on its own (no fused multiply-add).  A sum's terms are
 * double(a_i) * double(b_i), each rounded once, added in fp64 in one of the trees below.  inv(s) = 1 / sqrt(s) in fp64 (a correctly
 * rounded square root, then a correctly rounded quotient) where s > 0, and 0 where s is not > 0 (0, negative, NaN).
 *   Start:   x <- T(double(x) * inv(x.x)), the sum by the dense tree.  An all-zero x stays 0 (and every later x, and lambda).
 *   Step k = 0 .. iters-1:  y = A x through cvr_spmv_device's launch path (bit for bit its y for the same x); the three sums x.y, y.y, x.x
 *            of this x and y; then x <- T(double(y) * inv_k) with inv_0 = 1 and inv_k = inv(y.y of step k-1).
 *   Last step (k = iters-1), instead:  x <- T(double(y) * inv(y.y of this step)).
 *   *lambda = x.y / x.x of the last step; 0 for iters == 0 or an x.x that is not > 0.
 *   fp32 handles with iters > 1, after the sums of step 0:  est = sqrt(y.y / x.x) (0 where x.x is not > 0) is read back once.  Unless
 *            1e-15 < est < 1e15 (both strict), the exact mode is entered: x <- T(double(y) * inv(y.y of step 0)) now, and every later step
 *            is y = A x, x.y, x.x, y.y, x <- T(double(y) * inv(y.y of this step)), each sum by the dense tree (three times per step).
 *            fp64 handles and iters <= 1 never enter it.
 *   Dense tree (the start, the exact mode, the sharded loop, and the one-GPU loop where the fused tree below does not apply): thread
 *            g = 256 * workgroup + thread of a 1024 x 256 grid adds the terms g, g + 262 144, ... in order, starting from +0; the 64 lanes
 *            of a wavefront combine by the xor butterfly a += a[lane ^ o], o = 32, 16, 8, 4, 2, 1; thread 0 adds the workgroup's four
 *            wavefronts in order, from +0: 1024 partials.  Of those, lane t of one wavefront adds t, t + 64, ..., t + 960 in order from +0,
 *            and the lanes combine by the same butterfly.
 *   Fused tree (comm == NULL, column phases > 1, not interleaved, no row cut over chunks (info.nshared == 0), no hub table, no column
 *            panels, at most 1024 workgroups = ceil(nchunks / waves_per_block), and CVR_DEBUG=iter_unfused not set): the sums of every
 *            step that is not in the exact mode.  A chunk holds consecutive rows (cvr_export_image: desc[k][0] is its first; every row,
 *            empty ones included, belongs to exactly one chunk).  Lane l of the chunk's wavefront adds the terms of the chunk's rows
 *            l, l + 64, ... in order from +0; the lanes combine by the butterfly; a workgroup adds its wavefronts that have a chunk
 *            (chunks blk * waves_per_block ...) in chunk order, from +0, into cell blk of 1024 cells, the other cells being +0; the
 *            sum over the 1024 cells is the dense tree's last stage.  x itself is the same T(double(y) * inv_k).
 *   The sharded loop reads y as all-gathered, shard p's rows at y[p * max_rows ...] with max_rows the longest shard (row i belongs to the
 *            LAST p with bounds[p] <= i: empty shards own nothing), in the element order of the dense tree: the same bits as one GPU's
 *            dense loop over the same y.  At most 64 shards (CVR_ERR_INVALID beyond). */
int cvr_power_iteration(cvr_handle *h, cvr_comm *comm, const int64_t *bounds, int iters, void *x_dev, double *lambda,
                        double *seconds_per_iter, void *stream);

/* ---- solving A x = b on the device: conjugate gradients, BiCGSTAB and GMRES(m) ------------------------
 * cvr_cg_device / cvr_cg for a symmetric positive definite A, cvr_bicgstab_device / cvr_bicgstab and cvr_gmres_device / cvr_gmres for any nonsingular A,
 * nonsymmetric ones included,
 * held by a single-GPU handle of a square matrix (any layout; fused-preprocess, image-cache, mutable and transposed handles included).  The
 * solvers share the options, the result and the status codes below.  The whole loop runs on the device: the scalars live in a small state cell in device memory, every
 * vector kernel forms the scalar it needs from the partial sums of the kernel before (in every workgroup, in the same order), and the host
 * reads the cell back once per `check_every` iterations.  (The reference has no solver: its Ntimes loop, spmv.cpp:1024, recomputes one y.) */
typedef struct {
    int32_t     max_iters;    /* >= 0; 0: only the initial residual is formed and tested                 */
    int32_t     check_every;  /* iterations enqueued between two read-backs of the state cell; 0 = default */
    double      rtol;         /* stop when ||r||_2 <= rtol * ||b||_2 (recurrence residual); finite, >= 0    */
    const void *minv_dev;     /* NULL, or nrows values of the handle's type: z = minv .* r (Jacobi and the like);
                                 BiCGSTAB: the right preconditioner, p^ = minv .* p and s^ = minv .* s             */
    int32_t     reserved[4];  /* must be 0 (CVR_ERR_INVALID otherwise)                                       */
} cvr_cg_options;

#define CVR_CG_CONVERGED 0
#define CVR_CG_MAX_ITERS 1
#define CVR_CG_BREAKDOWN 2    /* CG: p.Ap <= 0 or not finite: A is not positive definite on the Krylov space;
                                 BiCGSTAB: r^.v, t.t, omega or r^.r zero or not finite;
                                 GMRES: a cycle's start residual not finite, or rho zero or not finite;
                                 LSQR: beta, alpha, rho or phi / rho not finite, or rho zero;
                                 MINRES: alfa or phi / gamma not finite, r2.z negative or not finite, or gamma zero or not finite */

typedef struct {
    int32_t iterations;       /* steps applied to x (BiCGSTAB: a stop at the half step counts as one)     */
    int32_t status;           /* CVR_CG_*                                                                  */
    int32_t spmv_count;       /* SpMV launches enqueued, incl. the initial residual and any behind the stop */
    int32_t reserved;
    double  residual_norm;    /* ||r||_2 of the recurrence at the stop (||s||_2 at a BiCGSTAB half step)   */
    double  b_norm;
    double  seconds;          /* HIP events around everything enqueued                                     */
} cvr_cg_result;

/* max_iters = 1000, check_every = 0 (the default batch: 8 iterations per read-back), rtol = 1e-8, no preconditioner, reserved = 0 */
void cvr_cg_default_options(cvr_cg_options *opt);
/* b_dev and x_dev: nrows values each of the handle's type, in the memory of the handle's device; x_dev is the start vector on entry and the
 * solution on exit.  Neither needs a pad element or a scratch tail: the search direction p (info.x_elems values, p[ncols] == 0) and q = A p
 * (info.yext_elems values), the residual r and (with minv_dev) z are buffers of the library, allocated per call.
 * Arithmetic, T = the handle's type, every operation below rounded on its own (no fused multiply-add):
 *   r = b - A x by one cvr_spmv_scaled_device with alpha = -1, beta = 1 (in T);  z = T(minv * r), or z is r itself without minv_dev;  p = z;
 *   per step: q = A p through cvr_spmv_device's launch path (bit for bit its y for the same p);  alpha = (r.z) / (p.q);
 *     x = T(double(x) + alpha * double(p));  r = T(double(r) - alpha * double(q));  z = T(double(minv) * double(r));
 *     beta = (r.z)_new / (r.z)_old;  p = T(double(z) + beta * double(p)).
 *   The sums p.q, r.z, r.r and b.b are accumulated in fp64 from the rounded T values in a fixed tree (1024 workgroups of 256 threads, each
 *   thread over its 16-byte packets in order, then lanes, wavefronts and workgroups in a fixed order; no atomics): a call gives the same bits
 *   every time, whatever the alignment of b_dev, x_dev and minv_dev (16-byte loads and stores are used where they are 16-byte aligned).
 *   alpha and beta are fp64 quotients of those sums.
 * Stop rule, evaluated on the device after every step (and once for the start vector): sqrt(r.r) <= rtol * sqrt(b.b) is CVR_CG_CONVERGED;
 * p.q <= 0 or not finite is CVR_CG_BREAKDOWN, found before the step is applied, so x stays at the last iterate; max_iters steps without
 * either is CVR_CG_MAX_ITERS with x the last iterate and residual_norm its recurrence residual.  b == 0: x = 0, 0 iterations, converged.
 * A NaN or an Inf in b or among A's values makes p.q of step 0 not finite: CVR_CG_BREAKDOWN with 0 iterations and x untouched (a residual norm
 * that is not finite never counts as converged, although Inf <= rtol * Inf holds).
 * A start vector within the tolerance: 0 iterations, x untouched.
 * check_every: the kernel that finds the stop records it in the state cell, and every later vector kernel of the batch returns without
 * writing, so x, iterations, status and residual_norm are bit for bit the same for every check_every; only spmv_count and seconds differ
 * (the SpMVs behind the stop write only q).  Three vector launches beside the SpMV per step.
 * Ordering: everything is enqueued on `stream` (NULL = HIP's null stream) and the stream is synchronised at every read-back and before the
 * call returns: it cannot be captured in a HIP graph.  A mutable handle's image, column panels' partial sums and a hub table's copy of x are
 * ordered with other launches of the handle as cvr_spmv_device orders them.  Makes the handle's device current.
 * Errors: null handle, b, x, opt or res; max_iters or check_every < 0; rtol negative or not finite; a non-zero reserved word: CVR_ERR_INVALID,
 * before any device work and before the handle is looked at.  nrows != ncols: CVR_ERR_INVALID.  Before cvr_preprocess: CVR_ERR_STATE. */
int cvr_cg_device(cvr_handle *h, const void *b_dev, void *x_dev, const cvr_cg_options *opt, cvr_cg_result *res, void *stream);
/* the same with host b and x (nrows values each; x in and out): copied up, cvr_cg_device on the handle's stream, x copied back.
 * opt->minv_dev stays a device pointer. */
int cvr_cg(cvr_handle *h, const void *b_host, void *x_host, const cvr_cg_options *opt, cvr_cg_result *res);

/* Conjugate gradients for several right-hand sides at once: A X = B for 1 <= nvec <= 8 columns, one cvr_spmm_device pass over the image per
 * step for all of them, four launches per step instead of four per column, one read-back for the block.  (16 columns: two calls.)
 * B_dev and X_dev: row-major blocks of exactly nrows rows of ldb / ldx values of the handle's type (row i holds b_0[i] .. b_{nvec-1}[i]), as
 * cvr_spmm_device's, but without a pad row or a scratch tail; values at positions >= nvec of a row are neither read nor written; any alignment
 * of the element type.  X_dev is the start block on entry and the solution block on exit.  opt->minv_dev is one preconditioner of nrows values,
 * shared by all columns; rtol, max_iters and check_every hold for every column.  res: nvec results.
 * The contract, for every column j: column j of X and res[j].iterations, .status, .residual_norm and .b_norm are bit for bit what cvr_cg_device
 * on the same handle returns for b = B[:, j] and x0 = X[:, j] with the same options -- for every check_every, ldb, ldx and alignment.  The
 * arithmetic is cvr_cg_device's per column (the initial residual is r = T(b - q) with Q = A X0 from the k-wide product, which is what the scaled
 * product with alpha = -1, beta = 1 stores); in the sums the thread that owns a 16-byte packet of rows of a single vector owns those rows of
 * every column and adds each column's terms in the same order, and every (sum, column) has its own 1024 partials in the same tree.
 * res[j].spmv_count is the number of k-wide products the call enqueued, the initial one included, and res[j].seconds the time of the whole
 * call: both are the same in every res[j].
 * Columns are independent: each has its own state cell and stops on its own -- converged, breakdown (p.q <= 0 or not finite; a NaN or an Inf
 * in its b: at step 0 with x untouched), or b == 0 (x = 0).  From then on no kernel writes its slices of X or of the library's blocks; the
 * other columns go on (the product keeps computing all nvec columns; a stopped column's q is written and ignored).  The host loop ends when
 * every column has stopped or at max_iters.
 * Handles: nvec >= 2, or any leading dimension other than 1, needs cvr_spmm_supported(h) (a handle created with cvr_options.nvec >= 2), else
 * CVR_ERR_STATE; nvec = 1 with ldb = ldx = 1 runs on every single-GPU handle through cvr_spmv_device's launch path.  A mutable handle's image
 * is ordered with its updates as cvr_spmm_device orders it.  Ordering otherwise as cvr_cg_device: `stream` is synchronised at every read-back
 * and before the call returns; not capturable in a HIP graph.  The library's blocks (P of ncols + 1 rows with a zero last row, Q and R of
 * info.yext_elems rows, Z with minv_dev; nvec values per row) are allocated per call.
 * Errors, in this order.  Before any device work and before the handle is looked at: cvr_cg_device's argument checks; nvec outside 1..8,
 * ldb < nvec or ldx < nvec: CVR_ERR_INVALID.  Then: before cvr_preprocess: CVR_ERR_STATE; nrows != ncols: CVR_ERR_INVALID; a handle that
 * does not take the block (above): CVR_ERR_STATE; (ncols + 1) * nvec values beyond 4 GiB: CVR_ERR_INVALID. */
int cvr_cg_multi_device(cvr_handle *h, const void *B_dev, int64_t ldb, void *X_dev, int64_t ldx, int32_t nvec, const cvr_cg_options *opt,
                        cvr_cg_result *res, void *stream);
/* the same with host B and X (nrows x nvec each, row-major, ld = nvec; X in and out): copied up, cvr_cg_multi_device on the handle's stream,
 * X copied back.  opt->minv_dev stays a device pointer. */
int cvr_cg_multi(cvr_handle *h, const void *B_host, void *X_host, int32_t nvec, const cvr_cg_options *opt, cvr_cg_result *res);

/* BiCGSTAB for a nonsymmetric A (needs no A^T): right-preconditioned, shadow residual r^ = r0, two SpMVs per step.  b_dev, x_dev, the options, the
 * result, the ordering and the errors are cvr_cg_device's; the buffers of the call are the library's, allocated per call: p, s (and with minv_dev
 * p^, s^) of info.x_elems values whose element ncols stays 0, v, t and r of info.yext_elems values, r^ of nrows values.
 * Arithmetic, T = the handle's type, every operation below rounded on its own (no fused multiply-add), M = diag(minv), p^ is p and s^ is s without
 * minv_dev (no extra buffer, no extra pass):
 *   r = b - A x by one cvr_spmv_scaled_device with alpha = -1, beta = 1 (in T);  r^ = r;  p = r;  p^ = T(minv * p);  rho = r^.r;
 *   per step: v = A p^ through cvr_spmv_device's launch path (bit for bit its y for the same p^);  alpha = rho / (r^.v);
 *     s = T(double(r) - alpha * double(v));  s^ = T(double(minv) * double(s));
 *     if sqrt(s.s) <= rtol * sqrt(b.b):  x = T(double(x) + alpha * double(p^)), CVR_CG_CONVERGED at the half step (counts as one step; residual_norm
 *       is sqrt(s.s)); the test is made behind t = A s^, so that SpMV is enqueued in any case;
 *     t = A s^ (the same path);  omega = (t.s) / (t.t);
 *     x = T((double(x) + alpha * double(p^)) + omega * double(s^));  r = T(double(s) - omega * double(t));
 *     if sqrt(r.r) <= rtol * sqrt(b.b):  CVR_CG_CONVERGED;
 *     rho' = r^.r;  beta = (rho' / rho) * (alpha / omega);  p = T(double(r) + beta * (double(p) - omega * double(v)));  p^ = T(double(minv) * double(p));
 *     rho = rho'.
 *   The sums r^.v, s.s, t.s, t.t, r.r, r^.r and b.b are accumulated in fp64 from the rounded T values in cvr_cg_device's fixed tree (1024 workgroups
 *   of 256 threads, each thread over its 16-byte packets in order, then lanes, wavefronts and workgroups in a fixed order; no atomics): a call gives
 *   the same bits every time, whatever the alignment of b_dev, x_dev and minv_dev.  alpha, omega and beta are fp64 quotients of those sums.
 * Stop rule, evaluated on the device after every half step and step (and once for the start vector): the two tests above are CVR_CG_CONVERGED;
 * r^.v, t.t, omega or rho' zero or not finite is CVR_CG_BREAKDOWN, found before the step or half step is applied (rho': before the next one), so x
 * stays at the last iterate; max_iters steps without either is CVR_CG_MAX_ITERS with x the last iterate and residual_norm its recurrence residual.
 * b == 0: x = 0, 0 iterations, converged.  A start vector within the tolerance: 0 iterations, x untouched.  A residual norm that is not finite
 * never counts as converged: a NaN or an Inf in b makes r^.v of step 0 not finite, CVR_CG_BREAKDOWN with 0 iterations and x untouched.
 * max_iters = 0: the initial residual is formed and tested (spmv_count == 1).
 * check_every: as for cvr_cg_device -- x, iterations, status and residual_norm are bit for bit the same for every check_every; only spmv_count
 * (1 + 2 per step enqueued) and seconds differ.  Five vector launches beside the two SpMVs per step. */
int cvr_bicgstab_device(cvr_handle *h, const void *b_dev, void *x_dev, const cvr_cg_options *opt, cvr_cg_result *res, void *stream);
/* the same with host b and x (nrows values each; x in and out), as cvr_cg.  opt->minv_dev stays a device pointer. */
int cvr_bicgstab(cvr_handle *h, const void *b_host, void *x_host, const cvr_cg_options *opt, cvr_cg_result *res);

/* Restarted GMRES(m) for any nonsingular A: never breaks down on one, its residual estimate never grows, and a cycle of m steps is bounded.  Right-
 * preconditioned (M = diag(minv_dev)), classical Gram-Schmidt applied twice, Givens rotations; one SpMV per step, one more per restart.  `restart` = m,
 * 1 .. CVR_GMRES_MAX_RESTART (an argument: cvr_cg_options.reserved stays 0).  The handles, b_dev, x_dev, the options, the result, the status codes, the
 * ordering ("not capturable in a HIP graph", makes the handle's device current) are cvr_bicgstab_device's.  The buffers of the call are the library's,
 * allocated per call: restart + 1 basis vectors and (with minv_dev) z of info.x_elems values whose element ncols stays 0, w and r of info.yext_elems
 * values.
 * Arithmetic, T = the handle's type; every operation below is rounded on its own (no fused multiply-add); scalars are fp64.  Every sum a.b is
 * cvr_cg_device's fixed tree over the terms double(a_i) * double(b_i), and each sum has its own 1024 partials, so its bits do not depend on how many
 * sums a kernel forms at once.  k = steps done in the call, j = k mod m the step within the cycle.
 *   Start of the call and of every cycle: r = b - A x by one cvr_spmv_scaled_device with alpha = -1, beta = 1 (in T);  bb = b.b (once), rr = r.r,
 *     bnorm = sqrt(bb), rnorm = sqrt(rr).  At the call's start bb == 0: x = 0, CVR_CG_CONVERGED, 0 iterations.  rnorm finite and
 *     rnorm <= rtol * bnorm: CVR_CG_CONVERGED, x untouched by this test, iterations = the steps so far, residual_norm = rnorm.  rnorm not finite:
 *     CVR_CG_BREAKDOWN, x untouched by this cycle (a NaN or an Inf in b: 0 iterations, x untouched), residual_norm = rnorm.  Otherwise
 *     v_0 = T(double(r) / rnorm) and g_0 = rnorm.
 *   Step j: z = T(double(minv) * double(v_j)), or v_j itself without minv_dev (no buffer, no pass);  w = A z through cvr_spmv_device's launch path
 *     (bit for bit its y).
 *     Pass 1: h_i = v_i . w for i = 0..j, all on the same w;  then t = double(w), t = t - h_0 * double(v_0), ..., t = t - h_j * double(v_j) in that
 *       order, w = T(t) (one rounding to T).
 *     Pass 2, the same on the new w: d_i = v_i . w, the same update with d;  then H_i = h_i + d_i.  Always two passes.
 *     ww = w.w;  H_(j+1) = sqrt(ww).
 *     The earlier rotations, i = 0..j-1 in order: t = cs_i * H_i + sn_i * H_(i+1);  H_(i+1) = cs_i * H_(i+1) - sn_i * H_i;  H_i = t.
 *     rho = sqrt(H_j * H_j + H_(j+1) * H_(j+1)).
 *     rho zero or not finite: CVR_CG_BREAKDOWN, found before the step is counted; x is formed from the j columns before it (below; j = 0: x is the
 *       cycle's start); residual_norm = |g_j|.
 *     Otherwise cs_j = H_j / rho, sn_j = H_(j+1) / rho;  R_(i,j) = H_i for i < j, R_(j,j) = rho;  g_(j+1) = -(sn_j * g_j), then g_j = cs_j * g_j.
 *       The step now counts: iterations = k + 1, and the estimate is e = |g_(j+1)|.
 *     e finite and e <= rtol * bnorm: x is formed from j + 1 columns, CVR_CG_CONVERGED with residual_norm = e (H_(j+1) == 0, the lucky breakdown,
 *       gives e == 0 and ends here: v_(j+1) is never formed).
 *     Else, k + 1 == max_iters: x is formed from j + 1 columns, CVR_CG_MAX_ITERS with residual_norm = e.
 *     Else, j + 1 == m: x is formed from m columns and the next cycle starts (above: from the true residual of that x).
 *     Else v_(j+1) = T(double(w) / H_(j+1)) with the unrotated H_(j+1) = sqrt(ww).
 *   Forming x from q columns (q = 0: nothing): for i = q-1 down to 0: t = g_i; for l = i+1..q-1 ascending t = t - R_(i,l) * y_l; y_i = t / R_(i,i).
 *     Per element u = +0; for i = 0..q-1: u = u + y_i * double(v_i);  x = T(double(x) + double(minv) * u), or T(double(x) + u) without minv_dev.
 * max_iters = 0: the start only (spmv_count == 1).  spmv_count = 1 + the steps enqueued + the restarts enqueued (a restart is enqueued in front of the
 * first step of a later cycle, not behind the last step of the call).
 * check_every: x, iterations, status, residual_norm and b_norm are bit for bit the same for every value (a batch may run across a cycle's end, the
 * restart's scaled product included; kernels behind a stop return without writing); only spmv_count and seconds differ.  Five vector launches beside
 * the SpMV per step, whatever j: the sums v_i . w of a pass in one launch, the update of a pass in one launch, and the finish.
 * Errors, in this order, before any device work and before the handle is looked at: cvr_cg_device's argument checks; restart < 1 or
 * restart > CVR_GMRES_MAX_RESTART: CVR_ERR_INVALID ("restart" in cvr_last_error).  Then: before cvr_preprocess: CVR_ERR_STATE; nrows != ncols:
 * CVR_ERR_INVALID; no device memory for the call's buffers: CVR_ERR_NOMEM, nothing allocated. */
#define CVR_GMRES_MAX_RESTART 64
int cvr_gmres_device(cvr_handle *h, const void *b_dev, void *x_dev, int32_t restart, const cvr_cg_options *opt, cvr_cg_result *res, void *stream);
/* the same with host b and x (nrows values each; x in and out), as cvr_cg.  opt->minv_dev stays a device pointer. */
int cvr_gmres(cvr_handle *h, const void *b_host, void *x_host, int32_t restart, const cvr_cg_options *opt, cvr_cg_result *res);

/* ---- a preconditioner the library owns: block-Jacobi, and the conjugate gradients that use it -----------
 * M = the block diagonal of A in blocks of block_size (1 .. CVR_PRECOND_MAX_BLOCK) rows and columns; the object holds W = M^-1, built once on the
 * device and applied by a kernel, z = W r.  It is independent of any handle (built from the CSR view, usable by every handle of the same n, type and
 * device, by several at once) and is not refreshed by cvr_update_values.  T = float or double by csr->is_f32.
 * CSR input: the view is read literally, as cvr_create reads it, and checked as there (CVR_ERR_INVALID: row_ptr decreasing, a column outside
 *   [0, ncols), ...).  arrays_on_device 0 or 1: host arrays are copied up once and released before the call returns, device arrays (memory of `device`)
 *   are read where they lie; row_ptr comes to the host once for the checks, copied on `stream`, which is synchronised before anything else reads the
 *   arrays: a caller that produced them on `stream` needs no synchronisation of its own.  The matrix must be square.
 * Blocks: block k covers rows and columns k*bs .. min(n, (k+1)*bs) - 1; nblocks = ceil(n / bs); n = 0 gives 0 blocks and is valid.  Entry (i, j) of a
 *   block is the fp64 sum of all CSR entries of row i with that column, in CSR order (duplicates are legal); entries outside the blocks are ignored.  A
 *   short last block is completed with the identity, so cvr_precond_export and the apply always see bs x bs.
 * Inverse: each block is inverted in fp64 by Gauss-Jordan elimination with partial pivoting (the largest magnitude of the column from the diagonal
 *   down), rounded once to T and stored; only W is kept.  A block whose elimination meets a pivot that is zero or not finite (an empty row, a NaN, a
 *   singular block), or whose inverse holds a value that is not finite, becomes the identity block and is counted in identity_blocks; the call still
 *   succeeds.
 * Storage: cvr_precond_export returns nblocks * bs * bs values of T, block after block, each row-major, whatever the device layout is (there every
 *   block lies transposed: the loads of neighbouring rows are contiguous).
 * Apply, for row i of block k, m = min(bs, n - k*bs) the columns of the block that exist:
 *     z_i = T(t_0 + t_1 + ... + t_(m-1))   with   t_j = double(W[i][j]) * double(r[k*bs + j]),
 *   summed left to right starting from t_0 (not from +0), every product and every addition rounded on its own (no fused multiply-add).  The columns
 *   and rows a short last block was completed with are never touched: no r and no z beyond n.  The kernel runs on the solvers' grid (1024 workgroups
 *   of 256 threads, a thread over its 16-byte packets of z in order); the result has the same bits every call and for every alignment of r_dev and z_dev.
 * cvr_precond_block_jacobi enqueues on `stream` (NULL = HIP's null stream), synchronises it and makes `device` current; cvr_precond_apply_device
 * only enqueues (r_dev and z_dev: n values of T each in the memory of the object's device, r_dev != z_dev, not overlapping) and makes the object's
 * device current.
 * Errors.  CVR_ERR_INVALID, before any device work: a null argument; block_size outside 1 .. CVR_PRECOND_MAX_BLOCK; nrows != ncols; r_dev == z_dev.
 * CVR_ERR_NO_DEVICE: `device` out of range.  CVR_ERR_NOMEM: an allocation failed (nothing is left allocated).  cvr_precond_destroy(NULL) is CVR_OK. */
typedef struct cvr_precond cvr_precond;
#define CVR_PRECOND_MAX_BLOCK 32
typedef struct {
    int64_t n;
    int32_t block_size, is_f32;
    int64_t nblocks, identity_blocks;
    int32_t device, reserved;
} cvr_precond_info;
int cvr_precond_block_jacobi(cvr_precond **out, const cvr_csr_view *csr, int32_t block_size, int32_t device, void *stream);
int cvr_precond_get_info(const cvr_precond *p, cvr_precond_info *info);
int cvr_precond_export(const cvr_precond *p, void *blocks_host);
int cvr_precond_apply_device(const cvr_precond *p, const void *r_dev, void *z_dev, void *stream);
int cvr_precond_destroy(cvr_precond *p);

/* Conjugate gradients preconditioned by such an object.  Everything cvr_cg_device's text above fixes holds word for word -- the handles, b_dev and
 * x_dev, the options and the result, r = b - A x by the scaled product, the updates of x, r and p, alpha and beta, the fixed-tree sums, the stop rule,
 * b == 0, a start within the tolerance, the non-finite cases, check_every, spmv_count, seconds, the ordering on `stream` -- with z = W r by the apply
 * arithmetic above in place of z = T(minv * r); z is a buffer of the library, allocated per call.  In the sum r.z the thread that owns element i adds
 * the term double(r_i) * double(z_i), in element order, as cvr_cg_device does.  Four vector launches beside the SpMV per step (z is formed by a launch
 * of its own between the update and the direction).
 * The contract that follows: with block_size = 1, x, iterations, status, residual_norm and b_norm are bit for bit what cvr_cg_device returns with
 * minv_dev = the exported W.
 * Errors, in this order.  Before any device work and before the handle is looked at: cvr_cg_device's argument checks; p null; opt->minv_dev != NULL
 * (one preconditioner per call): CVR_ERR_INVALID.  Then: before cvr_preprocess: CVR_ERR_STATE; nrows != ncols: CVR_ERR_INVALID; then, each
 * CVR_ERR_INVALID with cvr_last_error naming the mismatch: p's n differs from the handle's nrows, p's type from the handle's, p's device from the
 * handle's. */
int cvr_pcg_device(cvr_handle *h, const cvr_precond *p, const void *b_dev, void *x_dev, const cvr_cg_options *opt, cvr_cg_result *res, void *stream);
/* the same with host b and x (nrows values each; x in and out), as cvr_cg */
int cvr_pcg(cvr_handle *h, const cvr_precond *p, const void *b_host, void *x_host, const cvr_cg_options *opt, cvr_cg_result *res);

/* ---- a second kind of cvr_precond: the Chebyshev polynomial preconditioner, z = p_d(A) r ---------------
 * For a symmetric positive definite A whose spectrum lies in [lmin, lmax], p_d is the polynomial of `degree` terms (degree - 1 in A) of the Chebyshev
 * iteration for A z = r started from 0: the apply is degree - 1 products through cvr_spmv_device's launch path, each followed by one fused
 * element-wise kernel; it forms no dot product, and its scalars are constants the host computes once.  Block-Jacobi objects are kind 0 and unchanged;
 * this is kind 1.
 * The object borrows `h`, which must outlive it: a preprocessed, square, single-GPU handle of any layout, fp64 or fp32.  Its n, type and device are
 * the handle's.  It owns three device buffers: zi of info.x_elems values, whose element ncols stays 0, q of info.yext_elems values and d of n values.
 * Because it owns these buffers, one object serves one stream at a time: two applies or solves with the same object must not be in flight on
 * different streams.  A mutable handle's new values (cvr_update_values) are followed automatically, every product being the handle's own; the bounds
 * stay as given.
 * Arithmetic, T = the handle's type, scalars fp64, every operation rounded on its own (no fused multiply-add).  On the host, once
 * (cvr_precond_chebyshev_info returns all of it):
 *     theta = (lmax + lmin) / 2;  delta = (lmax - lmin) / 2;  sigma = theta / delta;  rho_0 = 1 / sigma;  c0 = 1 / theta;
 *     for k = 1 .. degree-1:  rho_k = 1 / (2 * sigma - rho_(k-1));  a[k] = rho_k * rho_(k-1);  b[k] = 2 * rho_k / delta;      a[0] = 0, b[0] = c0.
 *   Step 0:       d = T(c0 * double(r));  z = d.
 *   Step k >= 1:  q = A z through cvr_spmv_device's launch path (bit for bit its y for the same z);
 *                 d = T(a[k] * double(d) + b[k] * (double(r) - double(q)));  z = T(double(z) + double(d)).
 *   The last step writes z to the caller's array, earlier steps to the object's zi.  The kernels run on the solvers' grid (1024 workgroups of 256
 *   threads, a thread over its 16-byte packets in order); the result has the same bits every call and for every alignment of r_dev and z_dev.
 * cvr_precond_apply_device takes this kind: it enqueues degree - 1 SpMVs and degree vector launches on `stream`, and only enqueues.
 * cvr_pcg_device and cvr_pcg take this kind: everything cvr_pcg_device's text above fixes holds with this apply in place of z = W r.  The last kernel
 *   of an apply adds the terms of r.z into set 1 as the block-Jacobi apply does (the thread that owns element i, in element order), writes p = z at
 *   the start, and writes nothing once the state cell holds a stop; the earlier kernels and the SpMVs of an apply touch only the object's buffers.
 *   So x, iterations, status, residual_norm and b_norm do not depend on check_every.  spmv_count = 1 + (degree - 1) + degree * (steps enqueued);
 *   3 + degree vector launches per step.  The contract that follows: on an fp64 handle with degree = 1 the result is bit for bit cvr_cg_device's
 *   with minv_dev = n copies of c0.  The handle of the solve may be another one than the object's (same n, type and device: cvr_pcg_device's three
 *   checks): the polynomial is then in the object's matrix.
 *   Bounds that do not enclose the spectrum (lmax too small) make p_d(A) indefinite: r.z or p.q turns negative and the solve ends as
 *   CVR_CG_BREAKDOWN or runs to CVR_CG_MAX_ITERS; it never reports a wrong x as converged, the stop test being on ||r||.
 * cvr_precond_get_info works for both kinds: for this one block_size, nblocks and identity_blocks are 0.  cvr_precond_destroy frees the buffers.
 * cvr_precond_export, cvr_precond_apply_multi_device, cvr_pcg_multi_device / cvr_pcg_multi, cvr_pbicgstab_device / cvr_pbicgstab and
 * cvr_pgmres_device / cvr_pgmres take block-Jacobi objects only: for this kind they return CVR_ERR_STATE behind their other checks, with
 * cvr_last_error naming the kind.
 * Errors of cvr_precond_chebyshev, before any device work: a null argument; degree outside 1 .. CVR_CHEBYSHEV_MAX_DEGREE; bounds that are not finite
 * or not 0 < lmin < lmax: CVR_ERR_INVALID.  Before cvr_preprocess: CVR_ERR_STATE.  nrows != ncols: CVR_ERR_INVALID.  No device memory:
 * CVR_ERR_NOMEM, nothing left allocated.  cvr_precond_chebyshev_info: a null argument, or a block-Jacobi object: CVR_ERR_INVALID. */
#define CVR_CHEBYSHEV_MAX_DEGREE 16
typedef struct {
    int32_t degree, is_f32;
    double  lmin, lmax;
    double  a[CVR_CHEBYSHEV_MAX_DEGREE], b[CVR_CHEBYSHEV_MAX_DEGREE];   /* entries from `degree` on are 0 */
} cvr_chebyshev_info;
int cvr_precond_chebyshev(cvr_precond **out, cvr_handle *h, int32_t degree, double lmin, double lmax);
int cvr_precond_chebyshev_info(const cvr_precond *p, cvr_chebyshev_info *info);
/* Bounds for it from a few power steps.  The start vector is x_i = T(1 + double(uint32(i * 2654435761)) * 2^-32) (the product taken modulo 2^32) in
 * a buffer of the library; cvr_power_iteration(h, NULL, NULL, power_iters, ...) runs from it on `stream` and gives lambda; then
 * *lmax = CVR_CHEBYSHEV_LMAX_FACTOR * lambda and *lmin = *lmax / eig_ratio.  The Rayleigh quotient is a lower bound of lambda_max for a symmetric
 * A, hence the margin; the factor 1.1 and the usual eig_ratio = 30 are the convention of hypre and Ifpack2.  Synchronises `stream`.
 * Errors: a null h, lmin or lmax; power_iters < 0; eig_ratio not finite or not > 1: CVR_ERR_INVALID, before any device work.  Then
 * cvr_power_iteration's (before cvr_preprocess: CVR_ERR_STATE; not square: CVR_ERR_INVALID).  lambda not finite or not > 0 (power_iters = 0, an
 * indefinite or zero matrix): CVR_ERR_STATE, *lmin and *lmax untouched. */
#define CVR_CHEBYSHEV_LMAX_FACTOR 1.1
int cvr_chebyshev_bounds(cvr_handle *h, int32_t power_iters, double eig_ratio, double *lmin, double *lmax, void *stream);

/* ---- a third kind of cvr_precond: ILU(0), z = U^-1 L^-1 r by two level-scheduled triangular solves ------
 * A ~ L U on A's own pattern (no fill): L unit lower triangular, U upper triangular.  Unlike the two kinds above it couples unknowns across the whole
 * matrix, which is what PDE-type systems need: on the 5-point Laplacian it cuts CG's iterations to about a third.  Block-Jacobi objects are kind 0,
 * Chebyshev objects kind 1, both unchanged; this is kind 2.  Like a block-Jacobi object it is independent of any handle (built from the CSR view,
 * usable by every handle of the same n, type and device) and is not refreshed by cvr_update_values.  T = float or double by csr->is_f32.
 * CSR input: read and checked as cvr_precond_block_jacobi reads it (arrays_on_device 0 or 1; row_ptr comes to the host once on `stream`, which is
 *   synchronised before anything else reads the arrays) and, for the analysis, col_idx comes to the host once as well.  In addition, CVR_ERR_INVALID
 *   with cvr_last_error naming the first offending row: the matrix is not square; a row's columns are not strictly increasing (so: sorted, no
 *   duplicates); a row has no diagonal entry.  n = 0 is valid.
 * Analysis, on the host, once, O(nnz).  The level of row i in L is 0 when the row has no entry left of the diagonal, else 1 + the largest level among
 *   those columns; in U the same from the last row backwards over the entries right of the diagonal.  The rows of a level are independent; within a
 *   level they are ordered by row number.  cvr_ilu0_levels_host returns exactly these numbers (pure host code, no device needed: host arrays only,
 *   csr->vals is not read and may be NULL; lower_level and upper_level take n values each, *n_lower and *n_upper the number of levels).
 * Launch plan, per sweep, built once: a level of at least wide_threshold rows is a launch of its own over all its rows; a run of consecutive narrower
 *   levels is ONE launch of ONE workgroup (1024 threads) that walks its levels in order with a workgroup barrier between them.  No kernel ever waits
 *   on another workgroup (no flags, no spinning, no cooperative grid, no graph).  wide_threshold = 512 unless CVR_DEBUG=ilu_wide=<w> is set when the
 *   object is built (w = 1: one launch per level; a huge w: everything merged).  The plan changes launches, never bits.
 * Factorisation, on the device, on L's plan, on an fp64 copy of the values.  For row i, for each k < i of the row in column order:
 *       a_ik = a_ik / a_kk;   then for every j > k of row k that row i has as well:   a_ij = a_ij - a_ik * a_kj,
 *   every operation rounded on its own (no fused multiply-add), so each a_ij has one fixed update order; rounded once to T at the end.  A pivot a_ii
 *   that is zero or not finite: CVR_ERR_STATE, cvr_last_error names the lowest such row, nothing is left allocated.
 *   cvr_precond_ilu0_export writes row_ptr[n] values of T in the CSR's own positions: L strictly below the diagonal (without its unit diagonal), U from
 *   the diagonal up.
 * Apply, G = lanes_per_row lanes per row: G is the power of two from ceil((nnz - n) / (2 n)) up, at least 1 and at most 64, fixed per object.  Lane l
 *   of a row takes the entries l, l + G, .. of the row's part of the sweep's triangle in column order and forms s_l = +0 + t + t' + .. with
 *   t = double(f_ij) * double(v_j), left to right in fp64, every product and addition rounded on its own; the lanes are combined by the xor butterfly
 *   (s += s of lane ^ o for o = G/2 .. 1).  Then
 *       L's sweep:  y_i = T(double(r_i) - s),       v = y;       U's sweep:  z_i = T((double(y_i) - s) / double(u_ii)),   v = z.
 *   y is a buffer of the object, so one object serves one stream at a time (as the Chebyshev kind).  The result has the same bits every call, for every
 *   alignment of r_dev and z_dev and for every ilu_wide.  cvr_precond_apply_device takes this kind: it enqueues launches_lower + launches_upper
 *   launches on `stream` and nothing else, without a read-back.
 * cvr_pcg_device / cvr_pcg take this kind: cvr_pcg_device's text holds with this apply in place of z = W r; one kernel behind the sweeps forms the
 *   partial sums of r.z as the block-Jacobi apply does and, at the start, p = z; behind a stop x, r and p stay untouched (z is scratch).
 *   3 + launches_lower + launches_upper + 1 launches per step; spmv_count as with block-Jacobi.
 * cvr_pbicgstab_device / cvr_pbicgstab and cvr_pgmres_device / cvr_pgmres take this kind: their texts hold with p^ = M^-1 p, s^ = M^-1 s, z_j = M^-1 v_j
 *   by this apply, enqueued as launches of its own where the block-Jacobi apply is.  GMRES forms x from the fp64 combination u by the same two sweeps
 *   with u where L's sweep has double(r) (y_i = T(u_i - s)), the result zu in a buffer of the call, then x_i = T(double(x_i) + double(zu_i)).
 *   A kernel behind a stop writes nothing that reaches x or the result; spmv_count as with block-Jacobi.
 * cvr_precond_get_info works for this kind (block_size, nblocks and identity_blocks are 0); cvr_precond_destroy frees everything.
 * cvr_precond_export, cvr_precond_apply_multi_device and cvr_pcg_multi_device / cvr_pcg_multi decline this kind (the first takes block-Jacobi objects
 * only, the others those and cvr_precond_amg_block's): CVR_ERR_STATE behind their other checks, cvr_last_error naming the kind.
 * cvr_precond_chebyshev_info on this kind: CVR_ERR_INVALID.
 * Errors of cvr_precond_ilu0: a null argument, nrows != ncols: CVR_ERR_INVALID before any device work; `device` out of range: CVR_ERR_NO_DEVICE; the
 * view's checks above: CVR_ERR_INVALID; CVR_ERR_NOMEM: an allocation failed (nothing is left allocated).  cvr_precond_ilu0_info and
 * cvr_precond_ilu0_export: a null argument, or an object of another kind: CVR_ERR_INVALID. */
typedef struct {
    int64_t n, nnz;                            /* nnz = row_ptr[n]                                                          */
    int32_t levels_lower, levels_upper;        /* the number of levels of each sweep                                        */
    int32_t launches_lower, launches_upper;    /* ... and of launches of each sweep per apply                               */
    int32_t max_level_width;                   /* rows of the widest level of either sweep                                  */
    int32_t lanes_per_row;                     /* G                                                                         */
    int32_t wide_threshold;                    /* rows from which a level is a launch of its own                            */
    int32_t is_f32;
    int32_t reserved[8];                       /* 0                                                                         */
} cvr_ilu0_info;
int cvr_precond_ilu0(cvr_precond **out, const cvr_csr_view *csr, int32_t device, void *stream);
int cvr_precond_ilu0_info(const cvr_precond *p, cvr_ilu0_info *info);
int cvr_precond_ilu0_export(const cvr_precond *p, void *vals_host);
int cvr_ilu0_levels_host(const cvr_csr_view *csr, int32_t *lower_level, int32_t *upper_level, int32_t *n_lower, int32_t *n_upper);

/* ---- ILU(0) with Jacobi-swept triangular solves: 2 * sweeps launches per apply, whatever the levels ------
 * The same object as cvr_precond_ilu0's -- kind 2, the same input rules, checks, analysis and factorisation on the device, the same factor bits
 * (cvr_precond_ilu0_export returns them), the same G -- but each exact triangular solve of the apply is replaced by a fixed number s = `sweeps` of
 * Jacobi sweeps on the triangular system (Anzt, Chow, Dongarra 2015; Chow, Patel 2015).  A sweep is one launch over all n rows with every row
 * independent, so an apply is exactly 2 s launches on `stream` and nothing else (none when n = 0), without a read-back, where the exact object needs
 * one launch or one workgroup barrier per level.  s is fixed, so the apply is a fixed linear operator; for a symmetric positive definite A it is
 * symmetric positive definite (U = D L^T: M^-1 = Lt^-T D^-1 Lt^-1 with Lt^-1 = sum over j <= s of (I - L)^j, unit lower triangular), so PCG may use it.
 * Arithmetic.  S_i(v) is the exact apply's row sum over L's part of row i, S'_i(v) over U's part right of the diagonal: G lanes a row, lane l takes
 *   the entries l, l + G, .. in column order from +0 in fp64, every product and addition rounded on its own, the lanes combined by the xor butterfly
 *   G/2 .. 1.  With y(0) = r, read as it is (type T, or double where GMRES hands over its fp64 combination):
 *       L:  y(k)_i = T(double(r_i) - S_i(y(k-1))),                              k = 1 .. s;
 *       U:  z(0)_i = T(double(y(s)_i) / double(u_ii)),   z(k)_i = T((double(y(s)_i) - S'_i(z(k-1))) / double(u_ii)),   k = 1 .. s;   z = z(s).
 *   z(0) is written by the last L launch.  Every sweep reads one array and writes another: y(k) alternates between two buffers of the object, z(k)
 *   between z_dev and a third, z(s) in z_dev for odd and even s; no launch waits on another workgroup.  After k sweeps the rows of L-level < k hold
 *   the exact sweep's bits, after k U sweeps those of U-level <= k: with s >= max(levels_lower, levels_upper - 1) the apply equals the exact
 *   object's bit for bit.
 * Aliasing: r_dev and z_dev must not overlap at all (z_dev holds intermediate sweeps while r_dev is still read), and neither may be memory of the
 *   object.  cvr_precond_apply_device declines r_dev == z_dev as for every kind; cvr_pcg*, cvr_pbicgstab* and cvr_pgmres* pass buffers of their own
 *   that never overlap.  The result has the same bits on every call, for every alignment of r_dev and z_dev.  The buffers are the object's, so one
 *   object serves one stream at a time.
 * Everything the ILU(0) section above says of kind 2 holds with launches_lower = launches_upper = s: cvr_precond_apply_device, cvr_pcg_device /
 *   cvr_pcg (3 + 2 s + 1 launches per step), cvr_pbicgstab* and cvr_pgmres* take the object, under the same stop rules (every sweep launch returns at
 *   its top behind a stop) and with the same spmv_count; cvr_precond_export, cvr_precond_apply_multi_device and cvr_pcg_multi* decline it with
 *   CVR_ERR_STATE.  cvr_precond_ilu0_info works on it and reports launches_lower = launches_upper = s.  CVR_DEBUG=ilu_lanes is honoured as there.
 * Errors of cvr_precond_ilu0_jacobi: a null argument, sweeps < 1 or sweeps > CVR_ILU0_MAX_SWEEPS: CVR_ERR_INVALID before any device work; then
 * cvr_precond_ilu0's.  cvr_precond_ilu0_jacobi_info: a null argument, an object of another kind or one built by cvr_precond_ilu0: CVR_ERR_INVALID. */
#define CVR_ILU0_MAX_SWEEPS 64
typedef struct {
    int64_t n, nnz;                            /* nnz = row_ptr[n]                                                          */
    int32_t sweeps;                            /* s                                                                         */
    int32_t launches_per_apply;                /* 2 s (0 when n = 0)                                                        */
    int32_t lanes_per_row;                     /* G                                                                         */
    int32_t levels_lower, levels_upper;        /* of the exact sweeps: s >= max(levels_lower, levels_upper - 1) is exact    */
    int32_t is_f32;
    int32_t reserved[8];                       /* 0                                                                         */
} cvr_ilu0_jacobi_info;
int cvr_precond_ilu0_jacobi(cvr_precond **out, const cvr_csr_view *csr, int32_t sweeps, int32_t device, void *stream);
int cvr_precond_ilu0_jacobi_info(const cvr_precond *p, cvr_ilu0_jacobi_info *info);

/* ---- a fourth kind of cvr_precond: FSAI, z = Wb^T (Wa r) by two products on the SpMV path --------------
 * The factorised sparse approximate inverse (Kolotilina-Yeremin) of a symmetric positive definite A: M^-1 = W^T D^-1 W with W unit lower triangular
 * on the pattern of A's lower triangle.  Like ILU(0) it couples unknowns across the whole matrix; unlike ILU(0) its apply is no triangular sweep but
 * two sparse products through cvr_spmv_device's launch path, so its cost does not depend on the level structure.  It cuts fewer iterations than
 * ILU(0) (5-point Laplacian 24 x 24: CG 77, FSAI 44, ILU(0) 27).  Kinds 0 .. 2 are unchanged; this is kind 3.  Like an ILU(0) object it is
 * independent of any handle of A and is not refreshed by cvr_update_values.  T = float or double by csr->is_f32.
 * CSR input: read and checked exactly as cvr_precond_ilu0 reads it (host or device arrays; square; the columns of every row strictly increasing; a
 *   diagonal entry in every row; CVR_ERR_INVALID naming the first offending row).  Only entries with column <= row are read: A is taken to be
 *   symmetric with that lower triangle.  n = 0 is valid: no handles are made and an apply enqueues nothing.
 * Arithmetic of the set-up: fp64 on the values converted to double, every operation rounded on its own (no fused multiply-add), results rounded to
 *   T once at the end.
 *   Row pattern.  P = p_0 < ... < p_(m-1) = i: the columns <= i of row i; of more than CVR_FSAI_MAX_ROW the CVR_FSAI_MAX_ROW nearest the diagonal
 *     (the last ones in column order, the diagonal included); such a row counts in truncated_rows.
 *   The small matrix.  S[a][b] for b <= a is the entry (p_a, p_b) of A, found in row p_a by binary search, +0 when absent.
 *   LDL^T, right-looking.  For k = 0 .. m-1:  d_k = S[k][k]; a d_k that is not finite or not > 0 ends the set-up (below); for a > k: s_a = S[a][k],
 *     l_ak = s_a / d_k; for a > k and k < b <= a: S[a][b] = S[a][b] - l_ak * s_b.  So every element is updated in ascending k, one product and one
 *     subtraction each.
 *   Back substitution by columns.  w_(m-1) = 1, w_a = +0 for a < m-1; for b = m-1 down to 1, for a < b: w_a = w_a - l_ba * w_b.  So every w_a is
 *     updated in descending b.
 *   Outputs, on row i's positions of W's CSR:  Wa = T(w_a),  Wb = T(w_a / d_(m-1));  on the diagonal Wa_ii = 1 and Wb_ii = T(1 / d_(m-1)).
 *   W's CSR is the lower pattern after truncation, with its own row_ptr (from 0) and col_idx.  No square root is taken anywhere.
 *   A bad pivot: CVR_ERR_STATE, cvr_last_error names the lowest such row, nothing is left allocated.
 * The set-up runs on the device: lanes_per_row = G lanes of one wavefront work on one row, G the power of two from the object's largest m up, at
 *   least 4 and at most 64, fixed per object; the order above makes the bits independent of G and of the lane mapping.  No kernel waits on another
 *   workgroup.  cvr_fsai_factor_host is the same arithmetic in pure host code (no device needed: host arrays only): it writes W's row_ptr (n + 1),
 *   col_idx, Wa and Wb (room for as many entries as A has with column <= row; row_ptr[n] of them are written) and *bad_row = the lowest row with a
 *   bad pivot (then CVR_ERR_STATE; the arrays hold the rows before it) or -1.
 * The object owns two handles of its own -- cvr_create + cvr_preprocess of (W's pattern, Wa), and of (W's pattern, Wb) with transpose = 1, both from
 *   device arrays with cvr_default_options on `device`, so both are bit for bit what a caller's cvr_create of the exported arrays gives -- and three
 *   buffers: xin of the first handle's x_elems values, t (the first product's output and the second one's input; its element n is zeroed behind the
 *   first product, whose scratch begins there) and zo of the second handle's yext_elems values.  One object serves one stream at a time.
 *   cvr_options.transpose's limits (nrows below 2^31 - 1, fewer than 2^32 entries in W) are CVR_ERR_INVALID.
 * cvr_precond_apply_device takes this kind: it enqueues, in order, a copy kernel on the solvers' grid (xin = r, for every alignment of r_dev), the
 *   first product, the 4- or 8-byte fill of t[n], the second product and a kernel z = zo (for every alignment of z_dev); it only enqueues.  z is bit
 *   for bit the y of the two products through cvr_spmv_device on handles made from the exported arrays.
 * cvr_pcg_device / cvr_pcg take this kind: cvr_pcg_device's text holds with this apply in place of z = W r.  The last kernel also forms the partial
 *   sums of r.z into set 1 as the block-Jacobi apply does and, at the start, p = z; behind a stop it writes nothing; everything before it touches
 *   only the object's buffers.  So x, iterations, status, residual_norm and b_norm do not depend on check_every.
 *   spmv_count = 1 + 2 + 3 * (steps enqueued).
 * cvr_precond_get_info works for this kind (block_size, nblocks and identity_blocks are 0); cvr_precond_destroy frees the handles and the buffers.
 * cvr_precond_export, cvr_precond_apply_multi_device, cvr_pcg_multi_device / cvr_pcg_multi, cvr_pbicgstab_device / cvr_pbicgstab and
 * cvr_pgmres_device / cvr_pgmres decline this kind: CVR_ERR_STATE behind their other checks, cvr_last_error naming the kind.  The *_info and
 * *_export calls of the other kinds return CVR_ERR_INVALID on this kind, and this kind's return it on the others.
 * Errors of cvr_precond_fsai: a null argument, nrows != ncols, nrows >= 2^31 - 1: CVR_ERR_INVALID before any device work; `device` out of range:
 * CVR_ERR_NO_DEVICE; the view's checks above: CVR_ERR_INVALID; CVR_ERR_NOMEM: an allocation failed (nothing is left allocated).
 * cvr_precond_fsai_export writes host arrays: row_ptr (n + 1), col_idx, wa and wb (info.nnz each; may be NULL when nnz is 0). */
#define CVR_FSAI_MAX_ROW 32
typedef struct {
    int64_t n, nnz;                            /* nnz of W                                                                  */
    int32_t max_row, lanes_per_row;            /* the largest m; G                                                          */
    int64_t truncated_rows;                    /* rows with more than CVR_FSAI_MAX_ROW columns <= row                       */
    int32_t is_f32, reserved[9];               /* 0                                                                         */
} cvr_fsai_info;
int cvr_precond_fsai(cvr_precond **out, const cvr_csr_view *csr, int32_t device, void *stream);
int cvr_precond_fsai_info(const cvr_precond *p, cvr_fsai_info *info);
int cvr_precond_fsai_export(const cvr_precond *p, int64_t *row_ptr, int32_t *col_idx, void *wa, void *wb);
int cvr_fsai_factor_host(const cvr_csr_view *csr, int64_t *row_ptr, int32_t *col_idx, void *wa, void *wb, int64_t *bad_row);

/* ---- a fifth kind of cvr_precond: aggregation AMG, one V-cycle on the SpMV path ------------------------
 * Plain (unsmoothed) aggregation algebraic multigrid for a symmetric positive definite A: the only multilevel kind.  The four kinds above are
 * one-level methods, whose step count on a mesh problem grows with the mesh width; a V-cycle's grows far more slowly (5-point Laplacian, PCG steps
 * to 1e-8, plain CG / this kind: 24 x 24: 77 / 27, 40 x 40: 125 / 32, 100 x 100: 307 / 54).  Every level's operator is a handle, the smoother is
 * l1-Jacobi (one product and one element-wise kernel), restriction is a segmented sum and prolongation a gather, because the prolongator is
 * piecewise constant.  Kinds 0 .. 3 are unchanged; this is kind 4.  T = float or double by csr->is_f32.
 * The object borrows `h`, the caller's preprocessed handle of the same matrix (any layout), as a Chebyshev object does: it is used for level 0's
 *   products and must outlive the object; n, type and device are the handle's and must be the view's.  It is not refreshed by cvr_update_values.
 * CSR input: read and checked exactly as cvr_precond_fsai reads it (host or device arrays; square; the columns of every row strictly increasing; a
 *   diagonal entry in every row; CVR_ERR_INVALID naming the first offending row); pattern and values of device arrays come to the host once on
 *   `stream`.  n = 0 is valid: one empty level, an apply enqueues nothing.
 * Set-up, on the host, O(nnz) per level (cvr_amg_setup_host is this very code and needs no device).  fp64 on the values converted to double, every
 *   operation rounded on its own (no fused multiply-add), every stored value rounded to T once.  Level 0 is A.  At level l, in this order:
 *   Smoother diagonal.  a_ii not finite or not > 0: CVR_ERR_STATE, cvr_last_error names the level and the lowest such row, nothing is left
 *     allocated.  d_i = +0 + |a_i0| + |a_i1| + .. in column order; dinv_i = T(1 / d_i).
 *   Stopping.  The level is the coarsest when n_l <= coarse_size or max_levels levels exist.
 *   Strength.  Entry j != i of row i is strong when a_ij != 0 and a_ij * a_ij >= ((strength * strength) * a_ii) * a_jj.
 *   Aggregation, three passes over the rows in ascending order.  1: if i and all its strong neighbours are free they form the next aggregate (a row
 *     without strong neighbours becomes a singleton).  2: a free i with a strong neighbour that pass 1 aggregated joins the aggregate of the one
 *     with the largest |a_ij|, ties to the lowest j; only pass-1 membership counts.  3: a free i forms the next aggregate with its still-free strong
 *     neighbours.  agg[i] is the aggregate of row i.
 *   Stall.  With n_(l+1) aggregates, double(n_(l+1)) > 0.8 * double(n_l): the level is the coarsest and its aggregation is dropped.
 *   Coarse operator.  A_(l+1)(I, J) = +0 + a_ij + .. over i in I ascending, each row's entries in column order, for agg[j] = J; rounded to T once;
 *     the columns of a row ascending; an entry that sums to zero stays.  The next level reads the rounded values.
 *   Coarsest level, n <= CVR_AMG_MAX_COARSE (coarse_direct = 1): the explicit inverse W of its dense matrix, read from the lower triangle (+0 where
 *     the row has no such column).  Right-looking LDL^T in cvr_precond_fsai's order: for k = 0 .. n-1: d_k = S[k][k], not finite or not > 0:
 *     CVR_ERR_STATE naming the level and k; l_ak = S[a][k] / d_k; S[a][b] = S[a][b] - l_ak * S[b][k] for k < b <= a.  Y = L^-1 by columns: Y = I; for
 *     k ascending, a > k, c <= k: Y[a][c] = Y[a][c] - l_ak * Y[k][c].  For j <= i: W_ij = W_ji = T(+0 + t_i + .. + t_(n-1)), t_k = (Y[k][i] / d_k) *
 *     Y[k][j], k ascending.  Otherwise (a stall or max_levels; coarse_direct = 0) the coarsest level is "solved" by 2 * sweeps smoother sweeps.
 * The object owns, per coarse level, the level's arrays on the device and a handle of its own -- cvr_create + cvr_preprocess from device arrays with
 *   cvr_default_options on the object's device, so its products are bit for bit those of a caller's handle of the exported level (a directly solved
 *   coarsest level has no handle) -- and per level the buffers r (n), z (the handle's x_elems values; element n stays 0) and q (yext_elems).  One
 *   object serves one stream at a time.
 * Cycle at level l for the right-hand side r (level 0: the caller's), per element in fp64, each operation rounded on its own, each stored value
 *   rounded to T once; q = A_l z is the level's product through cvr_spmv_device's launch path:
 *     1. z_i = T(dinv_i * r_i).
 *     2. sweeps - 1 times:  q = A_l z;  z_i = T(z_i + dinv_i * (r_i - q_i)).
 *     3. q = A_l z;  r_(l+1)(I) = T(+0 + (r_i - q_i) + ..) over the rows i of I ascending: one kernel, one lane per aggregate, no atomics.
 *     4. z_(l+1) = the cycle at level l + 1.  The coarsest level: z_i = T(t_0 + t_1 + .. + t_(n-1)), t_j = W_ij * r_j, left to right starting from
 *        t_0, when coarse_direct; else step 1 and 2 * sweeps - 1 times step 2.
 *     5. z_i = T(z_i + coarse_scale * z_(l+1)(agg[i])).
 *     6. sweeps times:  q = A_l z;  z_i = T(z_i + dinv_i * (r_i - q_i)).
 *   With sweeps = 1 a level above the coarsest costs two products and four element-wise launches.  Level 0 begins with a copy kernel (r_0 = r_dev)
 *   and ends with one (z_dev = z_0) on the solvers' grid, for every alignment of r_dev and z_dev.  An apply enqueues 2 * sweeps * (levels - 1)
 *   products, and 2 * sweeps - 1 more when the coarsest level is smoothed.
 * cvr_precond_apply_device takes this kind: it only enqueues, reads nothing back, forms no dot product, has no kernel that waits on another
 *   workgroup, and gives the same bits on every call.
 * cvr_pcg_device / cvr_pcg take this kind: cvr_pcg_device's text holds with this apply in place of z = W r.  The last launch writes z, the partial
 *   sums of r.z into set 1 as the block-Jacobi apply does and, at the start, p = z; behind a stop it writes nothing; everything before it touches
 *   only the object's buffers.  So x, iterations, status, residual_norm and b_norm do not depend on check_every.  spmv_count = 1 + P + (1 + P) *
 *   (steps enqueued), P the products of an apply.
 * cvr_precond_get_info works for this kind (block_size, nblocks and identity_blocks are 0); cvr_precond_destroy frees the handles and the buffers.
 * cvr_precond_export, cvr_precond_apply_multi_device, cvr_pcg_multi_device / cvr_pcg_multi, cvr_pbicgstab_device / cvr_pbicgstab and
 * cvr_pgmres_device / cvr_pgmres decline this kind: CVR_ERR_STATE behind their other checks, cvr_last_error naming "kind 4 (AMG)".  (The two multi
 * entry points take a kind-4 object only when cvr_precond_amg_block built it; one of this constructor's is declined as ever.)  The *_info and
 * *_export calls of the other kinds return CVR_ERR_INVALID on this kind, and this kind's return it on the others.
 * Errors of cvr_precond_amg, in this order, before any device work: a null out, h or csr; the options (opt NULL: the defaults; max_levels outside
 * 1 .. CVR_AMG_MAX_LEVELS, coarse_size outside 1 .. CVR_AMG_MAX_COARSE, sweeps outside 1 .. 4, strength not in [0, 1), coarse_scale not finite or
 * not > 0, a reserved word not 0); nrows != ncols, nrows < 0, nrows >= 2^31 - 1: CVR_ERR_INVALID; h before cvr_preprocess: CVR_ERR_STATE; h not
 * square, or its nrows or type not the view's: CVR_ERR_INVALID; the view's checks (host arrays: before any device work): CVR_ERR_INVALID.  Then
 * CVR_ERR_STATE as above, CVR_ERR_NOMEM: an allocation failed (nothing is left allocated).
 * cvr_precond_amg_info fills a cvr_amg_info.  cvr_precond_amg_export_level writes host arrays of level `level` (0 .. levels - 1): row_ptr (n + 1),
 * col_idx and vals (nnz), dinv (n), agg (n; untouched and may be NULL on the coarsest level) and winv (n * n values of T, row-major, symmetric bit
 * for bit; written for a directly solved coarsest level only and may be NULL otherwise).
 * cvr_amg_setup_host is the pure-host set-up (host arrays only): it returns a cvr_amg_hierarchy with the same levels byte for byte, read by
 * cvr_amg_hierarchy_info and cvr_amg_hierarchy_export_level (the arguments of the two calls above) and released by cvr_amg_hierarchy_destroy.  On
 * CVR_ERR_STATE *bad_level and *bad_row name the level and the row (else -1) and no hierarchy is returned. */
#define CVR_AMG_MAX_LEVELS 16
#define CVR_AMG_MAX_COARSE 256
typedef struct {
    int32_t max_levels;                        /* 1 .. CVR_AMG_MAX_LEVELS, default 16                                       */
    int32_t coarse_size;                       /* 1 .. CVR_AMG_MAX_COARSE, default 64: stop coarsening at n_l <= this       */
    int32_t sweeps;                            /* 1 .. 4, default 1: pre- = post-smoothing sweeps                           */
    int32_t reserved0;                         /* must be 0                                                                 */
    double  strength;                          /* 0 <= s < 1, default 0.08                                                  */
    double  coarse_scale;                      /* finite, > 0, default 1.0: factor on the coarse correction                 */
    int32_t reserved[8];                       /* must be 0                                                                 */
} cvr_amg_options;
typedef struct {
    int32_t levels;                            /* 1 .. max_levels                                                           */
    int32_t coarse_direct;                     /* 1: the coarsest level applies its dense inverse; 0: 2 * sweeps sweeps     */
    int32_t sweeps, is_f32;
    int32_t max_levels, coarse_size;           /* the options the object was built with ...                                 */
    double  strength, coarse_scale;
    double  operator_complexity;               /* the sum of the levels' nnz over level 0's (0 when that is 0)              */
    int64_t n[CVR_AMG_MAX_LEVELS];             /* rows of level l; entries from `levels` on are 0                           */
    int64_t nnz[CVR_AMG_MAX_LEVELS];
    int32_t reserved[8];                       /* 0                                                                         */
} cvr_amg_info;
typedef struct cvr_amg_hierarchy cvr_amg_hierarchy;
int cvr_amg_default_options(cvr_amg_options *opt);
int cvr_precond_amg(cvr_precond **out, cvr_handle *h, const cvr_csr_view *csr, const cvr_amg_options *opt, void *stream);
int cvr_precond_amg_info(const cvr_precond *p, cvr_amg_info *info);
int cvr_precond_amg_export_level(const cvr_precond *p, int32_t level, int64_t *row_ptr, int32_t *col_idx, void *vals, void *dinv, int32_t *agg, void *winv);
int cvr_amg_setup_host(cvr_amg_hierarchy **out, const cvr_csr_view *csr, const cvr_amg_options *opt, int32_t *bad_level, int64_t *bad_row);
int cvr_amg_hierarchy_info(const cvr_amg_hierarchy *hier, cvr_amg_info *info);
int cvr_amg_hierarchy_export_level(const cvr_amg_hierarchy *hier, int32_t level, int64_t *row_ptr, int32_t *col_idx, void *vals, void *dinv, int32_t *agg, void *winv);
int cvr_amg_hierarchy_destroy(cvr_amg_hierarchy *hier);

/* ---- the fifth kind with a smoothed prolongator: smoothed-aggregation AMG, Galerkin products by the SpGEMM ----
 * A second way to build a kind-4 object.  With the piecewise-constant prolongator above the PCG step count still grows with the mesh (5-point
 * Laplacian to 1e-8: 27, 32, 54 steps on 24 x 24, 40 x 40, 100 x 100); one damped l1-Jacobi step on that prolongator, P_l = (I - omega D_l^-1 A_l) T_l,
 * makes it nearly mesh-independent (14, 16, 18 steps) at an operator complexity of about 1.4 against 1.26.  T_l is the tentative prolongator of the
 * aggregation (one 1.0 per row, in column agg[i]); D_l is the l1 diagonal the object computes anyway (1 / dinv): by Gershgorin the spectral radius of
 * D_l^-1 A_l is at most 1, so no eigenvalue estimate is needed.  The coarse operator is A_(l+1) = P_l^T (A_l P_l), two sparse products.
 * cvr_precond_amg, cvr_amg_setup_host and their structs are unchanged; the smoothed kind has entry points of its own.  The object is of kind 4:
 * everything said above of the borrowed handle, the CSR input, n = 0, one stream at a time, cvr_precond_get_info, cvr_precond_destroy, the entry
 * points that decline kind 4 (naming "kind 4 (AMG)") and the cross-kind calls holds for it, and cvr_precond_amg_info / cvr_precond_amg_export_level
 * (and their hierarchy twins) work on it unchanged: reserved words 0, agg the tentative aggregation.
 * omega: 0.0 means the default 4/3 (the literal 4.0 / 3.0; on the Laplacian the usual 4 / (3 rho) of the plain diagonal); any other value must be
 *   finite with 0 < omega < 2.
 * Set-up.  fp64 on the values converted to double, every operation rounded on its own (no fused multiply-add), every stored value rounded to T
 *   once; products "by the SpGEMM contract" are cvr_spgemm_create's C = A B: structural pattern (an entry that cancels to 0.0 stays), rows
 *   ascending, acc = +0, acc = T(acc + T(a * b)) in ascending position of the left row.  At level l the smoother diagonal, the stopping rule, the
 *   strength test, the aggregation and the stall rule are those above, in that order, unchanged.  Then:
 *   1. T_l as a CSR of n_l x n_(l+1): row_ptr = 0 .. n_l, col_idx[i] = agg[i], vals[i] = 1.
 *   2. G = A_l T_l by the SpGEMM contract.  Row i holds column agg[i], since row i of A_l has a diagonal entry.
 *   3. P_l on G's pattern: w_i = omega * double(dinv_i);  p_ij = T(t_ij - w_i * double(g_ij)) with t_ij = 1.0 for j == agg[i] and 0.0 otherwise:
 *      omega times dinv first, that times g second, the subtraction third.  A g_ij that is 0.0 keeps its entry in P_l.
 *   4. R_l = P_l^T as a CSR of n_(l+1) x n_l: row J holds P_l's entries of column J in ascending row of P_l (a stable transpose; values copied).
 *   5. A_(l+1) = R_l (A_l P_l): two products by the SpGEMM contract, so every value is a fixed-order sum with one rounding in T per product and per
 *      addition.  Its rows are ascending and every row has a diagonal entry (P_l's column J is not empty), so the structure rules hold for the next
 *      level.  A_(l+1) is symmetric only to rounding: R_l (A_l P_l) and its transpose sum the same terms in another order.  That is accepted: the
 *      dense inverse reads the lower triangle only, the strength test is per entry, and PCG meets a preconditioner that is symmetric to rounding.
 *   The coarsest level is treated as above (the dense inverse for n <= CVR_AMG_MAX_COARSE, else 2 * sweeps sweeps).
 * cvr_amg_smoothed_setup_host does steps 2 and 5 with cvr_spgemm_host and the rest in host loops.  cvr_precond_amg_smoothed does steps 1 - 5 on
 *   the device: agg and dinv are uploaded, steps 1 and 3 are kernels of a thread per row, step 4 is cvr_options.transpose's device transpose, steps
 *   2 and 5 are cvr_spgemm_create on device arrays (CVR_DEBUG=spgemm_limits applies; it never changes a bit).  A level's arrays stay on the device
 *   for the handles and come to the host once per level, for the next level's aggregation (host code) and for the exports.  Host and device SpGEMM
 *   give the same bits, so the object's levels and prolongators are the host twin's byte for byte.  Failures as above: CVR_ERR_STATE naming level
 *   and row, nothing left allocated; a CVR_ERR_NOMEM of a product propagates.
 * The object owns what a plain one owns (the members of the aggregates excepted) and, per level above the coarsest, a handle of P_l (n_l x n_(l+1))
 *   and a handle of R_l (made from the transposed arrays, not with transpose = 1), both cvr_create + cvr_preprocess from device arrays with
 *   cvr_default_options: their products are bit for bit those of a caller's handle of the exported arrays.  Beside r, z and q a level has t (R_l's
 *   x: x_elems values, element n_l stays 0) and e (P_l's y: yext_elems values); r_(l+1) is R_l's y (yext_elems) and z_(l+1) is P_l's x and
 *   A_(l+1)'s (the larger x_elems; element n_(l+1) stays 0).  No buffer is one product's y and another one's x: a y-scratch tail never meets a pad.
 * Cycle: steps 1, 2, 4 and 6 of the cycle above, and in place of steps 3 and 5:
 *     3'. q = A_l z;  t_i = T(r_i - q_i);  r_(l+1) = R_l t through cvr_spmv_device's launch path.
 *     5'. e = P_l z_(l+1) through the same path;  z_i = T(z_i + coarse_scale * e_i).
 *   An apply enqueues (2 * sweeps + 2) * (levels - 1) products, and 2 * sweeps - 1 more when the coarsest level is smoothed (products_per_apply);
 *   spmv_count of cvr_pcg_device follows with that P.  cvr_precond_apply_device and cvr_pcg_device / cvr_pcg take the object as they take a plain
 *   one: the apply only enqueues, reads nothing back, forms no dot product, has no kernel that waits on another workgroup and no floating-point
 *   atomic, gives the same bits on every call for every alignment of r_dev and z_dev, and its last launch writes z and the partial sums of r.z.
 * cvr_precond_amg_smoothed_info / cvr_amg_hierarchy_smoothed_info fill a cvr_amg_smoothed_info; of a plain kind-4 object or hierarchy: all zero.
 * cvr_precond_amg_export_prolongator / cvr_amg_hierarchy_export_prolongator write P_l of level 0 .. levels - 2 to host arrays: row_ptr (n_l + 1),
 *   col_idx and vals (p_nnz[level]); a caller reads the sizes from the two infos first.  The coarsest level, a level outside the hierarchy, a plain
 *   object or hierarchy, another kind, or a null array: CVR_ERR_INVALID.
 * Errors of cvr_precond_amg_smoothed: those of cvr_precond_amg in their order, with the check of omega (CVR_ERR_INVALID, "omega" in
 *   cvr_last_error) right behind the options; of cvr_amg_smoothed_setup_host: those of cvr_amg_setup_host, omega likewise. */
typedef struct {
    int32_t smoothed;                          /* 1: built by a *_smoothed entry point; 0: plain, and everything below is 0 */
    int32_t products_per_apply;
    double  omega;                             /* as used: 4/3 for an argument of 0.0                                       */
    int64_t p_nnz[CVR_AMG_MAX_LEVELS];         /* entries of P_l; 0 from the coarsest level on                              */
    int32_t reserved[8];                       /* 0                                                                         */
} cvr_amg_smoothed_info;                       /* 176 bytes */
int cvr_precond_amg_smoothed(cvr_precond **out, cvr_handle *h, const cvr_csr_view *csr, const cvr_amg_options *opt, double omega, void *stream);
int cvr_amg_smoothed_setup_host(cvr_amg_hierarchy **out, const cvr_csr_view *csr, const cvr_amg_options *opt, double omega, int32_t *bad_level, int64_t *bad_row);
int cvr_precond_amg_smoothed_info(const cvr_precond *p, cvr_amg_smoothed_info *info);
int cvr_amg_hierarchy_smoothed_info(const cvr_amg_hierarchy *hier, cvr_amg_smoothed_info *info);
int cvr_precond_amg_export_prolongator(const cvr_precond *p, int32_t level, int64_t *row_ptr, int32_t *col_idx, void *vals);
int cvr_amg_hierarchy_export_prolongator(const cvr_amg_hierarchy *hier, int32_t level, int64_t *row_ptr, int32_t *col_idx, void *vals);

/* Smoothed-aggregation AMG whose set-up runs on the device: cvr_precond_amg_smoothed with a distance-2 maximal independent set, MIS(2), in place of
 * the three serial passes -- an aggregation defined by parallel rounds (Bell, Dalton, Olson), since a pass that walks the rows in ascending order
 * cannot be a kernel.  The object is kind 4 with smoothed = 1: its cycle, products_per_apply, buffers, exports, infos and the entry points that
 * take or decline it are the smoothed kind's, unchanged.  Everything of the set-up but the aggregation keeps the text above bit for bit: the
 * smoother diagonal, the bad-diagonal rule (the lowest row), the stopping rule, the stall rule, steps 1 - 5, the dense inverse, omega.
 * The aggregation of a level (a CSR that passed the structure rules) with `strength`:
 *   N(i), the strong neighbours: the columns j != i of row i whose entry passes the strength test above (a_ij != 0 and
 *     a_ij * a_ij >= ((strength * strength) * a_ii) * a_jj in fp64).  N is taken row by row and never symmetrised: everything below is defined for
 *     a directed N (a coarse operator is symmetric only to rounding, and the structure rules do not ask for a symmetric pattern).
 *   Keys: h(i) = murmur3's 32-bit finaliser of uint32(i) (x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16, modulo 2^32);
 *     key(i) = (uint64(state_i) << 62) | (uint64(h(i) >> 1) << 31) | uint64(i) with the states 1 undecided, 2 root, 0 out.  n < 2^31 - 1, so keys
 *     are unique.  The hash is of the row index alone: no level, no seed -- the aggregation of a matrix is a function of that matrix.
 *   Rounds: all rows start undecided.  A round is a pure function of the states at its start: m1(i) = max(key(i), key(j) for j in N(i));
 *     m2(i) = max(m1(i), m1(j) for j in N(i)); an undecided i with m2(i) == key(i) becomes a root, an undecided i whose m2(i) carries state 2 goes
 *     out.  Rounds repeat until no row is undecided; `rounds` counts those that began with an undecided row (0 for n = 0).  The undecided row with
 *     the largest key sees a root or itself, so every round decides a row; a row with empty N(i) is a root after round 1 and ends as a singleton.
 *   Numbering: the aggregates are numbered by their roots in ascending row order (an exclusive scan of the root flags); nc = the roots.
 *   Join, two passes, each a pure function of the state before it: 1. a non-root i with a root in N(i) takes the aggregate of the root j with the
 *     largest |a_ij| (fp64; ties: the lowest j); 2. a still-free i takes the aggregate of the j in N(i) that is a root or was assigned by pass 1,
 *     by the same rule (rows assigned by pass 2 do not count).  An out row has a root within two directed steps, so no row stays free.  Nothing is
 *     merged, split or renumbered afterwards.
 * cvr_precond_amg_mis2 runs none of the level loop on the host.  Level 0 is copied once into arrays of the object's own on the device (from host
 *   arrays, checked on the host before any device work, or from device arrays, checked where they lie: the structure rules by a kernel that finds
 *   the lowest offending row).  Per level: a kernel for the diagonal, dinv and the lowest bad row (an integer atomicMin), one for the flags of the
 *   strong entries, two per round (m1; m2 with the state update and the count of undecided rows, an integer atomic add), a scan of the root flags,
 *   the two join passes, then steps 1 - 5 as cvr_precond_amg_smoothed does them.  A thread per row; no kernel waits on another workgroup; no
 *   floating-point atomic.  The host waits on scalars only (the bad-row word, the undecided counts, nc, the products' nnz) and reads the coarsest
 *   level (at most CVR_AMG_MAX_COARSE rows) for the dense inverse.  CVR_DEBUG=mis2_check=<k> reads the undecided counts back every k rounds
 *   (default 4); the surplus rounds change nothing and are not counted, so no bit and no count depends on k.
 *   The object keeps every level's CSR, dinv, agg and P_l in device arrays of its own beside the handles; the exports and infos copy from them when
 *   asked (and keep the host copy).  Levels, prolongators, infos and `rounds` are cvr_amg_mis2_setup_host's byte for byte.
 * cvr_amg_mis2_setup_host: cvr_amg_smoothed_setup_host with this aggregation in host loops.
 * cvr_precond_amg_mis2_info / cvr_amg_hierarchy_mis2_info fill a cvr_amg_mis2_info; of a kind-4 object or hierarchy built another way: all zero;
 *   another kind: CVR_ERR_INVALID.  cvr_precond_amg_smoothed_info reports smoothed = 1 on the new object.
 * cvr_amg_mis2_aggregate_host / _device: the aggregation alone, of any square matrix that passes the structure rules (nothing is asked of the
 *   diagonal's sign: the strength test reads it as it is): agg (nrows entries; host memory / memory of `device`), *nc and *rounds.  The device call
 *   checks the view as cvr_precond_amg_mis2 checks device arrays, orders itself behind `stream` and returns with it idle; both give the same agg.
 * Errors: those of cvr_precond_amg_smoothed / cvr_amg_smoothed_setup_host in their order, with the entry point's own name in cvr_last_error; on a
 *   failure nothing is left allocated. */
typedef struct {
    int32_t mis2;                              /* 1: built by a *_mis2 entry point; 0: otherwise, and everything below is 0 */
    int32_t reserved0;                         /* 0                                                                         */
    int32_t rounds[CVR_AMG_MAX_LEVELS];        /* MIS rounds of level l's aggregation; 0 from the coarsest level on         */
    int32_t reserved[8];                       /* 0                                                                         */
} cvr_amg_mis2_info;                           /* 104 bytes */
int cvr_precond_amg_mis2(cvr_precond **out, cvr_handle *h, const cvr_csr_view *csr, const cvr_amg_options *opt, double omega, void *stream);
int cvr_amg_mis2_setup_host(cvr_amg_hierarchy **out, const cvr_csr_view *csr, const cvr_amg_options *opt, double omega, int32_t *bad_level, int64_t *bad_row);
int cvr_precond_amg_mis2_info(const cvr_precond *p, cvr_amg_mis2_info *info);
int cvr_amg_hierarchy_mis2_info(const cvr_amg_hierarchy *hier, cvr_amg_mis2_info *info);
int cvr_amg_mis2_aggregate_host(const cvr_csr_view *csr, double strength, int32_t *agg, int64_t *nc, int32_t *rounds);
int cvr_amg_mis2_aggregate_device(const cvr_csr_view *csr_on_device, double strength, int32_t *agg_dev, int64_t *nc, int32_t *rounds, int device, void *stream);

/* The object with several right-hand sides (a block-Jacobi object; a cvr_precond_amg_block object: its section below): Z = W R for 1 <= nvec <= 8 columns at once.  R_dev and Z_dev: row-major blocks of exactly n rows of
 * ldr / ldz values of the object's type (row i holds the values of all columns at i) in the memory of the object's device; values at positions
 * >= nvec of a row are neither read nor written; any alignment of the element type; the blocks must not overlap.
 * Column c of Z is bit for bit what cvr_precond_apply_device gives for column c of R: the same left-to-right sum from t_0, every product and every
 * addition rounded on its own (no fused multiply-add); no R and no Z beyond row n - 1 for a short last block.  Each W[i][j] is loaded once for all
 * columns of its row, and a row of R in 16-byte pieces where nvec, the leading dimension and the base allow it.  The kernel runs on the solvers'
 * grid (1024 workgroups of 256 threads); the thread that owns a 16-byte packet of rows of a single vector owns those rows of every column.
 * The call only enqueues on `stream` and makes the object's device current; n == 0 is CVR_OK.
 * Errors, CVR_ERR_INVALID before any device work: a null argument; R_dev == Z_dev; nvec outside 1..8; ldr < nvec or ldz < nvec. */
int cvr_precond_apply_multi_device(const cvr_precond *p, const void *R_dev, int64_t ldr, void *Z_dev, int64_t ldz, int32_t nvec, void *stream);

/* Batched conjugate gradients preconditioned by such an object.  Everything cvr_cg_multi_device's text above fixes holds word for word -- the
 * blocks B_dev and X_dev, the leading dimensions, the padding columns that are never touched, res[nvec]; independent columns, each with its own
 * state cell and its own stop, and no write to a stopped column's slices; spmv_count and seconds the same in every res[j]; nvec = 1 with
 * ldb = ldx = 1 on every single-GPU handle through cvr_spmv_device's launch path; the ordering, a mutable handle's image, "not capturable in a HIP
 * graph" -- with Z = W R by the apply arithmetic above in place of z = T(minv * r); Z is a block of the library, allocated per call.  In the sum
 * r.z of a column the thread that owns element i adds the term double(r_i) * double(z_i), in element order.  Four vector launches beside the
 * k-wide product per step (Z is formed by a launch of its own between the update and the direction: an element of z needs its whole block of r).
 * The contract, for every column j: column j of X and res[j].iterations, .status, .residual_norm and .b_norm are bit for bit what cvr_pcg_device
 * returns on the same handle and object for b = B[:, j], x0 = X[:, j] and the same options -- for every check_every, ldb, ldx and alignment.  It
 * follows that with block_size = 1 column j is bit for bit cvr_cg_multi_device's with minv_dev = the exported W.
 * Errors, in this order.  Before any device work and before the handle is looked at: cvr_cg_device's argument checks; p null; opt->minv_dev != NULL
 * (one preconditioner per call); nvec outside 1..8, ldb < nvec or ldx < nvec: CVR_ERR_INVALID.  Then: before cvr_preprocess: CVR_ERR_STATE;
 * nrows != ncols: CVR_ERR_INVALID; a handle that does not take the block (cvr_cg_multi_device): CVR_ERR_STATE; (ncols + 1) * nvec values beyond
 * 4 GiB: CVR_ERR_INVALID; then the three mismatches of cvr_pcg_device (n, type, device), each CVR_ERR_INVALID naming the mismatch. */
int cvr_pcg_multi_device(cvr_handle *h, const cvr_precond *p, const void *B_dev, int64_t ldb, void *X_dev, int64_t ldx, int32_t nvec,
                         const cvr_cg_options *opt, cvr_cg_result *res, void *stream);
/* the same with host B and X (nrows x nvec each, row-major, ld = nvec; X in and out), as cvr_cg_multi */
int cvr_pcg_multi(cvr_handle *h, const cvr_precond *p, const void *B_host, void *X_host, int32_t nvec, const cvr_cg_options *opt, cvr_cg_result *res);

/* ---- the fifth kind for blocks of right-hand sides: one V-cycle for up to 8 vectors, and batched PCG on it ----
 * A fourth way to build a kind-4 object.  An AMG apply is bound by its launches (the many small coarse-level products), not by bytes; a cycle that
 * carries K vectors through every level issues the launches of a cycle for one and reads every level's image, dinv, agg and winv once for all K
 * columns.  The three constructors above, their objects and the entry points that decline them are unchanged: block support is this constructor's.
 * Object.  cvr_precond_amg_block(out, h, csr, opt, setup, omega, nvec, stream) returns a kind-4 object whose hierarchy is byte for byte what the
 *   constructor named by `setup` builds from the same h, csr, opt, omega and stream -- cvr_precond_amg (CVR_AMG_SETUP_PLAIN; omega is ignored),
 *   cvr_precond_amg_smoothed (CVR_AMG_SETUP_SMOOTHED) or cvr_precond_amg_mis2 (CVR_AMG_SETUP_MIS2): it is that constructor's set-up, not a copy of it.
 *   cvr_precond_amg_info, cvr_precond_amg_export_level, cvr_precond_amg_smoothed_info, cvr_precond_amg_export_prolongator and
 *   cvr_precond_amg_mis2_info work on it unchanged, and everything said above of the borrowed handle, the CSR input, n = 0, one stream at a time,
 *   cvr_precond_get_info and cvr_precond_destroy holds.
 * Width.  nvec = K, 1 .. 8, is the width the object is built for.  Every handle the object owns (the coarse operators, and P_l and R_l of the
 *   smoothed set-ups; R_l from the transposed arrays as above) is created with cvr_options.nvec = K: the plain layout for K >= 2, the default options
 *   for K = 1.  Every per-level buffer (r, z, q, t, e) is a row-major block of K columns with the fixed leading dimension K, sized from the handle's
 *   x_elems / yext_elems rows and zeroed once; the pad row of an SpMV input (row n_l of z and t) lies at one place for every block call and is never
 *   written.  cvr_amg_block_info.buffer_bytes is the sum of these blocks.
 * Level 0.  h is borrowed.  For K >= 2 it must satisfy cvr_spmm_supported(h), else CVR_ERR_STATE (create it with cvr_options.nvec >= 2), and
 *   (ncols + 1) * K values beyond 4 GiB is CVR_ERR_INVALID; both right behind the constructor's other checks of h.
 * Single-vector calls.  cvr_precond_apply_device and cvr_pcg_device / cvr_pcg take the object as they take any kind-4 object: they run the cycle
 *   above (steps 1 - 6; 3' and 5' for the smoothed set-ups) with each product through the level's handle at nvec = 1, ld = 1 (cvr_spmv_device's
 *   launch path), on the same buffers read as vectors.  At ld = 1 the pad of an SpMV input is element n_l, which a block call writes: the cycle
 *   begins with one small launch that zeroes those elements.  The bits are those of the cycle with a caller's handle of each exported level created
 *   with cvr_options.nvec = K in place of the object's.  They are not necessarily those of an ordinary object of the same set-up, whose handles have
 *   the default layout (another summation order inside a product).
 * cvr_precond_apply_multi_device(p, R, ldr, Z, ldz, nvec, stream) takes the object for 1 <= nvec <= K: copy-in (R of ldr -> r_0 of K), the cycle
 *   with k-wide kernels and each product through cvr_spmm_device's path (launch on the plain image at ld = K, inside the update ordering of a
 *   mutable level-0 handle; K = 1: cvr_spmv_device's path), copy-out (z_0 -> Z of ldz).  Column c of Z is bit for bit cvr_precond_apply_device of
 *   the same object on column c of R, for every nvec, ldr, ldz and alignment of the element type: per column the kernels perform the single-vector
 *   kernels' operations in their order (fp64, each rounded on its own, one rounding to T per stored value, no fused multiply-add), and a column of
 *   the k-wide product has cvr_spmv_device's bits.  Values at positions >= nvec of a row of R are not read, of a row of Z not written.  Columns
 *   nvec .. K - 1 of the object's buffers keep what an earlier call left; nothing reads them.  The call only enqueues, reads nothing back, and no
 *   kernel waits on another workgroup.  A thread owns a row of a level (an aggregate in the restriction; a row of the dense inverse, each W value
 *   loaded once for all columns) and moves its K values in 16-byte packets where K and the type allow it.  nvec > K: CVR_ERR_INVALID naming both
 *   numbers, behind the call's other checks in their order.
 * cvr_pcg_multi_device / cvr_pcg_multi take the object under cvr_pcg_multi_device's contract above, word for word: for every column j, column j of
 *   X and res[j].iterations, .status, .residual_norm and .b_norm are bit for bit cvr_pcg_device's on the same handle and object for b = B[:, j],
 *   x0 = X[:, j] -- for every check_every, ldb, ldx and alignment.  The cycle touches only the object's buffers and computes all nvec columns
 *   whatever their cells say; the apply's last launch writes Z, per column the partial sums of r.z into set 1 and, at the start, P = Z, for live
 *   columns only: a column whose cell holds a stop is not written.  spmv_count = 1 + P + (1 + P) * (steps enqueued), P the products of an apply (a
 *   k-wide product counts once).  nvec > K: CVR_ERR_INVALID, behind the call's other checks.  nvec = 1 with ldb = ldx = 1 runs on every single-GPU
 *   handle, as before (the object's own level-0 handle is the one it was built with).
 * cvr_precond_export, cvr_pbicgstab_device / cvr_pbicgstab and cvr_pgmres_device / cvr_pgmres decline the object as they decline kind 4.
 * Errors of cvr_precond_amg_block, in this order, before any device work: a null out, h or csr; setup outside 0 .. 2; nvec outside 1 .. 8:
 *   CVR_ERR_INVALID; then everything the constructor named by `setup` checks, in its order and with its codes, the texts that name an entry point
 *   beginning with cvr_precond_amg_block.
 * cvr_precond_amg_block_info fills a cvr_amg_block_info.  An object of another kind: CVR_ERR_INVALID ("... is of kind k, not an AMG object"); a
 *   kind-4 object of another constructor: CVR_ERR_INVALID, "was not built by cvr_precond_amg_block"; a null argument: CVR_ERR_INVALID. */
#define CVR_AMG_SETUP_PLAIN    0               /* cvr_precond_amg's set-up                                                  */
#define CVR_AMG_SETUP_SMOOTHED 1               /* cvr_precond_amg_smoothed's                                                */
#define CVR_AMG_SETUP_MIS2     2               /* cvr_precond_amg_mis2's                                                    */
typedef struct {
    int32_t nvec, setup;                       /* K and CVR_AMG_SETUP_* as given                                            */
    int64_t buffer_bytes;                      /* device bytes of the per-level blocks r, z, q, t, e                        */
    int32_t reserved[8];                       /* 0                                                                         */
} cvr_amg_block_info;                          /* 48 bytes */
int cvr_precond_amg_block(cvr_precond **out, cvr_handle *h, const cvr_csr_view *csr, const cvr_amg_options *opt, int32_t setup, double omega, int32_t nvec, void *stream);
int cvr_precond_amg_block_info(const cvr_precond *p, cvr_amg_block_info *info);

/* BiCGSTAB preconditioned by such an object.  Everything cvr_bicgstab_device's text above fixes holds word for word -- the handles, b_dev and x_dev,
 * the options and the result, r = b - A x by the scaled product, every update, the fixed-tree sums, alpha, omega and beta, the stop rules and status
 * codes, b == 0, a start within the tolerance, the non-finite cases, the half-step stop, check_every, spmv_count, seconds, the ordering on `stream` --
 * with M^-1 = W of the object in place of diag(minv): p^ = W p wherever that text says p^ = T(minv * p), s^ = W s wherever it says
 * s^ = T(double(minv) * double(s)), both by the apply arithmetic above.  p^ and s^ are buffers of the library, allocated per call with the others.
 * Each apply is a launch of its own (an element of p^ needs its whole block of p): seven vector launches beside the two SpMVs per step.  A kernel
 * behind a stop or a half-step stop writes nothing, the applies included: x and the result do not depend on check_every.
 * The contract that follows: with block_size = 1, x, iterations, status, residual_norm and b_norm are bit for bit what cvr_bicgstab_device returns
 * with minv_dev = the exported W, on every layout and for every check_every.
 * Errors, in this order.  Before any device work and before the handle is looked at: cvr_cg_device's argument checks; p null; opt->minv_dev != NULL
 * (one preconditioner per call): CVR_ERR_INVALID.  Then: before cvr_preprocess: CVR_ERR_STATE; nrows != ncols: CVR_ERR_INVALID; then, each
 * CVR_ERR_INVALID with cvr_last_error naming the mismatch: p's n differs from the handle's nrows, p's type from the handle's, p's device from the
 * handle's. */
int cvr_pbicgstab_device(cvr_handle *h, const cvr_precond *p, const void *b_dev, void *x_dev, const cvr_cg_options *opt, cvr_cg_result *res, void *stream);
/* the same with host b and x (nrows values each; x in and out), as cvr_cg */
int cvr_pbicgstab(cvr_handle *h, const cvr_precond *p, const void *b_host, void *x_host, const cvr_cg_options *opt, cvr_cg_result *res);

/* Restarted GMRES(m) preconditioned by such an object.  Everything cvr_gmres_device's text above fixes holds word for word -- `restart`, the handles,
 * b_dev and x_dev, the options and the result, the start of the call and of every cycle, the two Gram-Schmidt passes, the rotations, the scalars, the
 * fixed-tree sums, the stop rules and status codes, b == 0, a start within the tolerance, the non-finite cases, the lucky breakdown, check_every,
 * spmv_count, seconds, the ordering on `stream` -- with M^-1 = W of the object in place of diag(minv): z_j = W v_j by the apply arithmetic above
 * wherever that text says z = T(double(minv) * double(v_j)).  The apply is a launch of its own: six vector launches beside the SpMV per step.
 *   Forming x from q columns (q = 0: nothing): y as there.  Per element u = +0; for i = 0..q-1: u = u + y_i * double(v_i), kept in fp64 (never
 *     rounded to T) in a buffer of the library of n doubles, allocated with the call's other buffers.  Then, for row i of block k with m columns:
 *     x_i = T(double(x_i) + (t_0 + t_1 + ... + t_(m-1)))   with   t_j = double(W[i][j]) * u[k*bs + j],
 *     the apply's order and rounding with the fp64 u where the apply has double(r).  Two launches where cvr_gmres_device has one.
 * A kernel behind a stop writes nothing that reaches x or the result, the applies and the two x-forming kernels included.
 * The contract that follows: with block_size = 1, x, iterations, status, residual_norm and b_norm are bit for bit what cvr_gmres_device returns with
 * minv_dev = the exported W, on every layout and for every check_every.
 * Errors, in this order.  Before any device work and before the handle is looked at: cvr_cg_device's argument checks; p null; opt->minv_dev != NULL;
 * restart < 1 or restart > CVR_GMRES_MAX_RESTART ("restart" in cvr_last_error): CVR_ERR_INVALID.  Then: before cvr_preprocess: CVR_ERR_STATE;
 * nrows != ncols: CVR_ERR_INVALID; the three mismatches of cvr_pcg_device, each CVR_ERR_INVALID; no device memory for the call's buffers:
 * CVR_ERR_NOMEM, nothing allocated. */
int cvr_pgmres_device(cvr_handle *h, const cvr_precond *p, const void *b_dev, void *x_dev, int32_t restart, const cvr_cg_options *opt, cvr_cg_result *res,
                      void *stream);
/* the same with host b and x (nrows values each; x in and out), as cvr_cg */
int cvr_pgmres(cvr_handle *h, const cvr_precond *p, const void *b_host, void *x_host, int32_t restart, const cvr_cg_options *opt, cvr_cg_result *res);

/* ---- flexible GMRES(m): every kind of cvr_precond, or a caller's apply ----
 * cvr_pgmres forms x as x += M^-1 (V y): a second apply per cycle on an fp64 combination, which only block-Jacobi and ILU(0) have a form for, and
 * which is right only when M^-1 is the same linear operator at every step.  Flexible GMRES (Saad, SIAM J. Sci. Comput. 14, 1993) keeps
 * z_j = M_j^-1 v_j for every column of the cycle and forms x = x0 + Z y: no apply outside the steps, and M_j may differ from step to step.  The
 * price is `restart` more vectors.  The options, the result, the status codes, the range of `restart` (1 .. CVR_GMRES_MAX_RESTART), check_every and
 * the ordering on `stream` are cvr_gmres_device's; the start of the call and of every cycle, the two Gram-Schmidt passes, the rotations, the
 * scalars, the fixed-tree sums and the stop rules are its text word for word with w = T(A z_j).
 *
 * Which preconditioner is used: exactly one of three cases.
 *   p != NULL    any kind that cvr_precond_apply_device accepts (an object of cvr_precond_amg_block included), z_j = M^-1 v_j by that entry point's
 *                arithmetic for the kind.  (The kinds that are symmetric positive definite by construction -- Chebyshev, FSAI, plain AMG -- are taken
 *                as well: whether they help on a nonsymmetric A is the caller's judgement.)
 *   fn != NULL   z_j = whatever fn leaves in z_dev, see below.
 *   neither      z_j = v_j, Z is the basis itself (nothing is copied): x, iterations, status, residual_norm and b_norm are bit for bit what
 *                cvr_gmres_device returns without minv_dev.
 * Both set: CVR_ERR_INVALID.  opt->minv_dev != NULL: CVR_ERR_INVALID in all three cases (the diagonal is cvr_gmres_device's).
 *
 * Storage: restart + 1 basis vectors and, with a preconditioner, `restart` columns of Z, each an SpMV input of the handle (ncols + 1 values), in the
 *   call's one allocation; CVR_ERR_NOMEM names both counts and the bytes.  No fp64 combination is kept.
 * Forming x from q columns (q = 0: nothing): y as in cvr_gmres_device.  Per element u = +0; for i = 0..q-1: u = u + y_i * double(Z_i);
 *   x_i = T(double(x_i) + u).  One launch.
 * Stops inside a batch: a block-Jacobi or ILU(0) apply behind a stop writes nothing.  The other kinds' applies and the callback are not gated: for
 *   the steps the host has enqueued behind a stop they still run (the callback is still called), on vectors that hold no meaning, and write columns
 *   of Z that nothing reads -- the steps are ordered so that a column x is still owed is never written before x is formed.  The contract that
 *   follows: x and the result do not depend on check_every.
 * spmv_count: the handle's own products enqueued, 1 + the steps + the restarts, as cvr_gmres_device counts.  The products that an object's apply
 *   makes (Chebyshev, FSAI, AMG) are not counted, and a callback's are unknown.
 *
 * The callback: int fn(ctx, v_dev, z_dev, n, stream), called on the host, in the calling thread, while step k is being enqueued (once per step, in the
 *   order of the steps, so its k-th call, counted from 0, belongs to step k).  v_dev and z_dev are 16-byte-aligned buffers of the library of n
 *   values of the handle's type on the handle's device; they do not overlap.  It must leave z = M_k^-1 v complete in stream order on `stream`
 *   (cast to hipStream_t): it may enqueue there, or synchronise and do anything else.  It must not call into this library with the same handle.  A
 *   non-zero return ends the solve with CVR_ERR_STATE, cvr_last_error naming the callback's code and the step; nothing further is enqueued, the
 *   call's buffers are released behind what is enqueued, and x_dev holds no meaning.
 *
 * Errors, in this order.  Before any device work and before the handle is looked at: cvr_cg_device's argument checks (p may be null); p and fn
 * both set; opt->minv_dev != NULL; restart < 1 or restart > CVR_GMRES_MAX_RESTART: CVR_ERR_INVALID.  Then: before cvr_preprocess: CVR_ERR_STATE;
 * nrows != ncols: CVR_ERR_INVALID; with p, the three mismatches of cvr_pcg_device, each CVR_ERR_INVALID with "cvr_fgmres" in cvr_last_error; no
 * device memory for the call's buffers: CVR_ERR_NOMEM, nothing allocated. */
typedef int (*cvr_apply_fn)(void *ctx, const void *v_dev, void *z_dev, int64_t n, void *stream);
int cvr_fgmres_device(cvr_handle *h, const cvr_precond *p, cvr_apply_fn fn, void *ctx, const void *b_dev, void *x_dev, int32_t restart,
                      const cvr_cg_options *opt, cvr_cg_result *res, void *stream);
/* the same with host b and x (nrows values each; x in and out), as cvr_cg */
int cvr_fgmres(cvr_handle *h, const cvr_precond *p, cvr_apply_fn fn, void *ctx, const void *b_host, void *x_host, int32_t restart,
               const cvr_cg_options *opt, cvr_cg_result *res);

/* ---- a colouring of A's graph, and a sixth kind of cvr_precond on it: multicolour symmetric Gauss-Seidel ----
 * ILU(0)'s sweeps have as many stages as the longest dependency chain of the ordering, thousands on a Laplacian in its natural order.  Colour the
 * graph so that no two coupled rows share a colour, order the rows by colour, and a triangular sweep has as many stages as there are colours,
 * about five.  The colouring is an entry point of its own (it is also what a caller needs to reorder a matrix for cvr_precond_ilu0); the
 * preconditioner built on it is symmetric Gauss-Seidel in that order: no factorisation, no pivot breakdown beyond a zero diagonal, usable on
 * any sparse matrix with a diagonal, and symmetric positive definite (so CG may use it) when A is symmetric with a positive diagonal.  Kinds
 * 0 .. 4 are unchanged; this is kind 5.  Like an ILU(0) object it is independent of any handle and is not refreshed by cvr_update_values.
 *
 * The colouring: cvr_color_host (pure host code, no device needed: host arrays only) and cvr_color_device (arrays_on_device 0 or 1).
 * CSR input: a square view checked as cvr_precond_ilu0 checks one -- CVR_ERR_INVALID with cvr_last_error naming the first offending row where the
 *   columns of a row are not strictly increasing or a row has no diagonal entry.  In addition the off-diagonal pattern must be structurally
 *   symmetric: every stored (i, j), j != i, has a stored (j, i); stored zeros count as entries.  A violation is CVR_ERR_INVALID, and cvr_last_error
 *   names the lowest offending row and its lowest such column.  The values are not read: csr->vals may be NULL.  n = 0 is valid; n < 2^31.
 * Definition.  key(i) = (h(i) >> 1) << 31 | i, a 62-bit number: h is murmur3's 32-bit finaliser of uint32(i) (x ^= x >> 16; x *= 0x85ebca6b;
 *   x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16), the function the MIS(2) keys use, without a seed and without a level: a pattern has exactly one
 *   colouring.  All rows begin uncoloured.  One round is a pure function of the state before it: every uncoloured row whose key is greater than
 *   the key of each of its uncoloured neighbours (the columns j != i of its row) takes the smallest colour >= 0 that none of its neighbours
 *   holds.  Rounds repeat until no row is uncoloured.  The result equals greedy first-fit colouring of the rows in descending key order.
 *   A row's colour is at most its number of neighbours; there is no cap on the number of colours.
 * Outputs: color[n] (int32, 0 .. ncolors - 1, every colour used); *ncolors; *rounds, the number of rounds that coloured at least one row (0 for
 *   n = 0); perm[n], the rows ordered by (colour, row number); color_ptr[ncolors + 1], where each colour begins in perm (color_ptr[0] = 0,
 *   color_ptr[ncolors] = n; the array needs room for n + 1 values, since ncolors is not known before the call).
 * On the device a round is one launch with a thread per row that reads one array of int32 words (-1 or the colour) and writes another; the count
 *   of rows still uncoloured comes back every k rounds, k = 4 unless CVR_DEBUG=color_check=<k> is set; a round with nothing uncoloured changes
 *   nothing, so neither a bit nor *rounds depends on k.  perm and color_ptr come from a counting sort with a stable placement.  No kernel waits on
 *   another workgroup; the only atomics are integer (min, max, add) and order-free.  cvr_color_device synchronises `stream`.
 * Errors: a null argument (color and perm may be NULL for n = 0), nrows != ncols, nrows >= 2^31: CVR_ERR_INVALID before any array is read;
 *   cvr_color_host with arrays_on_device set: CVR_ERR_INVALID; `device` out of range: CVR_ERR_NO_DEVICE; cvr_create's checks of a view and the
 *   rules above: CVR_ERR_INVALID; CVR_ERR_NOMEM.  On an error *ncolors and *rounds are 0.
 *
 * The preconditioner, cvr_precond_mcsgs: M = (D + L) D^-1 (D + U), z = M^-1 r.  D is A's diagonal, L holds the entries a_ij with
 *   color[j] < color[i], U those with color[j] > color[i]; a valid colouring has no off-diagonal entry within one colour, so L + D + U = A.
 * Set-up, on the device, from host or device arrays (read and checked as above; the values are read): the colouring; then two CSR parts with the
 *   rows in perm order, the entries of a part in A's column order with their original column numbers and values of T; the diagonal as doubles.
 *   A diagonal entry that is zero or not finite: CVR_ERR_STATE, cvr_last_error names the lowest such row, nothing is left allocated.  The host
 *   waits on the scalars of the colouring, the ncolors + 1 colour offsets and the bad-row word, never on an array of n.
 * Apply, G = lanes_per_row lanes per row by ILU(0)'s rule: G is the power of two from ceil((nnz - n) / (2 n)) up, at least 1 and at most 64, fixed
 *   per object (CVR_DEBUG=mcsgs_lanes=<G>, a power of two 1 .. 64, overrides it when the object is built).  Lane l of a row takes the entries
 *   l, l + G, .. of the row's part and forms s_l = +0 + t + t' + .. with t = double(a_ij) * double(v_j), left to right in fp64, every product and
 *   addition rounded on its own; the lanes are combined by the xor butterfly (s += s of lane ^ o for o = G/2 .. 1).  Then
 *       forward, colours 0 .. ncolors - 1, one launch per colour over its rows:    y_i = T((double(r_i) - s) / double(a_ii)),   over L with v = y;
 *       backward, colours ncolors - 1 .. 0, one launch per colour:                 z_i = T(double(y_i) - s / double(a_ii)),   over U with v = z.
 *   y is a buffer of the object, so one object serves one stream at a time.  cvr_precond_apply_device takes this kind: exactly 2 ncolors launches
 *   on `stream` and nothing else, without a read-back; the same bits every call and for every alignment of r_dev and z_dev.
 * cvr_pcg_device / cvr_pcg take this kind: cvr_pcg_device's text holds with this apply in place of z = W r; one kernel behind the sweeps forms the
 *   partial sums of r.z and, at the start, p = z, exactly as for an ILU(0) object; behind a stop x, r and p stay untouched (z is scratch).
 *   3 + 2 ncolors + 1 launches per step; spmv_count as with block-Jacobi.
 * cvr_precond_get_info works for this kind (block_size, nblocks and identity_blocks are 0); cvr_precond_destroy frees everything.
 * cvr_precond_export, cvr_precond_apply_multi_device, cvr_pcg_multi_device / cvr_pcg_multi, cvr_pbicgstab_device / cvr_pbicgstab and
 * cvr_pgmres_device / cvr_pgmres decline this kind: CVR_ERR_STATE behind their other checks, cvr_last_error naming kind 5, "multicolour SGS".  The
 * other kinds' info and export calls on this kind, and cvr_precond_mcsgs_info / cvr_precond_mcsgs_export on another kind or with a null argument:
 * CVR_ERR_INVALID.  cvr_precond_mcsgs_export writes color[n], perm[n] and color_ptr[ncolors + 1] to the host.
 * Errors of cvr_precond_mcsgs: a null argument, nrows != ncols, nrows >= 2^31: CVR_ERR_INVALID before any device work; `device` out of range:
 * CVR_ERR_NO_DEVICE; the view's checks above: CVR_ERR_INVALID; CVR_ERR_NOMEM: an allocation failed (nothing is left allocated). */
typedef struct {
    int64_t n, nnz;                            /* nnz = the entries of the n rows                                           */
    int32_t ncolors, rounds;                   /* of the colouring                                                          */
    int32_t launches_per_apply;                /* 2 * ncolors                                                               */
    int32_t lanes_per_row;                     /* G                                                                         */
    int32_t max_color_rows, min_color_rows;    /* rows of the largest and of the smallest colour                            */
    int32_t is_f32;
    int32_t reserved[8];                       /* 0                                                                         */
} cvr_mcsgs_info;
int cvr_color_host(const cvr_csr_view *csr, int32_t *color, int32_t *perm, int32_t *color_ptr, int32_t *ncolors, int32_t *rounds);
int cvr_color_device(const cvr_csr_view *csr, int32_t device, void *stream, int32_t *color, int32_t *perm, int32_t *color_ptr, int32_t *ncolors, int32_t *rounds);
int cvr_precond_mcsgs(cvr_precond **out, const cvr_csr_view *csr, int32_t device, void *stream);
int cvr_precond_mcsgs_info(const cvr_precond *p, cvr_mcsgs_info *info);
int cvr_precond_mcsgs_export(const cvr_precond *p, int32_t *color_host, int32_t *perm_host, int32_t *color_ptr_host);

/* ---- least squares on the device: LSQR ------------------------------------------------------------------
 * min ||b - A x||_2 over x for A of any shape and rank -- over- and under-determined and rank-deficient systems included --, and with damp > 0
 * min ||b - A x||^2 + damp^2 ||x - x0||^2 (Tikhonov): LSQR of Paige and Saunders (ACM TOMS 8, 1982), the Golub-Kahan bidiagonalisation with one
 * product by A and one by A^T per step.  From x0 = 0 it converges to the solution of least 2-norm. */
typedef struct {
    double  arnorm;     /* estimate of ||A^T r - damp^2 (x - x0)||_2 at the stop                 */
    double  anorm;      /* running Frobenius estimate of [A; damp I]                             */
    int32_t stop_test;  /* 0: none (max_iters / breakdown); 1: residual test; 2: normal-equations test */
    int32_t reserved;
} cvr_lsqr_info;
/* a: the single-GPU handle of A, m x n (any layout).  at: a handle of A^T, n x m, of the same value type on the same device -- usually cvr_create
 * with cvr_options.transpose = 1 on the CSR that made `a`; a == at for a square symmetric A.  The library checks shapes, type and device; that `at`
 * holds A^T is the caller's promise.  b_dev: m values of the handles' type, x_dev: n values, the start vector x0 on entry and the solution on exit;
 * neither needs a pad element or a scratch tail.  The options, the result and the status codes are cvr_cg_device's; opt->minv_dev must be NULL.
 * info may be NULL.  The buffers of the call are the library's, allocated per call: v (a's info.x_elems values, v[n] == 0), u^ (the larger of a's
 * info.yext_elems and m + 1 values: the output of a's scaled product and the input of at's product, u^[m] == 0), q (a's info.yext_elems), p (at's
 * info.yext_elems) and w (n values).
 * Arithmetic, T = the handles' type, every operation below rounded on its own (no fused multiply-add); every scalar is fp64; u is kept unnormalised,
 * u^ = beta u (A^T u^ = beta A^T u, so no pass divides u^ by its norm); v is kept normalised:
 *   start: u^ = b - A x0 by one cvr_spmv_scaled_device on `a` with alpha = -1, beta = 1 (in T);  bnorm = sqrt(b.b);  beta = sqrt(u^.u^);
 *     p = A^T u^ through cvr_spmv_device's launch path on `at`;  v^ = T(double(p) / beta);  alpha = sqrt(v^.v^);  v = T(double(v^) / alpha);  w = v;
 *     rhobar = alpha;  phibar = beta;  anorm2 = 0;  psi2 = 0;  rnorm = beta;  arnorm = alpha * beta;  anorm = 0.
 *   per step: q = A v through cvr_spmv_device's launch path on `a` (bit for bit its y for the same v);
 *     u^ = T(double(q) - (alpha / beta) * double(u^));  beta' = sqrt(u^.u^);
 *     p = A^T u^ (the same path on `at`);  if beta' != 0: v^ = T(double(p) / beta' - beta' * double(v));  alpha' = sqrt(v^.v^), or 0 when beta' == 0;
 *     anorm2 = anorm2 + ((alpha * alpha + beta' * beta') + damp * damp);
 *     if damp > 0: rhobar1 = sqrt(rhobar * rhobar + damp * damp);  psi = (damp / rhobar1) * phibar;  phibar = (rhobar / rhobar1) * phibar;
 *       else rhobar1 = rhobar;  psi = 0;
 *     rho = sqrt(rhobar1 * rhobar1 + beta' * beta');  c = rhobar1 / rho;  s = beta' / rho;  theta = s * alpha';  rhobar = -c * alpha';
 *     phi = c * phibar;  phibar = s * phibar;
 *     x = T(double(x) + (phi / rho) * double(w));
 *     psi2 = psi2 + psi * psi;  rnorm = sqrt(phibar * phibar + psi2);  arnorm = alpha' * |s * phi|;  anorm = sqrt(anorm2);
 *     the stop tests;  then v = T(double(v^) / alpha');  w = T(double(v) - (theta / rho) * double(w));  alpha = alpha';  beta = beta'.
 *   The sums b.b, u^.u^ and v^.v^ are accumulated in fp64 from the rounded T values in cvr_cg_device's fixed tree (1024 workgroups of 256 threads,
 *   each thread over its 16-byte packets in order, then lanes, wavefronts and workgroups in a fixed order; no atomics): a call gives the same bits
 *   every time, whatever the alignment of b_dev and x_dev.
 * Stop rule, evaluated on the device after every step, with rnorm, arnorm and anorm all finite (a norm that is not finite never counts as converged):
 *   test 1: rnorm <= rtol * bnorm;  else test 2: arnorm <= (rtol * anorm) * rnorm.  Either is CVR_CG_CONVERGED with info->stop_test = 1 or 2.  The
 *   step that finds the stop has applied its update of x; it writes neither v nor w.
 *   beta', alpha', rho or phi / rho not finite, or rho == 0: CVR_CG_BREAKDOWN, found before x is touched, so x, iterations, residual_norm and info
 *   stay at the last iterate's.  beta' == 0 or alpha' == 0 is no breakdown: the formulas then end in test 1 or test 2.
 *   At the start, in this order: b == 0: x = 0, 0 iterations, converged, residual_norm = 0 (stop_test 0);  beta not finite: CVR_CG_BREAKDOWN;
 *   beta <= rtol * bnorm: converged by test 1;  (each of these three with arnorm = 0, since alpha is not looked at;)  alpha not finite:
 *   CVR_CG_BREAKDOWN;  alpha == 0: converged by test 2.  All with 0 iterations, x untouched (but for b == 0), residual_norm = beta, anorm = 0.  A NaN
 *   or an Inf in b makes beta not finite.
 *   max_iters steps without a stop: CVR_CG_MAX_ITERS with x the last iterate.  max_iters = 0 forms and tests the start only (spmv_count == 2).
 * residual_norm is rnorm, the recurrence's estimate of sqrt(||b - A x||^2 + damp^2 ||x - x0||^2); b_norm is bnorm.
 * check_every: as for cvr_cg_device -- x, iterations, status, residual_norm, b_norm and info are bit for bit the same for every check_every; only
 * spmv_count (2 + 2 per step enqueued) and seconds differ.  Three vector launches beside the two SpMVs per step.
 * Ordering: as cvr_cg_device on both handles; makes their device current.
 * Errors, in this order.  Before any device work and before a handle is looked at: cvr_cg_device's argument checks (on a, b, x, opt, res); at
 * null; opt->minv_dev != NULL ("minv_dev" in cvr_last_error); damp negative or not finite ("damp"): CVR_ERR_INVALID.  Then: either handle before
 * cvr_preprocess: CVR_ERR_STATE; at's nrows != a's ncols or at's ncols != a's nrows: CVR_ERR_INVALID; different value types or devices:
 * CVR_ERR_INVALID. */
int cvr_lsqr_device(cvr_handle *a, cvr_handle *at, const void *b_dev, void *x_dev, double damp, const cvr_cg_options *opt, cvr_cg_result *res,
                    cvr_lsqr_info *info, void *stream);
/* the same with host b (m values) and x (n values; in and out): copied up, cvr_lsqr_device on a's stream, x copied back */
int cvr_lsqr(cvr_handle *a, cvr_handle *at, const void *b_host, void *x_host, double damp, const cvr_cg_options *opt, cvr_cg_result *res,
             cvr_lsqr_info *info);

/* ---- symmetric indefinite systems on the device: MINRES -------------------------------------------------------
 * (A - shift I) x = b for a symmetric A, definite or not, singular consistent systems included: MINRES of Paige and Saunders (SIAM J. Numer. Anal. 12,
 * 1975), the symmetric Lanczos process with one Givens rotation per step -- one SpMV per step, a fixed number of vectors, and a residual norm that
 * does not increase from step to step.  (cvr_cg_device ends in CVR_CG_BREAKDOWN on an indefinite A; GMRES(m) and LSQR solve it without using the
 * symmetry.) */
typedef struct {
    double  anorm;        /* sqrt of the running sum of alfa^2 + oldb^2 + beta'^2: Frobenius estimate of the tridiagonal */
    double  acond;        /* gmax / gmin over the steps' gamma                                                          */
    int32_t reserved[2];
} cvr_minres_info;        /* 24 bytes */
/* h: any single-GPU handle of a square A (any layout; fused-preprocess, image-cache, mutable and transposed handles included, as for cvr_cg_device).
 * That A is symmetric is the caller's promise: the library does not check it.  b_dev and x_dev: nrows values each of the handle's type; x_dev is the
 * start vector on entry and the solution on exit; neither needs a pad element or a scratch tail.  shift: any finite value.  The options, the result
 * and the status codes are cvr_cg_device's.  opt->minv_dev is an optional diagonal preconditioner M^-1 (nrows values) and must be positive: the
 * caller's promise; a violation that makes r2.z negative is reported as a breakdown (below).  A cvr_precond object is deliberately not taken, and
 * there is no cvr_pminres: MINRES needs a symmetric positive definite M, and the block-Jacobi of an indefinite A is not one.  info may be NULL.
 * The buffers of the call are the library's, one allocation per call: v (info.x_elems values, v[n] == 0), q = A v (info.yext_elems), two r, two w
 * (zeroed at the start), z only with minv_dev, the partial sums and the state cell.
 * Arithmetic, T = the handle's type, every operation below rounded on its own (no fused multiply-add); every scalar is fp64:
 *   start: r2 = b - A x0 by one cvr_spmv_scaled_device with alpha = -1, beta = 1 (in T), and with shift != 0 then r2 = T(double(r2) + shift * double(x0)):
 *     the residual of A - shift I;  z = T(double(minv) * double(r2)), or z is r2 itself without minv_dev;  b_norm = sqrt(b . T(double(minv) * double(b))), the norm the residual is measured in (sqrt(b.b) without minv_dev);  beta = sqrt(r2.z);
 *     v = T(double(z) / beta);  w1 = w2 = 0;  oldb = 0, dbar = 0, epsln = 0, phibar = beta, cs = -1, sn = 0, tnorm2 = 0, gmax = 0, gmin = DBL_MAX.
 *   step k: q = A v through cvr_spmv_device's launch path (bit for bit its y for the same v);
 *     y' = T((double(q) - shift * double(v)) - (beta / oldb) * double(r1))  (no shift term when shift == 0, no r1 term at k = 0);  alfa = v.y';
 *     y = T(double(y') - (alfa / beta) * double(r2));  r1 <- r2, r2 <- y;  z = T(double(minv) * double(r2));  beta' = sqrt(r2.z);
 *     tnorm2 = tnorm2 + ((alfa * alfa + oldb * oldb) + beta' * beta');
 *     oldeps = epsln;  delta = cs * dbar + sn * alfa;  gbar = sn * dbar - cs * alfa;  epsln = sn * beta';  dbar = -cs * beta';
 *     gamma = sqrt(gbar * gbar + beta' * beta');  cs = gbar / gamma;  sn = beta' / gamma;  phi = cs * phibar;  phibar = sn * phibar;
 *     w = T(((double(v) - oldeps * double(w1)) - delta * double(w2)) / gamma);  x = T(double(x) + phi * double(w));  w1 <- w2, w2 <- w;
 *     gmax = max(gmax, gamma);  gmin = min(gmin, gamma);  rnorm = phibar;  the stop test;  then v = T(double(z) / beta'), oldb = beta, beta = beta'.
 *   The sums b.b, b.T(minv b), r2.z and v.y' are accumulated in fp64 from the rounded T values in cvr_cg_device's fixed tree (1024 workgroups of 256
 *   threads, each thread over its 16-byte packets in order, then lanes, wavefronts and workgroups in a fixed order; no atomics): a call gives the same
 *   bits every time, whatever the alignment of b_dev, x_dev and minv_dev.
 * Stop rule, evaluated on the device after every step and once at the start:
 *   rnorm finite and rnorm <= rtol * b_norm is CVR_CG_CONVERGED.  The step that finds it has applied its update of x and writes no v.  beta' == 0 is no
 *   breakdown: it makes phibar 0, which ends in this test even at rtol = 0.
 *   alfa not finite, r2.z negative or not finite (M not positive definite, or a NaN), gamma zero or not finite, or phi / gamma not finite:
 *   CVR_CG_BREAKDOWN, found before x is touched, so x, iterations, residual_norm and info stay at the last iterate's.
 *   At the start, in this order: b.b == 0: x = 0, 0 iterations, converged, residual_norm = 0;  r2.z negative or not finite: CVR_CG_BREAKDOWN with 0
 *   iterations and x untouched (residual_norm = sqrt(r2.z), not finite or NaN);  beta <= rtol * b_norm: converged with 0 iterations and x untouched.  A NaN
 *   or an Inf in b makes r2.z not finite.  After the start info->anorm = 0 and info->acond = 0; after a step anorm = sqrt(tnorm2), acond = gmax / gmin
 *   (oldb of step 1 is the start's beta, so tnorm2 carries r2.z of the start, as in Paige and Saunders' own code).
 *   max_iters steps without a stop: CVR_CG_MAX_ITERS with x the last iterate.  max_iters = 0 forms and tests the start only (spmv_count == 1).
 * residual_norm is rnorm = phibar, the recurrence's ||b - (A - shift I) x|| in the M^-1 norm (the 2-norm without minv_dev); b_norm is the same norm of b.
 * check_every: as for cvr_cg_device -- x, iterations, status, residual_norm, b_norm and info are bit for bit the same for every check_every; only
 * spmv_count (1 + one per step enqueued) and seconds differ.  Three vector launches beside the SpMV per step.
 * Ordering: as cvr_cg_device; makes the handle's device current.
 * Errors, in this order.  Before any device work and before the handle is looked at: cvr_cg_device's argument checks; shift not finite ("shift" in
 * cvr_last_error): CVR_ERR_INVALID.  Then: before cvr_preprocess: CVR_ERR_STATE; nrows != ncols: CVR_ERR_INVALID. */
int cvr_minres_device(cvr_handle *h, const void *b_dev, void *x_dev, double shift, const cvr_cg_options *opt, cvr_cg_result *res, cvr_minres_info *info,
                      void *stream);
/* the same with host b and x (nrows values each; x in and out), as cvr_cg; opt->minv_dev stays a device pointer */
int cvr_minres(cvr_handle *h, const void *b_host, void *x_host, double shift, const cvr_cg_options *opt, cvr_cg_result *res, cvr_minres_info *info);

/* ---- the sparse matrix-matrix product C = A B in CSR, on the device, with reproducible bits -----------------
 * A (m x k) and B (k x n) are cvr_csr_views of the same is_f32, both of host arrays or both of arrays in the memory of `device`; T = float or double.
 * A may have unsorted rows and duplicate entries.  B's rows must be strictly ascending in column (sorted, no duplicates): checked on the device, a
 *   violation is CVR_ERR_INVALID and cvr_last_error names the lowest offending row ("B row <r>").  A result satisfies this, so products chain.
 * C is a CSR with int64 row pointers, row_ptr[0] = 0, every row strictly ascending in column.  Entry (i, j) exists iff some position p of A's row i
 *   and some position q of B's row col_A[p] have col_B[q] = j: the pattern is structural, an entry whose terms cancel to 0.0 stays.  Its value is
 *   acc = +0; acc = T(acc + T(a[p] * b[q])) over those (p, q) in ascending p (q is unique for each p): the product and the sum each rounded once in
 *   T, no fused multiply-add.  The bits are the same on every call, for host and device arrays, for every alignment of the input arrays and for
 *   every launch plan; tests/spgemm_model.py states them in numpy and cvr_spgemm_host computes them in host code.
 * cvr_spgemm_create checks the views, copies the two patterns (the object keeps nothing of the caller's) and runs, as one submission on `stream`:
 *   the bound pass (products[i] = the sum over A's row i of nnz(B row col_A[p]), int64; its total and maximum), the rows binned into classes by
 *   products[i] in row order -- empty; group (products < group_limit): lanes_per_row lanes of a wavefront and a table in LDS per row; block
 *   (products < block_limit): a workgroup and one LDS table per row; spill: a workgroup and a table in a global arena --, a symbolic kernel per LDS
 *   class that counts each row's distinct columns, the scan to row_ptr, ONE read-back (nnz(C) with the statistics), the allocation of C and a
 *   numeric kernel per class that writes each row out sorted.  Only when rows spill does a second read-back follow: the arena is allocated behind the
 *   first one, sized by the largest row it reported (a table of twice that row's possible columns, as many tables as fit 256 MiB, at least one;
 *   CVR_ERR_NOMEM when one table does not fit), then the spill rows are counted and row_ptr is scanned again.  A product without spill rows allocates
 *   no arena.  It returns with the stream idle.  CVR_DEBUG=spgemm_limits=<group>:<block>, read by every
 *   cvr_spgemm_create, lowers the two limits: it changes the plan and never a bit.  The row pointers and columns of device arrays are checked as
 *   cvr_create checks them, with that call's small read-backs in front of the submission.
 * cvr_spgemm_get_info fills a cvr_spgemm_info_t.  cvr_spgemm_csr_device fills a view of C (arrays owned by the object, arrays_on_device = 1) that
 *   goes straight into cvr_create or a cvr_precond_* constructor.  cvr_spgemm_export copies C to host arrays (row_ptr: m + 1, col_idx and vals: nnz;
 *   each pointer may be NULL); it waits for the device first.
 * cvr_spgemm_numeric_device runs the numeric step alone, into the existing C, with new value arrays of A and B in device memory, indexed like the
 *   views' vals at creation (same patterns): it only enqueues on `stream`, and gives the bits a fresh create with those values would give.
 * cvr_spgemm_host is the pure-host twin (host arrays only), in two calls: with c_col_idx == NULL and c_vals == NULL it fills c_row_ptr (m + 1)
 *   alone, with both it fills all three.  The same checks, the same errors, the same bits; *bad_row = the offending row of B, else -1.
 * Errors.  CVR_ERR_INVALID: a null argument; the views' is_f32 differ; a->ncols != b->nrows; one view of host and one of device arrays; a malformed
 *   CSR (cvr_create's checks of a view, without its limit that a vector of ncols values fit 4 GiB: the product has no x); B not strictly ascending; b->ncols >= 2^31 - 1; a null value array to cvr_spgemm_numeric_device.
 *   CVR_ERR_NO_DEVICE, CVR_ERR_NOMEM (nothing is left allocated) and CVR_ERR_HIP as elsewhere.  m = 0, k = 0, n = 0 and nnz = 0 are valid: an empty
 *   C, nothing launched past the bound pass.  cvr_spgemm_destroy(NULL) is CVR_OK. */
typedef struct cvr_spgemm cvr_spgemm;
typedef struct {
    int64_t nrows, ncols, inner, nnz;          /* m, n, k, nnz(C)                                                           */
    int64_t products, max_row_products;        /* the bound pass: the sum and the maximum of products[i]                    */
    int64_t rows_empty, rows_group, rows_block, rows_spill;
    int64_t group_limit, block_limit;          /* the limits in force for this object (32 and 4096 unless lowered)          */
    int32_t is_f32, lanes_per_row;             /* the lanes of a group row (8)                                              */
    double  symbolic_s, numeric_s;             /* host seconds of cvr_spgemm_create up to the read-back, and behind it      */
} cvr_spgemm_info_t;
int cvr_spgemm_create(cvr_spgemm **out, const cvr_csr_view *a, const cvr_csr_view *b, int32_t device, void *stream);
int cvr_spgemm_get_info(const cvr_spgemm *g, cvr_spgemm_info_t *info);
int cvr_spgemm_csr_device(const cvr_spgemm *g, cvr_csr_view *c);
int cvr_spgemm_export(const cvr_spgemm *g, int64_t *row_ptr, int32_t *col_idx, void *vals);
int cvr_spgemm_numeric_device(cvr_spgemm *g, const void *a_vals_dev, const void *b_vals_dev, void *stream);
int cvr_spgemm_destroy(cvr_spgemm *g);
int cvr_spgemm_host(const cvr_csr_view *a, const cvr_csr_view *b, int64_t *c_row_ptr, int32_t *c_col_idx, void *c_vals, int64_t *bad_row);

/* ---- a few extreme eigenpairs of a symmetric A on the device: thick-restart Lanczos --------------------------
 * cvr_eigsh_device / cvr_eigsh find the nev algebraically largest or smallest eigenvalues of a symmetric A and their eigenvectors: the Lanczos process
 * with full reorthogonalisation (classical Gram-Schmidt applied twice, GMRES's kernels) and the thick restart of Wu and Simon (SIAM J. Matrix Anal. Appl.
 * 22, 2000).  Any single-GPU handle of a square matrix works, in fp32 or fp64 and in any layout (fused-preprocess, image-cache, mutable and transposed
 * handles included): the solver only goes through cvr_spmv_device's launch path.  The caller guarantees symmetry; nothing checks it.  (cvr_power_iteration
 * gives one dominant pair and has no stop test.) */
#define CVR_EIG_MAX_NCV 64
#define CVR_EIG_LARGEST  0   /* algebraically largest  ("LA") */
#define CVR_EIG_SMALLEST 1   /* algebraically smallest ("SA") */
#define CVR_EIG_CONVERGED    0
#define CVR_EIG_MAX_RESTARTS 1
#define CVR_EIG_BREAKDOWN    2   /* a sum that is not finite: NaN/Inf in A or v0, or v0 == 0 */
#define CVR_EIG_INVARIANT    3   /* the Krylov space closed with fewer than nev columns; nconv exact pairs returned */
#define CVR_EIG_EPS23 3.666852862501036e-11   /* eps23 below: ARPACK's eps^(2/3) for eps = 2^-52, as this literal */

typedef struct {
    int32_t nev;              /* pairs wanted, >= 1                                                          */
    int32_t ncv;              /* m, the columns of the basis: 0 = min(n, max(2 * nev + 1, 20), 64), else nev + 2 .. CVR_EIG_MAX_NCV */
    int32_t which;            /* CVR_EIG_LARGEST or CVR_EIG_SMALLEST                                         */
    int32_t max_restarts;     /* >= 0; 0: one cycle of m steps                                               */
    double  tol;              /* finite, >= 0: pair c has converged when e_c <= tol * max(eps23, |theta_c|)  */
    int32_t reserved[4];      /* must be 0 (CVR_ERR_INVALID otherwise)                                       */
} cvr_eig_options;        /* 40 bytes */
typedef struct {
    int32_t nconv;            /* wanted pairs that have converged (CVR_EIG_INVARIANT: the pairs returned)    */
    int32_t status;           /* CVR_EIG_*                                                                   */
    int32_t restarts;         /* restarts done                                                               */
    int32_t spmv_count;       /* steps enqueued, those behind a stop included                                */
    double  seconds;          /* HIP events around everything enqueued                                       */
    double  max_estimate;     /* the largest e_c / max(eps23, |theta_c|) among the returned pairs            */
} cvr_eig_result;         /* 32 bytes */

/* nev = 1, ncv = 0, CVR_EIG_LARGEST, max_restarts = 100, tol = 1e-8, reserved = 0 */
void cvr_eig_default_options(cvr_eig_options *opt);
/* v0_dev: the start vector, n = nrows values of the handle's type T in the memory of the handle's device, any alignment of T; it is not written.
 * evals_host receives the eigenvalues found, nev doubles in ascending order (CVR_EIG_INVARIANT: the first nconv; CVR_EIG_BREAKDOWN: nothing is written,
 * to evals_host or to evecs_dev).  evecs_dev may be NULL (values only: the same evals); otherwise the vector of evals_host[c] is column c, n values of T
 * at evecs_dev + c * ldv, ldv >= n, any alignment; values at positions >= n of a column are not touched.
 * The buffers of the call are the library's, in one allocation per call: m + 1 basis vectors of info.x_elems values whose element ncols stays 0, w of
 * info.yext_elems values, and nev + (m - nev) / 2 more vectors that take the restart's output (which is then copied back over the basis: no kernel reads
 * a column that another workgroup of the same launch may be writing).
 * Arithmetic, T = the handle's type, m = ncv; every operation below is rounded on its own (no fused multiply-add); scalars are fp64.  Every sum a.b is
 * cvr_cg_device's fixed tree over the terms double(a_i) * double(b_i), and each sum has its own 1024 partials.
 *   Start: s = v0.v0.  s not finite or not > 0: CVR_EIG_BREAKDOWN, nothing is written.  Otherwise v_0 = T(double(v0) / sqrt(s)).  The first cycle runs
 *     the steps j = 0 .. m-1; a cycle behind a restart that kept k columns runs j = k .. m-1.
 *   Step j (basis column j): w = A v_j through cvr_spmv_device's launch path (bit for bit its y).  Then cvr_gmres_device's two Gram-Schmidt passes
 *     against v_0 .. v_j, unchanged.  Pass 1: h_i = v_i . w for i = 0..j, all on the same w; then t = double(w), t = t - h_0 * double(v_0), ...,
 *     t = t - h_j * double(v_j) in that order, w = T(t) (one rounding to T).  Pass 2, the same on the new w with d_i = v_i . w.
 *     alpha_j = h_j + d_j (the other coefficients only orthogonalise: they do not enter the projected matrix).
 *     ww1 = w.w between the two passes, ww = w.w of the new w;  beta_(j+1) = sqrt(ww).  ww1, ww or alpha_j not finite: CVR_EIG_BREAKDOWN.
 *     ww <= 0.25 * ww1 -- which beta_(j+1) == 0 satisfies --: the Krylov space is invariant (closed) with q = j + 1 columns, and the cycle ends there
 *     (below).  (The second pass takes away only what rounding left of the first; where it halves the norm once more, w is rounding noise inside
 *     the span of the basis -- "twice is enough", Daniel, Gragg, Kaufman and Stewart, Math. Comp. 30, 1976 -- and normalising it would put a column
 *     of noise into the basis.  A test for an exact zero alone would miss every closed space but the exactly representable ones.)
 *     Otherwise v_(j+1) = T(double(w) / beta_(j+1)).
 *   The projected matrix P of q columns (q = m at the end of a full cycle), symmetric: in the first cycle tridiagonal, P_(j,j) = alpha_j,
 *     P_(j+1,j) = beta_(j+1).  Behind a restart that kept k columns: P_(c,c) = theta_c for c < k, the arrow P_(k,c) = s_c in row and column k, and from
 *     there tridiagonal as before (P_(j,j) = alpha_j for j >= k, P_(j+1,j) = beta_(j+1)).  alpha and beta stay in a state cell on the device, which the
 *     host reads once per cycle; theta and s are the host's from the restart.
 *   End of a cycle: cvr_sym_eig_host of P gives theta_0 <= .. <= theta_(q-1) and the orthonormal S.  The wanted pairs are the min(nev, q) at the chosen
 *     end (CVR_EIG_LARGEST: q - nev .. q - 1), kept in ascending order.  The estimate of pair c is e_c = |beta_q * S[q-1,c]| (a closed space: beta_q = 0),
 *     and the pair has converged when e_c <= tol * max(eps23, |theta_c|) with eps23 = CVR_EIG_EPS23, the decimal literal above (not a pow call).
 *     nconv = the wanted pairs that have converged.  The cycle ends the call
 *       when nconv == nev, or the space is closed with q >= nev: CVR_EIG_CONVERGED (a closed space: every pair is exact and nconv = nev);
 *       when the space is closed with q < nev: CVR_EIG_INVARIANT, the q pairs are returned and nconv = q;
 *       when restarts == max_restarts: CVR_EIG_MAX_RESTARTS, the wanted pairs as they are, nconv as counted.
 *     max_estimate = the largest e_c / max(eps23, |theta_c|) among the returned pairs.
 *   Thick restart: k = nev + min(nconv, (m - nev) / 2) in integers (at most m - 1, because m >= nev + 2).  The k Ritz pairs at the wanted end are kept, in
 *     ascending order (CVR_EIG_LARGEST: c-th kept pair = pair m - k + c): theta_c, s_c = beta_m * S[m-1,c], and per value
 *     u = +0, u = u + S[l,c] * double(v_l) for l = 0 .. m-1 ascending (each product and each addition rounded on its own), new v_c = T(u).
 *     The new v_k is the old v_m.  The cycle continues at step k.
 *   The eigenvectors returned are formed by the same rule from the q columns into evecs_dev; they are not renormalised.
 * restarts = the restarts done; spmv_count = the steps enqueued: m in the first cycle and m - k in each later one, whether or not a breakdown or a closed
 * space ends the cycle early (the kernels behind it return without writing).  Five vector launches beside the SpMV per step, whatever j; a restart is one
 * launch of the product and two device copies.
 * Ordering: everything is enqueued on `stream` (NULL = HIP's null stream), which is synchronised once per cycle and once before the call returns: it
 * cannot be captured in a HIP graph.  A mutable handle's image is ordered with other launches of the handle as cvr_spmv_device orders it.  Makes the
 * handle's device current.
 * Errors, in this order, before any device work and before the handle is looked at, each CVR_ERR_INVALID with the name in cvr_last_error: null h, v0,
 * evals, opt or res; nev < 1; ncv other than 0 or nev + 2 .. CVR_EIG_MAX_NCV; which not one of the two values; max_restarts < 0; tol negative or not
 * finite; a non-zero reserved word; ldv < 1 when evecs is not NULL.  Then: before cvr_preprocess: CVR_ERR_STATE; nrows != ncols: CVR_ERR_INVALID;
 * ncv > n, or the default ncv below nev + 2 (n too small): CVR_ERR_INVALID; ldv < n with evecs: CVR_ERR_INVALID; no device memory for the call's
 * buffers: CVR_ERR_NOMEM, nothing allocated. */
int cvr_eigsh_device(cvr_handle *h, const void *v0_dev, double *evals_host, void *evecs_dev, int64_t ldv, const cvr_eig_options *opt, cvr_eig_result *res,
                     void *stream);
/* the same with host v0 and evecs (column c at evecs_host + c * ldv): copied up, cvr_eigsh_device on the handle's stream, the vectors copied back */
int cvr_eigsh(cvr_handle *h, const void *v0_host, double *evals_host, void *evecs_host, int64_t ldv, const cvr_eig_options *opt, cvr_eig_result *res);
/* The dense symmetric eigensolver of the projected problem, on the host: all eigenpairs of a symmetric m x m matrix, 1 <= m <= CVR_EIG_MAX_NCV, by the
 * cyclic Jacobi method by rows in Rutishauser's form (threshold sweeps, rotations skipped where they cannot move the diagonal), plain fp64 in a fixed
 * order: the same input gives the same bits every time.  Element (i, j) with i >= j is read at a[i + j * lda]; the other triangle is never read.
 * w receives the eigenvalues ascending; equal values keep the order of the diagonal positions they ended at.  z (may be NULL) receives the
 * orthonormal eigenvector of w[c] at z + c * ldz, its sign fixed so that its component of largest magnitude (the first of them) is positive.
 * Errors: m out of range, null a or w, lda < m, ldz < m with z, an element of the triangle that is not finite: CVR_ERR_INVALID. */
int cvr_sym_eig_host(int32_t m, const double *a, int32_t lda, double *w, double *z, int32_t ldz);

/* ---- a block of extreme eigenpairs with a preconditioner: LOBPCG ----------------------------------------------
 * cvr_lobpcg_device / cvr_lobpcg find the k = nev (1 .. CVR_LOBPCG_MAX_BLOCK) algebraically smallest or largest eigenvalues of a symmetric A and their
 * eigenvectors by the locally optimal block preconditioned conjugate gradient method (Knyazev, SIAM J. Sci. Comput. 23, 2001), optionally with a
 * preconditioner object p of ANY kind (block-Jacobi, Chebyshev, ILU(0), FSAI, the AMG kinds, multicolour SGS): the call only goes through the object's
 * apply, one column at a time, which is cvr_precond_apply_device's path, and through cvr_spmv_device's launch path, so any single-GPU handle of a square
 * matrix works, in fp32 or fp64 and in any layout.  The caller guarantees symmetry (and, with p, that p suits A); nothing checks it.  p == NULL: W = R.
 * A preconditioner approximates A^-1 and only helps the lower end: p with CVR_EIG_LARGEST is an error.
 * Not in this version, each left out on purpose: soft locking of converged columns (W is always rebuilt from all k columns, and all k columns go on
 * being combined until every one has converged); the generalised problem A x = lambda B x; constraints (a deflation block Y); a k-wide product
 * through cvr_spmm_device (the block is column-major and takes k single-vector products, so every handle works, not only nvec >= 2 ones); more than
 * 8 columns; cvr_eigsh is unchanged.
 * X: column-major like cvr_eigsh's evecs, column c at X + c * ldx, ldx >= n, n values of the handle's type T each, any alignment of T; it carries the
 * start block in and the eigenvectors out (values at positions >= n of a column are neither read nor written).  evals_host and resnorms_host receive k
 * doubles each: theta_c ascending (CVR_EIG_LARGEST: the k largest, ascending) and ||A x_c - theta_c x_c||_2 as the solver formed it.
 * CVR_EIG_BREAKDOWN: nothing is written, to X, evals_host or resnorms_host.
 * Status: CVR_EIG_CONVERGED, CVR_EIG_MAX_ITERS (max_iters iterations done, the block as it is) or CVR_EIG_BREAKDOWN (a sum that is not finite, a
 * start block that is not of full rank to working precision, a column of W whose norm is zero).  Column c has converged when
 * ||A x_c - theta_c x_c||_2 <= tol * max(CVR_EIG_EPS23, |theta_c|), with ||x_c||_2 = 1 to rounding: cvr_eigsh's rule with the true residual in place of
 * the estimate.  The call ends when all k columns have.
 * Arithmetic, T = the handle's type; every operation below is rounded on its own (no fused multiply-add); scalars are fp64.  Every sum a.b is
 * cvr_cg_device's fixed tree over the terms double(a_i) * double(b_i), and each sum has its own 1024 partials: no floating-point atomics, no matrix
 * instructions, the same bits on every call and for every alignment of X.  S = [X W P] has m = 2k columns in the first iteration and when an iteration
 * falls back (below), and 3k columns otherwise; A S = [AX AW AP] is carried beside it.
 *   Rayleigh-Ritz step on m columns (host, plain fp64 in this order).  G = S^T S and H = S^T (A S), the lower triangles (entry (i, j), i >= j, is
 *     S_i . S_j and S_i . (A S)_j).  Cholesky G = L L^T column by column j = 0 .. m-1: s = G_jj, s = s - L_jp * L_jp for p = 0 .. j-1 ascending; a
 *     pivot s that is not finite, not > 0 or not > tau * G_jj is a bad pivot (with m = 3k, where dropping P is always possible,
 *     tau = CVR_LOBPCG_PIVOT_F64 = 2^-30 for fp64 handles and CVR_LOBPCG_PIVOT_F32 = 2^-20 for fp32 ones; with m = k or 2k, tau = 0: s / G_jj is the squared sine of the angle between column j and the columns in front, and the
 *     combination of step 7 loses a factor 1 / sqrt(s / G_jj) of T's precision -- a pivot that is merely positive, 1e-14 say, gives back an A X that
 *     is no longer A times X); L_jj = sqrt(s); for i > j: t = G_ij, t = t - L_ip * L_jp (p ascending), L_ij = t / L_jj.
 *     Y = L^-1 H, column by column: t = H_ij (H_ji above the diagonal), t = t - L_ip * Y_pj for p = 0 .. i-1, Y_ij = t / L_ii.  M = Y L^-T, lower
 *     triangle, row by row: t = Y_ij, t = t - M_ip * L_jp for p = 0 .. j-1, M_ij = t / L_jj.  cvr_sym_eig_host of M gives theta ascending and Z; the k
 *     wanted pairs are the first k (CVR_EIG_LARGEST: the last k), kept ascending.  C = L^-T Z of those: for i = m-1 .. 0: t = Z_ic,
 *     t = t - L_pi * C_pc for p = i+1 .. m-1 ascending, C_ic = t / L_ii.
 *   0. Start: S = [X] (the caller's block, copied), A S by k products through cvr_spmv_device's launch path (bit for bit its y), the Rayleigh-Ritz
 *      step with m = k, and X = T(S C), AX = T((A S) C) by step 7's sums (no P).  A bad pivot here: CVR_EIG_BREAKDOWN.  The block is orthonormal and
 *      theta are its Ritz values from here on.
 *   1. R_c = T(double(AX_c) - theta_c * double(X_c)) and rr_c = R_c . R_c, one launch for all columns.
 *   2. W_c = M R_c by the object's apply (k applies), or W = R without an object.  There is no locking: all k columns, every iteration.
 *   3. Twice: h_ic = X_i . W_c for all i and c on the same W; then per value t = double(w_c), t = t - h_0c * double(x_0), ..,
 *      t = t - h_(k-1)c * double(x_(k-1)), w_c = T(t).  Then ww_c = W_c . W_c and W_c = T(double(W_c) / sqrt(ww_c)); a ww_c that is not finite or not
 *      > 0 ends the call with CVR_EIG_BREAKDOWN (seen at the read-back of step 6).
 *   4. AW = A W by k products.
 *   5. The lower triangles of G and H over the m columns, in fp64.
 *   6. The single read-back of the iteration: G, H, rr and ww.  The residual norms are sqrt(rr_c): they belong to the X of step 1, the convergence
 *      test uses them, and so the X returned is the X they belong to.  All converged: CVR_EIG_CONVERGED.  Otherwise, when max_iters iterations are
 *      done: CVR_EIG_MAX_ITERS (that last pass enqueues step 1 and the read-back only).  Otherwise the Rayleigh-Ritz step; a bad pivot (or an M that
 *      is not finite) with m = 3k: P is dropped, m = 2k, restarts_without_p counts it, and the step is tried once more on the top-left 2k x 2k blocks
 *      of the same G and H; a bad pivot at 2k: CVR_EIG_BREAKDOWN.
 *   7. Into the second set of blocks (the two sets alternate: no kernel reads a column that another workgroup of the same launch may be writing):
 *      per value u = +0, u = u + C_lc * double(S_l) for l = 0 .. m-1 ascending, X'_c = T(u); AX'_c the same over A S.  P'_c and AP'_c are those sums
 *      over l = k .. m-1 only (C~, which is C with its first k rows zeroed).  Then pp_c = P'_c . P'_c and, where pp_c is finite and > 0,
 *      P'_c = T(double(P'_c) / sqrt(pp_c)) and AP'_c likewise (a P'_c that is zero stays zero, and the next iteration falls back).  C is uploaded once
 *      per iteration.  theta = the new Ritz values; the next iteration has m = 3k.
 * max_iters = 0 returns the Rayleigh-Ritz vectors of the start block with their residual norms and CVR_EIG_MAX_ITERS (or CVR_EIG_CONVERGED).
 * iterations = the combinations of step 7 done; spmv_count = k * (1 + the iterations enqueued) and precond_applies = k * (the iterations enqueued)
 * (with p), where the iteration that finds all columns converged counts as enqueued: its steps 2 to 5 were.  max_rel_residual = the largest
 * sqrt(rr_c) / max(CVR_EIG_EPS23, |theta_c|).
 * The buffers of the call are the library's, in one allocation per call: 13 k vectors (two sets of S and A S and R), each of the larger of
 * info.x_elems and info.yext_elems values, and the partial sums.
 * Ordering: everything is enqueued on `stream` (NULL = HIP's null stream), which is synchronised once per iteration and once before the call returns:
 * it cannot be captured in a HIP graph.  One object serves one stream at a time, as in cvr_precond_apply_device.  Makes the handle's device current.
 * Errors, in this order, before any device work and before the handle is looked at, each CVR_ERR_INVALID with the name in cvr_last_error: null h, X,
 * evals, resnorms, opt or res; nev outside 1 .. CVR_LOBPCG_MAX_BLOCK; which not one of the two values; max_iters < 0; tol negative or not finite; a
 * non-zero reserved word (reserved0, then reserved[]); ldx < 1; p != NULL with CVR_EIG_LARGEST.  Then: before cvr_preprocess: CVR_ERR_STATE;
 * nrows != ncols, n < 3 * nev, ldx < n: CVR_ERR_INVALID; p of another n, type or device than the handle: CVR_ERR_INVALID; no device memory for the
 * call's buffers: CVR_ERR_NOMEM, nothing allocated. */
#define CVR_LOBPCG_MAX_BLOCK 8
#define CVR_LOBPCG_PIVOT_F64 9.313225746154785e-10   /* 2^-30: the smallest pivot / G_jj the Cholesky step accepts, fp64 handles */
#define CVR_LOBPCG_PIVOT_F32 9.5367431640625e-07      /* 2^-20: fp32 handles */
#define CVR_EIG_MAX_ITERS    4   /* cvr_lobpcg only: max_iters iterations done before every column converged */
typedef struct {
    int32_t nev;              /* k, the columns of the block: 1 .. CVR_LOBPCG_MAX_BLOCK                        */
    int32_t which;            /* CVR_EIG_SMALLEST (default) or CVR_EIG_LARGEST                                 */
    int32_t max_iters;        /* >= 0, default 200                                                             */
    int32_t reserved0;        /* must be 0                                                                     */
    double  tol;              /* finite, >= 0, default 1e-8                                                    */
    int32_t reserved[4];      /* must be 0 (CVR_ERR_INVALID otherwise)                                         */
} cvr_lobpcg_options;     /* 40 bytes */
typedef struct {
    int32_t nconv;            /* columns that have converged                                                   */
    int32_t status;           /* CVR_EIG_CONVERGED, CVR_EIG_MAX_ITERS or CVR_EIG_BREAKDOWN                     */
    int32_t iterations;       /* combinations (step 7) done                                                    */
    int32_t spmv_count;       /* products enqueued                                                             */
    int32_t precond_applies;  /* applies of the object enqueued                                                */
    int32_t restarts_without_p;          /* iterations that fell back to S = [X W]                              */
    double  seconds;          /* HIP events around everything enqueued                                         */
    double  max_rel_residual; /* the largest ||r_c|| / max(eps23, |theta_c|) of the returned block             */
} cvr_lobpcg_result;      /* 40 bytes */
/* nev = 1, CVR_EIG_SMALLEST, max_iters = 200, tol = 1e-8, reserved = 0 */
void cvr_lobpcg_default_options(cvr_lobpcg_options *opt);
int cvr_lobpcg_device(cvr_handle *h, const cvr_precond *p, void *X_dev, int64_t ldx, double *evals_host, double *resnorms_host, const cvr_lobpcg_options *opt,
                      cvr_lobpcg_result *res, void *stream);
/* the same with a host X (column c at X_host + c * ldx): copied up, cvr_lobpcg_device on the handle's stream, the block copied back */
int cvr_lobpcg(cvr_handle *h, const cvr_precond *p, void *X_host, int64_t ldx, double *evals_host, double *resnorms_host, const cvr_lobpcg_options *opt,
               cvr_lobpcg_result *res);

/* ---- a few leading singular triplets of any A on the device: thick-restart Golub-Kahan-Lanczos ---------------
 * cvr_svds_device / cvr_svds find the nev largest singular values of A (nrows x ncols, any shape) with their left and right singular vectors:
 * Golub-Kahan-Lanczos bidiagonalisation with full two-sided reorthogonalisation (classical Gram-Schmidt applied twice, GMRES's kernels) and a thick
 * restart on Ritz vectors (Baglama and Reichel, SIAM J. Sci. Comput. 27, 2005; Hernandez, Roman and Tomas, ETNA 31, 2008).  It is the rectangular twin
 * of cvr_eigsh_device and works on A itself, not on A^T A: the condition number is not squared and nothing fills in.  `a` is any single-GPU handle,
 * in fp32 or fp64 and in any layout, and `at` a handle of A^T (cvr_options.transpose = 1 on the same CSR; `a` itself for a symmetric A), as in
 * cvr_lsqr_device: the solver only goes through cvr_spmv_device's launch path of the two handles.
 * Not in this version, each left out on purpose: the smallest singular values (they need harmonic-Ritz restarts to be useful); shift-and-invert; more
 * than one GPU; a block variant; an implicit A^T without a second handle.
 * v0_dev: the start vector, ncols values of the handles' type T in the memory of their device, any alignment of T; it is not written.
 * svals_host receives the singular values found, nev doubles in descending order (CVR_EIG_INVARIANT: the first nconv, which may be none;
 * CVR_EIG_BREAKDOWN: nothing is written, to svals_host, U_dev or V_dev; whatever is not written keeps the caller's bytes).  U_dev and V_dev may each
 * be NULL independently (the same svals); otherwise the left vector of svals_host[c] is column c of U_dev, nrows values of T at U_dev + c * ldu,
 * ldu >= nrows, and the right one column c of V_dev, ncols values at V_dev + c * ldv, ldv >= ncols, any alignment; values beyond the column length,
 * and columns beyond the returned count, are never touched.
 * The buffers of the call are the library's, in one allocation per call: m + 1 right-basis columns v_0 .. v_m whose stride covers a's info.x_elems
 * and whose element ncols stays 0; m left-basis columns u_0 .. u_(m-1) whose stride covers at's info.x_elems and whose element nrows stays 0; w of
 * a's info.yext_elems values and z of at's; and nev + (m - nev) / 2 more columns of either kind that take the restart's output (which is then copied
 * back over the bases: no kernel reads a column that another workgroup of the same launch may be writing).
 * Arithmetic, T = the handles' type, m = ncv; every operation below is rounded on its own (no fused multiply-add); scalars are fp64.  Every sum a.b is
 * cvr_cg_device's fixed tree over the terms double(a_i) * double(b_i), and each sum has its own 1024 partials.
 *   Start: s = v0.v0.  s not finite or not > 0: CVR_EIG_BREAKDOWN, nothing is written.  Otherwise v_0 = T(double(v0) / sqrt(s)).  The first cycle runs
 *     the steps j = 0 .. m-1; a cycle behind a restart that kept k triplets runs j = k .. m-1.
 *   Step j, left half: w = A v_j through cvr_spmv_device's launch path of `a` (bit for bit its y).  Then cvr_gmres_device's two Gram-Schmidt passes
 *     against u_0 .. u_(j-1), unchanged.  Pass 1: h_i = u_i . w for i < j, all on the same w; then t = double(w), t = t - h_0 * double(u_0), ...,
 *     t = t - h_(j-1) * double(u_(j-1)) in that order, w = T(t) (one rounding to T).  Pass 2, the same on the new w.  For j = 0 there is no column:
 *     nothing is summed or subtracted and w stays as it is.  ww1 = w.w behind pass 1 and ww = w.w behind pass 2 (for j = 0 the same sum twice: w.w
 *     of A v_0), as in cvr_eigsh_device; alpha_j = sqrt(ww).  The Gram-Schmidt coefficients only orthogonalise: they do not enter the projected
 *     matrix.  ww1 or ww not finite: CVR_EIG_BREAKDOWN.  ww <= 0.25 * ww1 -- which alpha_j == 0 satisfies, and for j = 0 nothing else does --: the left
 *     half is closed at step j ("twice is enough": see cvr_eigsh_device; ww1 is taken behind pass 1 and not in front of it, because in front of it w
 *     holds its whole component beta_j u_(j-1), or the spike, which says nothing about closure).  Otherwise u_j = T(double(w) / alpha_j).
 *   Step j, right half: z = A^T u_j through the launch path of `at`; the same two passes against v_0 .. v_j (j + 1 columns); zz1 and zz likewise;
 *     beta_(j+1) = sqrt(zz); zz1 or zz not finite: CVR_EIG_BREAKDOWN; zz <= 0.25 * zz1: the right half is closed at step j; otherwise
 *     v_(j+1) = T(double(z) / beta_(j+1)).
 *   The projected matrix B has p rows (left vectors) and q columns (right vectors), p = q = m at the end of a full cycle.  In the first cycle it is
 *     upper bidiagonal: B_(j,j) = alpha_j, B_(j,j+1) = beta_(j+1).  Behind a restart that kept k triplets: B_(c,c) = sigma_c for c < k, the spike
 *     B_(c,k) = s_c in column k, and from there bidiagonal as before (B_(j,j) = alpha_j for j >= k, B_(j,j+1) = beta_(j+1)).  alpha and beta stay in
 *     a state cell on the device, which the host reads once per cycle; sigma and s are the host's from the restart.
 *     A right half closed at step j: A^T u_j lies in span(v_0 .. v_j); p = q = j + 1, B is square (beta_(j+1) is not part of it) and its q triplets are
 *     exact: cvr_eigsh_device's closed-space rule.  A left half closed at step j: A v_j lies in span(u_0 .. u_(j-1)); p = j and q = j + 1, B is the
 *     j x (j + 1) matrix whose last column holds beta_j in row j - 1 (or the spike, when j = k), and its j triplets are exact.  j = 0 (A v_0 = 0, a
 *     zero matrix for one): there is nothing to return: CVR_EIG_INVARIANT with nconv = 0, and nothing is written to svals_host, U_dev or V_dev.
 *   End of a cycle: cvr_svd_host of B gives sigma_0 >= .. >= sigma_(p-1), Q (p x p) and P (q x p) with B = Q diag(sigma) P^T.  The wanted triplets are
 *     the first min(nev, p).  The estimate of triplet c is e_c = |beta_m * Q[m-1,c]| (a closed space: 0), and the triplet has converged when
 *     e_c <= tol * max(eps23, sigma_c) with eps23 = CVR_EIG_EPS23.  nconv = the wanted triplets that have converged.  The cycle ends the call
 *       when nconv == nev, or a half is closed with p >= nev: CVR_EIG_CONVERGED (a closed space: every triplet is exact and nconv = nev);
 *       when a half is closed with p < nev: CVR_EIG_INVARIANT, the p triplets are returned and nconv = p;
 *       when restarts == max_restarts: CVR_EIG_MAX_RESTARTS, the wanted triplets as they are, nconv as counted.
 *     max_estimate = the largest e_c / max(eps23, sigma_c) among the returned triplets (none returned: 0).
 *   Thick restart: k = nev + min(nconv, (m - nev) / 2) in integers (at most m - 1).  The k leading triplets are kept: sigma_c, s_c = beta_m * Q[m-1,c],
 *     and per value u = +0, u = u + P[l,c] * double(v_l) for l = 0 .. m-1 ascending (each product and each addition rounded on its own),
 *     new v_c = T(u); new u_c the same from Q[l,c] and u_l.  The new v_k is the old v_m.  The cycle continues at step k.
 *   The vectors returned are formed by the same rule from the p left and q right columns into U_dev and V_dev; they are not renormalised.
 * restarts = the restarts done; spmv_count = the products enqueued through both handles: 2 m in the first cycle and 2 (m - k) in each later one,
 * whether or not a breakdown or a closed space ends the cycle early (the kernels behind it return without writing).  Per step two products and ten
 * vector launches (five per half: sums, update, sums, update, norm; step 0 has eight, its left half having no sums); a restart is two launches of
 * the product and three device copies.
 * Ordering: everything is enqueued on `stream` (NULL = HIP's null stream), which is synchronised once per cycle and once before the call returns: it
 * cannot be captured in a HIP graph.  Mutable handles' images are ordered as cvr_spmv_device orders them.  Makes the handles' device current.
 * Errors, in this order, before any device work and before a handle is looked at, each CVR_ERR_INVALID with the name in cvr_last_error: null a, at,
 * v0, svals, opt or res; nev < 1; ncv other than 0 or nev + 2 .. CVR_SVD_MAX_NCV; max_restarts < 0; reserved0 not 0; tol negative or not finite; a
 * non-zero word of reserved[]; ldu < 1 with U; ldv < 1 with V.  Then: either handle before cvr_preprocess: CVR_ERR_STATE.  Then, each
 * CVR_ERR_INVALID: at not ncols x nrows of a; different value types; different devices; ncv > min(nrows, ncols), or the default ncv below nev + 2
 * (the matrix too small); ldu < nrows with U; ldv < ncols with V.  No device memory for the call's buffers: CVR_ERR_NOMEM, nothing allocated.
 * The status codes are cvr_eigsh's (CVR_EIG_CONVERGED, CVR_EIG_MAX_RESTARTS, CVR_EIG_BREAKDOWN, CVR_EIG_INVARIANT). */
#define CVR_SVD_MAX_NCV 64
typedef struct {
    int32_t nev;              /* triplets wanted, >= 1                                                       */
    int32_t ncv;              /* m: 0 = min(min(nrows, ncols), max(2 * nev + 1, 20), 64), else nev + 2 .. CVR_SVD_MAX_NCV, and <= min(nrows, ncols) */
    int32_t max_restarts;     /* >= 0; 0: one cycle of m steps                                               */
    int32_t reserved0;        /* must be 0                                                                   */
    double  tol;              /* finite, >= 0: triplet c has converged when e_c <= tol * max(eps23, sigma_c) */
    int32_t reserved[4];      /* must be 0 (CVR_ERR_INVALID otherwise)                                       */
} cvr_svd_options;        /* 40 bytes */
typedef struct {
    int32_t nconv;            /* wanted triplets that have converged (CVR_EIG_INVARIANT: the triplets returned) */
    int32_t status;           /* CVR_EIG_CONVERGED, CVR_EIG_MAX_RESTARTS, CVR_EIG_BREAKDOWN or CVR_EIG_INVARIANT */
    int32_t restarts;         /* restarts done                                                               */
    int32_t spmv_count;       /* products enqueued through both handles, those behind a stop included        */
    double  seconds;          /* HIP events around everything enqueued                                       */
    double  max_estimate;     /* the largest e_c / max(eps23, sigma_c) among the returned triplets           */
} cvr_svd_result;         /* 32 bytes */
/* nev = 1, ncv = 0, max_restarts = 100, tol = 1e-8, reserved = 0 */
void cvr_svd_default_options(cvr_svd_options *opt);
int cvr_svds_device(cvr_handle *a, cvr_handle *at, const void *v0_dev, double *svals_host, void *U_dev, int64_t ldu, void *V_dev, int64_t ldv,
                    const cvr_svd_options *opt, cvr_svd_result *res, void *stream);
/* the same with host v0 (ncols values), U (column c at U_host + c * ldu) and V: copied up, cvr_svds_device on a's stream, the vectors copied back */
int cvr_svds(cvr_handle *a, cvr_handle *at, const void *v0_host, double *svals_host, void *U_host, int64_t ldu, void *V_host, int64_t ldv,
             const cvr_svd_options *opt, cvr_svd_result *res);
/* The dense singular value decomposition of the projected matrix, on the host, the sibling of cvr_sym_eig_host: B (p x q, 1 <= p <= q <=
 * CVR_SVD_MAX_NCV + 1, element (i, j) read at b[i + j * ldb]) = Q diag(s) P^T by the one-sided cyclic Jacobi method of Hestenes by rows (plane
 * rotations between rows i < j of B until every pair is orthogonal to 2^-52 of the product of its norms; a row that has fallen below 2^-52 of B's
 * Frobenius norm is a zero singular value and is left alone), plain fp64 in a fixed order: the same input gives the same bits every time.  s receives
 * the p singular values descending; equal values keep the order of the rows they ended at.  uq (may be NULL) receives Q, p x p orthonormal, the left
 * vector of s[c] at uq + c * lduq, its sign fixed so that its component of largest magnitude (the first of them) is positive; vp (may be NULL)
 * receives P, q x p with orthonormal columns, the right vector of s[c] at vp + c * ldvp.  Where s[c] is at most q 2^-52 s[0], the row's direction is
 * rounding noise: that column of P is the unit vector the other columns leave most of (the first of them), orthogonalised against them twice, so P
 * stays orthonormal for rank-deficient B.
 * Errors: p or q out of range, null b or s, ldb < p, lduq < p with uq, ldvp < q with vp, an element that is not finite: CVR_ERR_INVALID. */
int cvr_svd_host(int32_t p, int32_t q, const double *b, int32_t ldb, double *s, double *uq, int32_t lduq, double *vp, int32_t ldvp);

/* the handle's own device vectors (valid until cvr_destroy) and stream */
void *cvr_x_device(cvr_handle *h);
void *cvr_y_device(cvr_handle *h);
void *cvr_stream(cvr_handle *h);
/* `iters` back-to-back launches on the handle's stream and buffers between two HIP events;
 * returns mean seconds per launch.  No host copies.  (bench.py's roofline leg) */
int cvr_spmv_bench(cvr_handle *h, int warmup, int iters, double *mean_s);
/* Diagnostics (no counterpart in the reference, which times its phases with microtime(), spmv.cpp:575 / 1009, 1033 / 1656): a handle
 * created with CVR_DEBUG=phase_clocks in the environment (headline layout: fp64, column phases + window + dictionary) runs the SpMV
 * kernel in a build that stamps the chip's 100-MHz real-time counter per wavefront at entry / prologue done / window barrier passed /
 * loop done / rows stored; this copies the stamps of the last SpMV out: [workgroup][16 wavefronts][8] =
 * {t_entry, t_prologue, t_window (barrier passed), t_loop_end, t_stored, XCC id, t_arrived at the window barrier (loaders: hardware id), kind (1 computing, 2 loader, 0 none)}.
 * *nwords = words available; tools/phase_clocks.py makes the per-XCD histogram. */
int cvr_debug_phase_clocks(cvr_handle *h, unsigned long long *out, int64_t max_words, int64_t *nwords);

/* Calibration for the roofline: a 16-byte-per-lane copy kernel over `bytes` of device memory (read
 * `bytes`, write `bytes`); returns the mean read+write rate in GB/s over `iters` launches on `device`. */
int cvr_device_copy_bench(int device, int64_t bytes, int iters, double *gbs);

/* Copies the device-resident CVR64 image back for inspection (tests compare it bit for bit with the
 * CPU mirror).  Any pointer may be NULL.  Sizes: cols_vals = image_bytes of the stream part
 * (nchunks * S/4 * group_bytes), desc = 4 u32 per chunk, target = 64 u8 per chunk,
 * shared = 3 i64 per shared row {row, first chunk, last chunk}.  With column phases desc[k][1] counts the (row, phase)
 * segments of the chunk and the last column word of a segment carries the chunk's row of the segment above the column index. */
int cvr_export_image(cvr_handle *h, void *stream_image, uint32_t *desc, uint8_t *target, int64_t *shared);
/* The rest of an image with gang chunks (cvr_options.gang), for the same comparison: group_first_cols = nchunks * S/4 u32 -- the first column of
 * every group of every gang, gang b's groups from (b * waves_per_block) * S/4 on, zeros behind its last (all zeros when the image carries 16-bit
 * tags) --, desc2 = 2 u32 per chunk {groups of the gang that hold non-zeros (at its first chunk; 0 at the others), rows of the chunk}.
 * Either pointer may be NULL.  CVR_ERR_STATE for images without gang chunks. */
int cvr_export_gang(cvr_handle *h, uint32_t *group_first_cols, uint32_t *desc2);
/* host planner only (no device needed): chunk boundaries for a row_ptr; returns nchunks or <0.
 * out arrays (each may be NULL) need room for cvr_plan_bound(nrows, nnz, S) chunks. */
int64_t cvr_plan_bound(int64_t nrows, int64_t nnz, int32_t S);
int64_t cvr_plan_chunks(int64_t nrows, const int64_t *row_ptr, int32_t S, int64_t split_threshold,
                        int64_t *nz_begin /*[n+1]*/, int64_t *row_first, int64_t *nseg, int64_t *pad_cnt);

/* diagnostics (needs a device): plans row_ptr with the device planner (cvr_plan_dev.hip) and with the host planner and
 * compares the two plans field by field (CVR_OK = identical); seconds of both, chunk count. */
int cvr_plan_selfcheck(int device, int64_t nrows, const int64_t *row_ptr, int32_t S, int64_t split_threshold, int64_t max_rows,
                       double *host_seconds, double *device_seconds, int64_t *nchunks);
/* diagnostics (needs a device): the vector work of one cvr_power_iteration step on the caller's device arrays, so that the sharded form can be
 * checked on one GPU without a communicator.  x_dev: n values of T (float if is_f32, else double), in: x, out: T(double(y) * inv) with inv = 1 for
 * prev_dev == NULL, else inv(y.y) of the partial sums a call before left in its partial_dev.  partial_dev: 3 * 1024 doubles, out: this step's partial
 * sums (x.y, y.y, x.x; dense tree), sums[3] (host): their totals.  bounds == NULL: y_dev holds n values (the dense step).  bounds[nparts + 1]
 * (host; 0 .. n, not decreasing, 1 <= nparts <= 64, every shard <= max_rows): y_dev holds nparts * max_rows values, shard p's rows at
 * y_dev[p * max_rows ...] (the padded step), and dense_dev, where not NULL, receives the n rows in row order (the un-padding pass of the last
 * step).  Synchronises `stream`. */
int cvr_power_step_selfcheck(int device, int64_t n, int is_f32, void *x_dev, const void *y_dev, const double *prev_dev, double *partial_dev,
                             const int64_t *bounds, int nparts, int64_t max_rows, void *dense_dev, double *sums, void *stream);

/* ---- host side of the reference program ------------------------------------------------------ */
#define CVR_MM_REFCOMPAT 0   /* the reference loader's arrays bit for bit (quirks Q1-Q9)           */
#define CVR_MM_STRICT    1   /* Matrix-Market semantics: 0-based, fp64 values, no padding, 64-bit  */
typedef struct {
    int64_t  nrows, ncols, nnz;   /* of the arrays below, taken literally (see cvr_csr_view)      */
    int64_t  ref_numRows, ref_numCols, ref_nItems, ref_nItemsRaw;  /* header rows/cols, padded and */
                                                                   /* raw entry counts (refcompat) */
    int64_t *row_ptr;
    int32_t *col_idx;
    double  *vals;
} cvr_mm_matrix;
int  cvr_mm_read(const char *path, int mode, cvr_mm_matrix *out);   /* readMatrix, spmv.cpp:311-535 */
void cvr_mm_free(cvr_mm_matrix *m);
/* binary image of a parsed matrix (all fields of cvr_mm_matrix): skips the text parse on the next run */
int  cvr_mm_write_bin(const char *path, const cvr_mm_matrix *m);
int  cvr_mm_read_bin(const char *path, cvr_mm_matrix *out);
/* The same, keyed to the source: the identity of a file is its size, its modification time (ns) and a 64-bit FNV-1a hash of its
 * first and last MiB, together with the loader mode.  A keyed image is only read back under the key it was written with:
 * CVR_ERR_STATE says the source has changed since (or the image carries no key) and the caller parses the text again. */
typedef struct { int64_t size, mtime_ns; uint64_t hash; int32_t mode, reserved; } cvr_source_key;
int  cvr_source_key_of(const char *path, int mode, cvr_source_key *key);
int  cvr_mm_write_bin_keyed(const char *path, const cvr_mm_matrix *m, const cvr_source_key *key);
int  cvr_mm_read_bin_keyed(const char *path, const cvr_source_key *expect, cvr_mm_matrix *out);
/* readMatrix through the cache beside the file (<mtx>.ref.csrbin / <mtx>.strict.csrbin): the cache when its key is the file's,
 * else the text, after which the cache is rewritten; *cache_hit (may be NULL) says which */
int  cvr_mm_read_cached(const char *mtx_path, int mode, cvr_mm_matrix *out, int *cache_hit);
/* The converted CVR64 image of a handle on disk (after cvr_preprocess; single images, column panels, hub tables alike): a second run
 * on the same matrix loads it straight into device memory and skips analysis, planner and converter (the reference repeats its
 * pre_processing on every run, spmv.cpp:1857).  The file is keyed by the source file's identity (`key`; NULL = none), the options,
 * the device's CU / XCD counts, the format and library version; cvr_load_image returns CVR_ERR_STATE when any of them differs
 * (the caller then runs cvr_create + cvr_preprocess and saves again).  The loaded handle computes the same y, bit for bit.
 * opt: the options the image must have been built with (NULL = defaults; opt->device = where to load it; a file of A^T's handle loads only with
 * opt->transpose = 1, one of A's only with 0, else CVR_ERR_STATE).  *seconds: load time. */
int  cvr_save_image(cvr_handle *h, const char *path, const cvr_source_key *key);
int  cvr_load_image(cvr_handle **out, const char *path, const cvr_source_key *expect, const cvr_options *opt, double *seconds);
/* x[j] = 1.0 (mode 0; fill, spmv.cpp:556-563) or splitmix64(0xC0FFEE, j) -> [-1,1) (mode 1) */
void cvr_fill_x(double *x, int64_t n, int mode);
/* the reference's self-check loop, OpenMP over rows, j ascending (spmv.cpp:1843-1850) */
void cvr_csr_spmv_host(int64_t nrows, const int64_t *row_ptr, const int32_t *col_idx, const double *vals,
                       const double *x, double *y, int nthreads);
/* rows i in [0, nrows_checked) with (y[i]-yref[i])^2 > 1e-6 (spmv.cpp:1916-1929) */
int64_t cvr_verdict(const double *y, const double *yref, int64_t nrows_checked);

#ifdef __cplusplus
}
#endif
#endif
