/*
 * tsg.h -- C ABI of the MI355X-native TileSpGEMM (libtsg.so).
 *
 * Drop-in for the GPU path of for-the-juan/SpGEMM (a TileSpGEMM fork).  Plain C
 * types only: int / pointers / sizes, no torch or HIP types in the signatures
 * (a stream is passed as `void *` = hipStream_t).  Every function returns an int
 * status (TSG_OK = 0, negative on error) and never calls exit().
 *
 * Two layers:
 *  (1) Host-pointer functions with the reference's names and argument meaning
 *      (callee allocates outputs with malloc, caller owns them; free with
 *      tsg_matrix_destroy / tsg_csr_free).  Each runs the hand-written gfx950
 *      HIP kernels; host<->device copies happen inside, as in the reference.
 *  (2) Device-resident functions (tsg_dev_*) on a tsg_context: device pointers
 *      in and out, one explicit stream, outputs owned by the context.
 *
 * The library fails loudly (TSG_ERR_NO_DEVICE) when no HIP device is present:
 * there is no CPU fallback.
 */
#ifndef TSG_H
#define TSG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSG_OK 0
#define TSG_ERR_INVALID (-1)     /* bad argument / tile size / shape             */
#define TSG_ERR_HIP (-2)         /* a HIP runtime call failed                    */
#define TSG_ERR_OOM (-3)         /* device or host allocation failed             */
#define TSG_ERR_OVERFLOW (-4)    /* a count exceeds the int32 layout fields       */
#define TSG_ERR_NO_DEVICE (-5)   /* no HIP device visible                         */
#define TSG_ERR_UNSUPPORTED (-6) /* shape/tile size not built into this library   */
#define TSG_ERR_IO (-7)          /* Matrix-Market read failure                    */

/* Field-for-field the reference SMatrix (src/common.h:150-172), so a caller's
 * SMatrix* can be passed as tsg_smatrix* unchanged.  Tile index types are
 * uint16_t as in src/common.h:140-146. */
typedef struct tsg_smatrix {
    int m;
    int n;
    int nnz;
    int isSymmetric;
    double *value;
    int *columnindex;
    int *rowpointer;
    int tilem;
    int tilen;
    int *tile_ptr;
    int *tile_columnidx;
    int *tile_rowidx;
    int *tile_nnz;
    int numtile;
    double *tile_csr_Value;
    uint16_t *tile_csr_Col;
    uint16_t *tile_csr_Ptr;
    uint16_t *mask;
    int *csc_tile_ptr;
    int *csc_tile_rowidx;
} tsg_smatrix;

/* Per-call measurements (device timestamps from HIP events on the call's stream). */
typedef struct tsg_stats {
    double t_csr2tile_ms;  /* GPU csr2tile of A and B                          */
    double t_step1_ms;     /* tile-level symbolic (C tile structure)            */
    double t_step2_ms;     /* per-tile bitmask symbolic + nnz scan              */
    double t_step3_ms;     /* per-tile numeric                                  */
    double t_tile2csr_ms;  /* GPU tile2csr                                      */
    double t_malloc_ms;    /* host-side allocation + size read-back stalls      */
    double t_kern_ms;      /* steps 1-3 incl. allocation (reference's timer)     */
    double t_e2e_ms;       /* device CSR in -> device CSR out                   */
    long long nnzCub;      /* sum_{a in A} rowlen_B(col(a))                     */
    long long numtileA, numtileB, numblkC, nnzC;  /* numtileB = -1: not counted (B too wide
                                                      for the count units; CSR path only) */
    long long tile_products; /* tile-level intermediate products (step-1 work)  */
    double t_step3_kernel_ms;  /* the step-3 numeric kernel alone (dominant kernel) */
    long long path;            /* the CSR path that ran: TSG_PATH_TILES / _BAND / _ROWS */
} tsg_stats;

/* tsg_stats.path (the CSR-in -> CSR-out routing) */
#define TSG_PATH_TILES 0  /* staged tile pipeline: csr2tile structure, steps 1-3, tile2csr */
/* 1: retired (the fused element path of rounds 1-3; the row-merge path is faster on short rows too) */
#define TSG_PATH_BAND 2   /* banded rows: dense LDS window per row */
#define TSG_PATH_ROWS 3   /* row merge: rows binned by products, B runs merged in LDS */
#define TSG_PATH_NUMERIC 4 /* numeric-only run on a known C pattern (tsg_dev_numeric_run) */
#define TSG_PATH_MASKED 5  /* masked run: A*B on a mask's pattern only (tsg_dev_masked_run) */
#define TSG_PATH_SYMBOLIC 6 /* symbolic pass: C's pattern without values (tsg_dev_spgemm_symbolic) */
#define TSG_PATH_EWISE 7    /* element-wise union / intersection / difference of two CSRs (tsg_dev_ewise) */

/* ---------------- library / device ---------------- */
const char *tsg_version(void);
int tsg_device_count(int *count);
const char *tsg_status_string(int status);

/* ---------------- layer 1: reference-named host functions ---------------- */

/* Matrix-Market reader with mmio_allinone's exact CSR order
 * (src/mmio_highlevel.h:593-759): counting sort by row, in-row file order,
 * symmetric/hermitian mirrored in file order, pattern -> 1.0. */
int tsg_mmio_allinone(const char *filename, tsg_smatrix *A);

/* value[k] = k % 10 by CSR position (src/main.cu:111-112). */
void tsg_values_pos_mod10(tsg_smatrix *A);

/* Stable CSR->CSC transpose on the GPU (replaces matrix_transposition,
 * src/utils.h:161-198).  Writes B := A^T as a new malloc'd CSR. */
int tsg_transpose(const tsg_smatrix *A, tsg_smatrix *B);

/* sum_{a in A} rowlen_B(col(a)) on the GPU (src/main.cu:155-162). */
int tsg_nnzcub(const tsg_smatrix *A, const tsg_smatrix *B, unsigned long long *nnzCub);

/* Replaces csr2tile_row_major (src/csr2tile.h:205).  Fills the tile fields of A
 * (tile_ptr, tile_columnidx, tile_rowidx, tile_nnz, tile_csr_Ptr [numtile*tm],
 * tile_csr_Col = r*tn+c, tile_csr_Value, mask).  tile_rowidx[t] (numtile) is
 * the tile row of tile t of the row-major list: i for tile_ptr[i] <= t <
 * tile_ptr[i+1]. */
int tsg_csr2tile_row_major(tsg_smatrix *A, int tile_size_m, int tile_size_n);

/* Replaces csr2tile_col_major (src/csr2tile.h:279).  B tiles are tn x tm:
 * row-major structure (tile_ptr/tile_columnidx), CSC structure
 * (csc_tile_ptr/csc_tile_rowidx), payload in CSC tile order (tile_nnz,
 * tile_csr_Ptr [numtile*tn], tile_csr_Col = local col, tile_csr_Value, mask).
 * tile_rowidx (numtile) goes with the row-major structure as for A: the tile
 * row of tile t of tile_ptr / tile_columnidx.  (The reference allocates B's
 * tile_rowidx zero-filled and neither fills nor reads it, src/csr2tile.h:336-337;
 * csc_tile_rowidx is the field its SpGEMM steps use.) */
int tsg_csr2tile_col_major(tsg_smatrix *B, int tile_size_m, int tile_size_n);

/* Replaces tilespgemm (src/tilespgemm-cuda.h:2220-2235), same argument list.
 * blk_intersec_bitmask_A/B may be NULL (they are not needed by this
 * implementation; the reference builds them on the host, src/main.cu:194-232).
 * Fills C's tile fields (tile_ptr, tile_columnidx, tile_rowidx, tile_nnz
 * exclusive [numblkC+1], tile_csr_Ptr [numblkC*tm], tile_csr_Col,
 * tile_csr_Value, mask) plus m, n, tilem, tilen, numtile, nnz.  Structurally
 * empty C tiles (step-1 tiles whose element product is empty) are kept with
 * nnz 0, an all-zero Ptr and an all-zero mask, exactly the reference's C tile
 * list.  C's mask (numblkC * tm * tm/16 words, which the reference leaves on the
 * device) has the operands' layout: word c / 16 of row r, bit 15 - c % 16, set
 * for every structural nonzero; tile_rowidx as for A.
 * filename is only echoed in the printed lines (may be NULL). */
int tsg_tilespgemm(tsg_smatrix *A, tsg_smatrix *B, tsg_smatrix *C,
                   unsigned int *blk_intersec_bitmask_A, unsigned int *blk_intersec_bitmask_B,
                   int blk_intersec_bitmask_len, double densityA, double densityB,
                   unsigned long long nnzCub, unsigned long long *nnzC_computed,
                   double *compression_rate, double *time_tile, double *gflops_tile,
                   const char *filename, double *time_step1, double *time_step2,
                   double *time_step3, double *time_malloc, int tile_size_m, int tile_size_n);

/* Replaces tile2csr (src/tile2csr.h:72-140), called as tile2csr(C, tm, tm). */
int tsg_tile2csr(tsg_smatrix *C, int tile_size_m, int tile_size_n);

/* One shot CSR -> CSR: C = A * B, fp64, structural pattern (no zero dropping),
 * ascending columns.  Uploads A and B and runs tsg_dev_spgemm (below) -- the
 * routed device pipeline (row-merge, banded or staged tile path, whichever
 * its statistics pick; stats->path says which) -- then downloads C.  The same C
 * as csr2tile + steps 1-3 + tile2csr.  C->rowpointer/columnindex/value are
 * malloc'd. stats may be NULL. */
int tsg_spgemm_csr(const tsg_smatrix *A, const tsg_smatrix *B, tsg_smatrix *C,
                   int tile_size_m, int tile_size_n, tsg_stats *stats);

/* Numeric-only product on a known pattern: C->m, n, nnz, rowpointer and
 * columnindex given (strictly ascending columns per row, containing A*B's
 * structural pattern), C->value (malloc'd by the caller, nnz doubles)
 * overwritten with the values of A*B.  Uploads the operands, creates a numeric
 * plan (below), runs it once and destroys it.  TSG_ERR_INVALID for a malformed
 * pattern or one that lacks a column of A*B (C->value is then unspecified).
 * stats may be NULL. */
int tsg_spgemm_csr_numeric(const tsg_smatrix *A, const tsg_smatrix *B, tsg_smatrix *C, tsg_stats *stats);

/* Masked product C<M> = A*B on a structural mask: C->m, n, nnz, rowpointer and
 * columnindex are the mask (strictly ascending columns per row), C->value
 * (malloc'd by the caller, nnz doubles) is overwritten with the entries of A*B
 * at the mask's positions, 0.0 where no product reaches; products elsewhere
 * are dropped.  mode: TSG_MASKED_AUTO / _ROWS / _DOT (below).  Uploads the
 * operands, creates a masked plan, runs it once and destroys it.  stats may be
 * NULL. */
int tsg_spgemm_csr_masked(const tsg_smatrix *A, const tsg_smatrix *B, tsg_smatrix *C, int mode, tsg_stats *stats);

/* Symbolic product: C's structural pattern without values.  Uploads the
 * patterns of A and B (their value fields are not read and may be NULL), runs
 * tsg_dev_spgemm_symbolic (below) and downloads the result: C->m, n, nnz and
 * C->rowpointer (malloc'd, m + 1), and for TSG_SYMBOLIC_PATTERN C->columnindex
 * (malloc'd, strictly ascending per row); C->value is NULL (TSG_SYMBOLIC_COUNT:
 * C->columnindex too).  stats may be NULL. */
int tsg_spgemm_csr_symbolic(const tsg_smatrix *A, const tsg_smatrix *B, tsg_smatrix *C, int mode, tsg_stats *stats);

/* Masked symbolic product: the pattern of A*B restricted to the structural mask
 * (complement = 0) or to its complement (complement = 1).  Uploads the patterns
 * of A, B and Mask (no value field is read; all may be NULL), runs
 * tsg_dev_spgemm_symbolic_masked (below) and downloads the result as
 * tsg_spgemm_csr_symbolic does.  Mask->m == A->m, Mask->n == B->n, its columns
 * strictly ascending per row.  stats may be NULL. */
int tsg_spgemm_csr_symbolic_masked(const tsg_smatrix *A, const tsg_smatrix *B, const tsg_smatrix *Mask,
                                   int complement, int mode, tsg_smatrix *C, tsg_stats *stats);

/* ---- semirings of the numeric and masked plans ----
 * c(i,j) = (+) over the k with A(i,k) and B(k,j) both stored of A(i,k) (x)
 * B(k,j), for a semiring ((+), (x)) chosen per run (a plan holds patterns only:
 * one plan serves every semiring).
 *  - Entries are structural: a stored 0.0 takes part (in MIN_PLUS it is a
 *    zero-length edge), and no result is dropped, so C's pattern is the same
 *    for every semiring: tsg_dev_spgemm_symbolic's.
 *  - A pattern or mask entry no product reaches gets the (+)-identity: +inf for
 *    MIN_*, -inf for MAX_*, 0.0 for PLUS_* (also in a row whose A row is empty).
 *  - A column repeated in a B row is combined with (+) on the row-wise leg, as
 *    it is added by the arithmetic product.
 *  - NaN inputs and the sign of a zero result are unspecified for the min / max
 *    semirings.
 *  - For the five min / max semirings and PLUS_PAIR the result does not depend
 *    on the order of the sum: both legs of the masked plan and every class of
 *    the numeric plan are bit-reproducible, and agree with each other bit for
 *    bit.  (PLUS_TIMES: the dot leg only, as before.) */
#define TSG_SEMIRING_PLUS_TIMES 0  /* the arithmetic product: what every other call computes */
#define TSG_SEMIRING_MIN_PLUS   1  /* identity +inf */
#define TSG_SEMIRING_MAX_PLUS   2  /* identity -inf */
#define TSG_SEMIRING_MAX_TIMES  3  /* identity -inf */
#define TSG_SEMIRING_MAX_MIN    4  /* identity -inf */
#define TSG_SEMIRING_MIN_MAX    5  /* identity +inf */
#define TSG_SEMIRING_PLUS_PAIR  6  /* every product counts 1.0; a_val / b_val are not read and may be NULL; identity 0 */

/* *identity := the semiring's (+)-identity.  Host only (no device is touched);
 * TSG_ERR_INVALID for an unknown semiring or a NULL identity. */
int tsg_semiring_identity(int semiring, double *identity);
/* "plus_times", "min_plus", "max_plus", "max_times", "max_min", "min_max",
 * "plus_pair"; NULL for an unknown semiring. */
const char *tsg_semiring_name(int semiring);

/* One shot host CSR -> host CSR over a semiring: C = A (+).(x) B on A*B's full
 * structural pattern.  Uploads A and B, runs the symbolic pass, creates a
 * numeric plan on its pattern, runs it once with the semiring and destroys it,
 * downloads C.  C->rowpointer / columnindex / value are malloc'd like
 * tsg_spgemm_csr's.  PLUS_PAIR: A->value / B->value are not read and may be
 * NULL.  TSG_ERR_INVALID for an unknown semiring (nothing is launched).
 * stats (nullable): the numeric run's. */
int tsg_spgemm_csr_semiring(const tsg_smatrix *A, const tsg_smatrix *B, tsg_smatrix *C, int semiring,
                            tsg_stats *stats);
/* tsg_spgemm_csr_masked over a semiring: C->value[p] := the (+)-sum of the
 * products reaching mask entry p, the (+)-identity where none does.
 * TSG_SEMIRING_PLUS_TIMES is tsg_spgemm_csr_masked itself. */
int tsg_spgemm_csr_masked_semiring(const tsg_smatrix *A, const tsg_smatrix *B, tsg_smatrix *C, int mode, int semiring,
                                   tsg_stats *stats);
/* One shot host CSR -> host CSR with GraphBLAS mask semantics: C<Mask> (complement
 * = 0) or C<!Mask> (complement = 1) = A (+).(x) B, holding exactly the entries
 * that a product reaches and the mask admits.  Uploads A, B and the mask's
 * pattern (Mask->value is not read), runs the masked symbolic pass, creates a
 * masked plan (TSG_MASKED_AUTO) on its pattern, runs it once with the semiring,
 * destroys it and downloads C.  C->rowpointer / columnindex / value are malloc'd
 * like tsg_spgemm_csr's.  Every returned entry is reached by a product: none
 * holds a (+)-identity that was merely filled in.  PLUS_PAIR: A->value /
 * B->value are not read and may be NULL.  TSG_ERR_INVALID for an unknown
 * semiring or a complement outside {0, 1} (nothing is launched).  stats
 * (nullable): the masked run's. */
int tsg_spgemm_csr_masked_sparse(const tsg_smatrix *A, const tsg_smatrix *B, const tsg_smatrix *Mask, int complement,
                                 int semiring, tsg_smatrix *C, tsg_stats *stats);

/* ---- element-wise combination of two CSRs (tsg_dev_ewise, below) ---- */
#define TSG_EWISE_UNION      0  /* pattern A u B: op(alpha a, beta b) where both are stored, alpha a or beta b where one is */
#define TSG_EWISE_INTERSECT  1  /* pattern A n B: op(alpha a, beta b) */
#define TSG_EWISE_DIFFERENCE 2  /* pattern A \ B: alpha a; op, beta and B's values are not read */

#define TSG_BINOP_PLUS 0
#define TSG_BINOP_TIMES 1
#define TSG_BINOP_MIN 2
#define TSG_BINOP_MAX 3
#define TSG_BINOP_FIRST 4   /* alpha a */
#define TSG_BINOP_SECOND 5  /* beta b */

/* "plus", "times", "min", "max", "first", "second"; NULL for an unknown op. */
const char *tsg_binop_name(int op);

/* One shot host CSR -> host CSR: uploads A and B, runs tsg_dev_ewise (below;
 * its contract holds: A->m == B->m, A->n == B->n, strictly ascending columns
 * per row, A->value == NULL for a structural call), downloads C.  C->rowpointer
 * / columnindex / value are malloc'd like tsg_spgemm_csr's (columnindex and
 * value NULL for an empty C, value NULL for a structural call).  stats may be
 * NULL. */
int tsg_ewise_csr(const tsg_smatrix *A, const tsg_smatrix *B, int mode, int op, double alpha, double beta,
                  tsg_smatrix *C, tsg_stats *stats);

/* Frees every non-NULL pointer field and zeroes the struct (covers the
 * reference's matrix_destroy, src/csr2tile.h:509-518, and the CSR arrays). */
void tsg_matrix_destroy(tsg_smatrix *M);

/* ---------------- layer 2: device-resident API ---------------- */
typedef struct tsg_context tsg_context;

/* Device CSR: pointers are device memory. */
typedef struct tsg_dev_csr {
    int m, n, nnz;
    int *rowpointer;
    int *columnindex;
    double *value;
} tsg_dev_csr;

/* Device tiled matrix (the reference's tile fields, device memory).  For a
 * col-major (B) tiling, csc_* and tile_rm2csc are set. */
typedef struct tsg_dev_tiles {
    int m, n, nnz;
    int tile_m, tile_n;        /* rows / cols of one tile                     */
    int tilem, tilen, numtile;
    int *tile_ptr;
    int *tile_columnidx;
    int *tile_rowidx;
    int *tile_nnz;
    uint16_t *tile_csr_Ptr;
    uint16_t *tile_csr_Col;
    double *tile_csr_Value;
    uint16_t *mask;
    int *csc_tile_ptr;
    int *csc_tile_rowidx;
    int *tile_rm2csc;          /* row-major tile index -> CSC tile index      */
    uint16_t *rm_mask;         /* B only: tile masks in row-major tile order   */
    int *rm_rowstart;          /* B only: per row-major tile, tile_n+1 absolute
                                  row starts into the CSC-ordered payload      */
} tsg_dev_tiles;

/* A context owns a device, a caching device allocator and the outputs of the
 * tsg_dev_* calls made on it.  One stream per call; not thread-safe per context.
 *
 * Error contract of the tsg_dev_* calls: a call that returns an error has
 * drained its stream, has returned every block it took from the context's
 * allocator to the cache (temporaries and half-built outputs alike), and has
 * zeroed its output struct (*plan = NULL for a numeric plan).  Blocks of
 * earlier calls -- their outputs -- are untouched, and the context stays usable:
 * the same call can simply be made again.  A call that succeeds leaves only its
 * outputs allocated, and synchronises no more than it documents. */
int tsg_context_create(int device, tsg_context **ctx);
int tsg_context_destroy(tsg_context *ctx);
/* Returns every context-owned output/temporary block to the cache (numeric
 * plans keep their memory: it is not the cache's). */
int tsg_context_reset(tsg_context *ctx);

/* ---- diagnostics ----
 * The caching allocator's counters, and a one-shot allocation failure, so that
 * the error contract of the tsg_dev_* calls can be tested. */
typedef struct tsg_pool_stats {
    long long live_blocks;    /* blocks handed out and not yet returned to the cache */
    long long live_bytes;     /* their size classes' bytes                           */
    long long reserved_bytes; /* device memory held: live + cached                   */
    long long allocs;         /* pool allocations since the context was created      */
} tsg_pool_stats;
int tsg_context_pool_stats(tsg_context *ctx, tsg_pool_stats *out);
/* The nth pool allocation from now (0 = the next) returns TSG_ERR_OOM once,
 * without calling hipMalloc; nth < 0 clears a pending injection.  Returns 1
 * if an injection was still pending when this call was made (it had not
 * fired), else 0; TSG_ERR_INVALID for a NULL ctx.  A host-side counter in the allocator, nothing more. */
int tsg_context_fail_alloc(tsg_context *ctx, long long nth);

int tsg_dev_csr2tile_row_major(tsg_context *ctx, const tsg_dev_csr *A, int tile_size_m,
                               int tile_size_n, void *stream, tsg_dev_tiles *out);
int tsg_dev_csr2tile_col_major(tsg_context *ctx, const tsg_dev_csr *B, int tile_size_m,
                               int tile_size_n, void *stream, tsg_dev_tiles *out);
int tsg_dev_tilespgemm(tsg_context *ctx, const tsg_dev_tiles *A, const tsg_dev_tiles *B,
                       void *stream, tsg_dev_tiles *C, tsg_stats *stats);
int tsg_dev_tile2csr(tsg_context *ctx, const tsg_dev_tiles *C, void *stream, tsg_dev_csr *out);
int tsg_dev_transpose(tsg_context *ctx, const tsg_dev_csr *A, void *stream, tsg_dev_csr *out);
/* Full pipeline, device CSR in -> device CSR out (outputs owned by ctx). */
int tsg_dev_spgemm(tsg_context *ctx, const tsg_dev_csr *A, const tsg_dev_csr *B,
                   int tile_size_m, int tile_size_n, void *stream, tsg_dev_csr *C,
                   tsg_stats *stats);
/* Whether every row of M is strictly column-sorted (*sorted = 1, else 0): the
 * check tsg_dev_spgemm makes on B on every call (the row-merge and banded
 * routes need it), on its own. */
int tsg_dev_csr_rows_sorted(tsg_context *ctx, const tsg_dev_csr *M, void *stream, int *sorted);
/* tsg_dev_spgemm for a B whose rows the caller has found column-sorted
 * (tsg_dev_csr_rows_sorted returned 1 and B has not changed since; the
 * caller's contract -- an unsorted B passed here gives a wrong C): the
 * per-call check of B is skipped, so a sequence of row blocks of A against one
 * B checks B once.  b_checked_sorted = 0 is tsg_dev_spgemm itself. */
int tsg_dev_spgemm_sorted_b(tsg_context *ctx, const tsg_dev_csr *A, const tsg_dev_csr *B,
                            int b_checked_sorted, int tile_size_m, int tile_size_n, void *stream,
                            tsg_dev_csr *C, tsg_stats *stats);

/* ---- numeric-only SpGEMM on a known C pattern ----
 * For callers that multiply in a loop with fixed patterns and changing values
 * (AMG setup, time stepping, Newton loops): the plan holds everything that
 * depends on the patterns alone; a run computes c_val and nothing else -- no
 * symbolic work, no allocation, no host read-back, C written once. */
typedef struct tsg_numeric_plan tsg_numeric_plan;

typedef struct tsg_numeric_info {
    long long products;      /* sum over A entries of rowlen_B(col) */
    long long nnzC;          /* pattern entries */
    long long rows_class[4]; /* rows per class: packed / wave / workgroup / split */
    long long split_units;   /* work units of the split class */
    int b_rows_sorted;       /* what the plan found (1: every B row strictly column-sorted) */
} tsg_numeric_info;

/* Creates a plan for C = A*B on the three patterns.  The value fields of A, B
 * and Cpattern are ignored.  The pattern arrays are device memory the caller
 * keeps alive and unchanged for the plan's life.  C's pattern: strictly
 * ascending columns per row, containing the structural pattern of A*B (a
 * superset is allowed: entries no product reaches get 0.0).  B's rows need not
 * be sorted and may repeat a column.
 * All three patterns are validated on the device before anything indexes with
 * them: rowpointer[0] == 0, non-decreasing, rowpointer[m] == nnz; A's and B's
 * columns in [0, n); C's columns in [0, n) and strictly ascending per row;
 * A->n == B->m, C->m == A->m, C->n == B->n.  Any violation returns
 * TSG_ERR_INVALID and creates no plan (*plan = NULL).  Whether the pattern
 * really contains A*B is not checked here; a run finds out (below).
 * Synchronous; this is the one-off cost.
 * Ownership: the plan's device memory is its own, outside the context's cache:
 * it survives tsg_context_reset and every other tsg_dev_* call on the context.
 * tsg_context_destroy destroys every plan still alive on the context; a plan
 * must not be used or destroyed after its context. */
int tsg_dev_numeric_plan_create(tsg_context *ctx, const tsg_dev_csr *A, const tsg_dev_csr *B,
                                const tsg_dev_csr *Cpattern, void *stream,
                                tsg_numeric_plan **plan, tsg_numeric_info *info /*nullable*/);
/* c_val[0..nnzC) := values of A*B for a_val / b_val laid on the plan's patterns
 * (device pointers).  Synchronous on return, like tsg_dev_spgemm.  If a product's
 * column is missing from its C row's pattern (the pattern is not a superset of
 * A*B) nothing is written outside the row's own c_val range, the call returns
 * TSG_ERR_INVALID and c_val's contents are unspecified; the plan stays usable.
 * stats (nullable): t_e2e_ms, t_step3_kernel_ms (the numeric kernels), nnzCub
 * (= products), nnzC, path = TSG_PATH_NUMERIC; the rest 0 or -1. */
int tsg_dev_numeric_run(tsg_context *ctx, tsg_numeric_plan *plan, const double *a_val,
                        const double *b_val, double *c_val, void *stream, tsg_stats *stats /*nullable*/);
/* tsg_dev_numeric_run over a semiring (TSG_SEMIRING_*, above): c_val[p] := the
 * (+)-sum of the products reaching pattern entry p, the (+)-identity where none
 * does.  An unknown semiring returns TSG_ERR_INVALID before anything is
 * launched (c_val untouched).  A product on a column the pattern lacks returns
 * TSG_ERR_INVALID as above, for every semiring.  TSG_SEMIRING_PLUS_PAIR reads
 * neither a_val nor b_val (they may be NULL).  TSG_SEMIRING_PLUS_TIMES is
 * tsg_dev_numeric_run itself.  stats as there (path = TSG_PATH_NUMERIC). */
int tsg_dev_numeric_run_semiring(tsg_context *ctx, tsg_numeric_plan *plan, int semiring, const double *a_val,
                                 const double *b_val, double *c_val, void *stream, tsg_stats *stats /*nullable*/);
/* TSG_ERR_INVALID for a plan that is not alive on ctx (e.g. destroyed twice). */
int tsg_dev_numeric_plan_destroy(tsg_context *ctx, tsg_numeric_plan *plan);

/* ---- masked SpGEMM: C<M> = A*B computed on the mask's pattern only ----
 * For callers that want A*B at known positions (triangle counting L*L<L>,
 * k-truss, clustering coefficients): only the mask's nnz values are computed
 * and written; the full product is neither formed nor allocated.  The mask is
 * structural (a CSR pattern) and taken in the plain sense.  For a complemented
 * mask, or for C<M> with only the entries a product reaches, take the pattern
 * from tsg_dev_spgemm_symbolic_masked (below) and create the plan on it; to
 * accumulate a product into an existing C, combine the two with tsg_dev_ewise
 * (below).  Valued masks remain out of scope.  A plan has the numeric plan's life
 * cycle: patterns fixed at creation, values per run, device memory of its own
 * (it survives tsg_context_reset; tsg_context_destroy frees the plans still
 * alive).
 * Each row with mask entries runs on one of two legs.  Row-wise: the numeric
 * plan's kernels over the mask as the C pattern, every element product of the
 * row walked, those on a column the mask lacks dropped.  Dot: per mask entry
 * (i, j) the sorted intersection of A's row i with B^T's row j (B^T is built
 * at plan time).  The dot leg needs A's rows strictly ascending and B free of a
 * repeated (row, column); the row-wise leg takes unsorted and repeating B rows
 * as the numeric plan does.  The dot leg uses no atomics and a summation order
 * fixed by the plan: its values are bit-reproducible from run to run. */
#define TSG_MASKED_AUTO 0 /* per row: the dot leg when dot_eligible and D_i < P_i (D_i: the sum over the
                             row's mask entries of min(len A_i, len B^T_j); P_i: its element products) */
#define TSG_MASKED_ROWS 1 /* every row on the row-wise leg */
#define TSG_MASKED_DOT 2  /* every row with mask entries on the dot leg (TSG_ERR_INVALID unless dot_eligible) */

typedef struct tsg_masked_plan tsg_masked_plan;

typedef struct tsg_masked_info {
    long long products;      /* sum over A entries of rowlen_B(col): the full product's work */
    long long nnzM;          /* mask entries = values a run writes */
    long long rows_rowwise, rows_dot; /* rows per leg (rows without mask entries are in neither) */
    long long products_rowwise;       /* element products the row-wise leg walks */
    long long dot_work;               /* sum over the dot leg's entries of min(len A_i, len B^T_j) */
    long long dot_units;              /* work units of the dot leg */
    int a_rows_sorted, b_rows_sorted, b_no_repeats, dot_eligible; /* what the plan found (1 / 0) */
} tsg_masked_info;

/* Creates a plan for C<Mask> = A*B on the three patterns (value fields ignored;
 * device arrays the caller keeps alive and unchanged for the plan's life).
 * Validation is the numeric plan's, on the device before anything indexes with
 * the patterns: rowpointer[0] == 0, non-decreasing, rowpointer[m] == nnz;
 * columns in range; the mask's columns strictly ascending per row; A->n ==
 * B->m, Mask->m == A->m, Mask->n == B->n.  Any violation, an unknown mode, or
 * TSG_MASKED_DOT on operands that are not dot_eligible returns
 * TSG_ERR_INVALID and creates no plan (*plan = NULL).  Synchronous. */
int tsg_dev_masked_plan_create(tsg_context *ctx, const tsg_dev_csr *A, const tsg_dev_csr *B,
                               const tsg_dev_csr *Mask, int mode, void *stream,
                               tsg_masked_plan **plan, tsg_masked_info *info /*nullable*/);
/* c_val[p] := sum_k A(i,k) * B(k,j) for every mask entry p = (i, j), 0.0 where
 * no product reaches; nothing is written outside c_val[0, nnzM).  Synchronous on
 * return.  stats (nullable): path = TSG_PATH_MASKED, nnzCub (= products), nnzC
 * (= nnzM), t_e2e_ms, t_step3_kernel_ms (the gather and both legs' kernels);
 * the rest as in the numeric run. */
int tsg_dev_masked_run(tsg_context *ctx, tsg_masked_plan *plan, const double *a_val, const double *b_val,
                       double *c_val, void *stream, tsg_stats *stats /*nullable*/);
/* tsg_dev_masked_run over a semiring (TSG_SEMIRING_*, above): c_val[p] := the
 * (+)-sum over k of A(i,k) (x) B(k,j) for every mask entry p = (i, j), the
 * (+)-identity where no product reaches (a mask entry on an empty A row
 * included); products elsewhere are dropped.  An unknown semiring returns
 * TSG_ERR_INVALID before anything is launched (c_val untouched).
 * TSG_SEMIRING_PLUS_PAIR reads neither a_val nor b_val (they may be NULL) and
 * skips the gather of b_val into B^T's order.  TSG_SEMIRING_PLUS_TIMES is
 * tsg_dev_masked_run itself.  stats as there (path = TSG_PATH_MASKED). */
int tsg_dev_masked_run_semiring(tsg_context *ctx, tsg_masked_plan *plan, int semiring, const double *a_val,
                                const double *b_val, double *c_val, void *stream, tsg_stats *stats /*nullable*/);
/* TSG_ERR_INVALID for a plan that is not alive on ctx (e.g. destroyed twice). */
int tsg_dev_masked_plan_destroy(tsg_context *ctx, tsg_masked_plan *plan);

/* ---- symbolic SpGEMM: C's pattern and row counts without values ----
 * The first half of the symbolic / numeric split: the pattern that
 * tsg_dev_numeric_plan_create and tsg_dev_masked_plan_create start from, and
 * the exact nnz(C) before anything is computed.  Entry (i, j) is in C iff some
 * k has A(i,k) and B(k,j) stored (no zero is dropped): element for element the
 * rowpointer / columnindex of tsg_dev_spgemm for the same operands, columns
 * strictly ascending per row, value == NULL.  The value fields of A and B are
 * never read and may be NULL; their rows may be unsorted and may repeat a
 * column.  Count-first: a count per row, a scan, then every column written once
 * at its final place -- no values, no product-sized staging, no compaction.
 * A and B are validated on the device before anything indexes with them, as
 * the numeric plan validates them (rowpointer[0] == 0, non-decreasing,
 * rowpointer[m] == nnz, columns in [0, n), A->n == B->m): a violation or an
 * unknown mode returns TSG_ERR_INVALID.  nnz(C) > INT32_MAX returns
 * TSG_ERR_OVERFLOW in both modes with the output zeroed, but info->nnzC holds
 * the exact count.  Synchronous on return; the outputs are context-owned,
 * valid until tsg_context_reset.  TSG_SYMBOLIC_COUNT: Cpattern->columnindex is
 * NULL and nnz is set.  An empty C has columnindex NULL in both modes.
 * stats (nullable): path = TSG_PATH_SYMBOLIC, nnzCub (= products), nnzC,
 * t_e2e_ms, t_step3_kernel_ms (the count and fill kernels); the rest as in the
 * numeric run. */
#define TSG_SYMBOLIC_PATTERN 0  /* rowpointer and columnindex */
#define TSG_SYMBOLIC_COUNT   1  /* rowpointer only: the count phase and the scan */

typedef struct tsg_symbolic_info {
    long long products;      /* sum over A entries of rowlen_B(col) */
    long long nnzC;          /* exact, also when it does not fit int32 */
    long long rows_class[4]; /* rows per class: packed / set / window / hub; rows without products are in none */
    long long units;         /* work units of the classes that cut rows (window and hub) */
    int b_rows_sorted;       /* what the call found (1: every B row strictly column-sorted) */
} tsg_symbolic_info;

int tsg_dev_spgemm_symbolic(tsg_context *ctx, const tsg_dev_csr *A, const tsg_dev_csr *B,
                            int mode, void *stream, tsg_dev_csr *Cpattern,
                            tsg_symbolic_info *info /*nullable*/, tsg_stats *stats /*nullable*/);

/* ---- masked symbolic SpGEMM: the exact pattern of C<M> and C<!M> ----
 * tsg_dev_spgemm_symbolic under a structural mask: entry (i, j) is in C iff some
 * k has A(i,k) and B(k,j) stored AND ((i, j) is in Mask) != complement.
 * complement = 1 is the frontier step of BFS and its kin, N = F*A<!Visited>,
 * whose pattern is not known in advance; complement = 0 gives C<M> without the
 * mask entries no product reaches.  A masked plan created on the result drops
 * exactly the products the mask excludes, over any semiring.
 * The output is tsg_dev_spgemm_symbolic's: rowpointer, columns strictly
 * ascending per row, value == NULL, context-owned, count-first, nothing sized
 * by the products; the unmasked pattern is never formed.
 * Mask: values never read (value may be NULL); validated on the device with A
 * and B before anything indexes with it, as tsg_dev_masked_plan_create
 * validates its mask (row pointers, columns in [0, n) and strictly ascending
 * per row, Mask->m == A->m, Mask->n == B->n); a mask with nnz 0 may have
 * columnindex == NULL.  A violation, a complement outside {0, 1} or an unknown
 * mode returns TSG_ERR_INVALID.  A and B may have unsorted rows and repeated
 * columns.
 * info: products, rows_class and units are those of the unmasked product (the
 * rows are classed by their products, which still bound their lengths); nnzC
 * is the masked count, exact also on TSG_ERR_OVERFLOW, which is decided on it.
 * stats as for tsg_dev_spgemm_symbolic (path = TSG_PATH_SYMBOLIC). */
int tsg_dev_spgemm_symbolic_masked(tsg_context *ctx, const tsg_dev_csr *A, const tsg_dev_csr *B,
                                   const tsg_dev_csr *Mask, int complement /*0|1*/, int mode /*TSG_SYMBOLIC_**/,
                                   void *stream, tsg_dev_csr *Cpattern, tsg_symbolic_info *info /*nullable*/,
                                   tsg_stats *stats /*nullable*/);

/* ---- element-wise union, intersection and difference of two CSRs ----
 * What sits between two products of a graph algorithm: Visited u= N of a BFS
 * (structural union), D = min(D, D*A) of Bellman-Ford (union with MIN),
 * alpha A + beta B (union with PLUS), and with them the accumulation of a
 * product into an existing C.  C's pattern is A u B, A n B or A \ B (mode:
 * TSG_EWISE_*, above); an entry stored in both operands holds op(alpha a, beta b)
 * (op: TSG_BINOP_*), one stored in A alone alpha a, in B alone beta b.
 * Count-first like the symbolic pass: the entries stored in both operands are
 * counted per row (the columns alone are read), the counts scanned, then every
 * column and value written once at its final place -- no staging sized by the
 * operands, no compaction.
 *  - Shapes and order: A->m == B->m and A->n == B->n; both operands have
 *    strictly ascending columns per row (every output of this library has).
 *    Both are validated on the device before anything indexes with them:
 *    rowpointer[0] == 0, non-decreasing, rowpointer[m] == nnz, columns in
 *    [0, n) and strictly ascending per row.  A violation, an unknown mode or an
 *    unknown op returns TSG_ERR_INVALID with *C zeroed and nothing launched past
 *    the validation.  An operand with nnz == 0 may have columnindex == NULL.
 *  - Structural or valued: A->value == NULL makes the call structural:
 *    C->value == NULL and no value, op or scalar is read.  Otherwise C has
 *    values and B->value must be non-NULL -- except for TSG_EWISE_DIFFERENCE and
 *    for TSG_BINOP_FIRST under TSG_EWISE_INTERSECT, which never read B's values
 *    (B->value may be NULL).  Any other NULL value pointer (of an operand with
 *    entries) is TSG_ERR_INVALID.
 *  - Values: alpha a and beta b are each rounded once, then op is applied and
 *    rounded once; nothing is contracted into a fused multiply-add.  MIN and
 *    MAX are fmin / fmax; NaN inputs and the sign of a zero are unspecified, as
 *    for the semirings.  No atomic takes part: every result is bit-reproducible.
 *    Entries are structural: a stored 0.0 takes part and no result is dropped.
 *  - Output: rowpointer, columnindex strictly ascending per row, and value;
 *    context-owned, valid until tsg_context_reset, synchronous on return like
 *    tsg_dev_spgemm's C.  An empty C has columnindex and value NULL.
 *    nnz(C) > INT32_MAX returns TSG_ERR_OVERFLOW with C zeroed and info->nnzC
 *    exact (the counts are summed in 64 bits).
 * Rows are classed by L = len A_i + len B_i: packed (L <= 32, 16 lanes per
 * row), wave (L <= 512, a wave per row) and tile (the rest: the row's merge
 * cut into units of 2,048 merged entries, a workgroup each, so that one long
 * row spreads over the whole device).
 * The error contract of the tsg_dev_* calls holds.
 * stats (nullable): path = TSG_PATH_EWISE, nnzCub = nnzA + nnzB (the entries
 * merged), nnzC, t_e2e_ms, t_step3_kernel_ms (the count and fill kernels); the
 * rest as in the numeric run. */
typedef struct tsg_ewise_info {
    long long nnzA, nnzB;
    long long both;          /* entries stored in A and in B */
    long long nnzC;          /* exact, also when it does not fit int32 */
    long long rows_class[3]; /* rows per class: packed / wave / tile; rows with no entry in A or B are in none */
    long long units;         /* work units of the class that cuts rows (tile) */
} tsg_ewise_info;

int tsg_dev_ewise(tsg_context *ctx, const tsg_dev_csr *A, const tsg_dev_csr *B, int mode, int op,
                  double alpha, double beta, void *stream, tsg_dev_csr *C,
                  tsg_ewise_info *info /*nullable*/, tsg_stats *stats /*nullable*/);

/* Copies between host and device (stream-ordered, synchronous on return). */
int tsg_memcpy_h2d(tsg_context *ctx, void *dst, const void *src, size_t bytes, void *stream);
int tsg_memcpy_d2h(tsg_context *ctx, void *dst, const void *src, size_t bytes, void *stream);
int tsg_memcpy_d2d(tsg_context *ctx, void *dst, const void *src, size_t bytes, void *stream);
int tsg_dev_malloc(tsg_context *ctx, void **ptr, size_t bytes);
int tsg_dev_free(tsg_context *ctx, void *ptr);

#ifdef __cplusplus
}
#endif
#endif /* TSG_H */
