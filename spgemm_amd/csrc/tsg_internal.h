// tsg_internal.h -- host-side internals shared by the device code (the .hip
// files: each declaration below names the one that implements it, tsg_device.hip
// where none is named) and the C-ABI layer (tsg_api.cpp).  gfx950 / wave64 only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <map>
#include <unordered_map>
#include <vector>

#include "../../include/tsg.h"

namespace tsg {

#define TSG_HIP(call)                                                    \
    do {                                                                 \
        hipError_t _e = (call);                                          \
        if (_e != hipSuccess) {                                          \
            ::tsg::report_hip_error(_e, #call, __FILE__, __LINE__);      \
            return (_e == hipErrorOutOfMemory) ? TSG_ERR_OOM : TSG_ERR_HIP; \
        }                                                                \
    } while (0)

#define TSG_TRY(call)                   \
    do {                                \
        int _rc = (call);               \
        if (_rc != TSG_OK) return _rc;  \
    } while (0)

void report_hip_error(hipError_t e, const char *what, const char *file, int line);

// Wait for the stream's work: poll for up to ~1 ms (a blocking wait costs
// 20-50 us of wake-up on every mid-pipeline size read-back), then block.
int stream_wait(hipStream_t s);

// Caching device allocator: power-of-two size classes, blocks return to a free
// list and are reused by later allocations on the (single) call stream, so the
// steady-state pipeline performs no hipMalloc.
class DevicePool {
  public:
    ~DevicePool();
    int alloc(void **p, size_t bytes);
    void release(void *p);
    void release_all_live();  // returns every live block to the cache
    void trim();              // hipFree of the cached blocks
    size_t bytes_reserved() const { return reserved_; }
    // diagnostics (tsg_context_pool_stats / tsg_context_fail_alloc)
    tsg_pool_stats stats() const;
    void fail_alloc(long long nth) { fail_in_ = nth < 0 ? -1 : nth; }
    bool fail_pending() const { return fail_in_ >= 0; }

  private:
    std::multimap<size_t, void *> free_;
    std::unordered_map<void *, size_t> live_;
    size_t reserved_ = 0;
    long long allocs_ = 0;
    long long fail_in_ = -1;  // allocations left before the injected failure (-1: none)
};

// Run-time knobs of the environment, parsed once at the top of each C-ABI call
// (per call, not per process: tests switch them inside one process).
struct Knobs {
    int force_path = -1;             // TSG_PATH=tiles / band / rows: TSG_PATH_*, else -1 (routed)
    int step2_mode = -1;             // TSG_STEP2_MODE=elem (1) / tile (0), else -1 (by tile density)
    bool tiled_csr = true;           // TSG_TILED_CSR=0: tsg_tilespgemm keeps the tile-payload kernels
    bool rows_checked_scan = false;  // TSG_ROWS_CHECKED_SCAN=1 (tests): the checked scan whatever the size
    bool dr_per_row = false;         // TSG_DR_PER_ROW (tests): per-row chunks also below DR_GMAX rows
    long long sym_hub_bytes = 0;     // TSG_SYM_HUB_BYTES (tests): the symbolic hub bitmaps' byte budget (0: kSymHubBitmapBytes)
};

// The row-merge setup's device counters (RowsPlan::cls).  The entry kernels zero
// the block as 32 ints and the setup reads it back up to kReadBytes in one copy,
// so the layout is part of the kernels' contract.
struct RowsCounters {
    int ncls[8];                    // rows per class
    unsigned long long hprod;       // class-H rows' products
    unsigned long long pmax;        // the longest row's products
    unsigned long long products;    // all products
    unsigned long long hubprod;     // hub rows' products (past kRowsHubProducts)
    unsigned long long hk;          // class-H rows with more runs than the one-walk kernel takes
    int pad0[2];
    int dr_chunks, dr_rows;         // the dominant-run kernels' cursors: fill chunks, rows
    int pad1[2];
    unsigned long long hbig;        // class-H rows' products past the one-walk register share
    unsigned long long ow_cursor;   // the one-walk kernel's scratch cursor
    int pad2[4];
    static constexpr size_t kReadBytes = 26 * sizeof(int);  // the host's part: everything before ow_cursor
};
static_assert(sizeof(RowsCounters) == 32 * sizeof(int), "the entry kernels zero 32 ints");
static_assert(offsetof(RowsCounters, hprod) == 32 && offsetof(RowsCounters, dr_chunks) == 80 &&
                  offsetof(RowsCounters, hbig) == 96 && offsetof(RowsCounters, ow_cursor) == RowsCounters::kReadBytes,
              "RowsCounters: the layout the row-merge kernels were measured with");

// the band check's statistics (tsg_band.hip: one record per slot on the device, their total read back)
struct BandStats {
    int wide;             // rows whose window is wider than the kernel's span
    int wmax;             // the widest window
    unsigned long long products;  // element products (they bound nnz(C))
    unsigned long long wcols;     // window columns in all
};
static_assert(sizeof(BandStats) == 6 * sizeof(int), "BandStats: the check's copy and memset count six ints");

// the hub plan's device counters (tsg_rows.hip, k_rows_wplan)
struct HubCounters {
    unsigned long long wprod;    // windowed rows' products
    unsigned long long drprod;   // dominant-run rows' products
    unsigned long long ndr;      // dominant-run rows
    unsigned long long pad;
};

// the symbolic pass's device counters (tsg_symbolic.hip, k_sym_classify)
struct SymCounters {
    int nlist[8];                   // rows per launch list (kSymLists of them)
    unsigned long long products;    // all element products
    unsigned long long win_units;   // the window class's (row, window) units (host side: read from their scan)
    unsigned long long hub_units;   // the hub class's product chunks
    unsigned long long pad;
};

// The windowed fill lists' three sizes in one u64 (one atomic per wave instead
// of three): 21 bits each, so fewer than kFillListMax units.
constexpr int kFillListBits = 21, kFillListMax = 1 << kFillListBits;
struct FillSizes { int sort, heavy, mid; };  // the sort fill's units, the bitmap fill's past / within a workgroup's registers
__host__ __device__ inline unsigned long long fill_sizes_pack(int sort, int heavy, int mid) {
    return (unsigned long long)sort | ((unsigned long long)heavy << kFillListBits) |
           ((unsigned long long)mid << (2 * kFillListBits));
}
__host__ __device__ inline FillSizes fill_sizes_unpack(unsigned long long pk) {
    return FillSizes{(int)(pk & (kFillListMax - 1)), (int)((pk >> kFillListBits) & (kFillListMax - 1)),
                     (int)(pk >> (2 * kFillListBits))};
}

// Small results on their way to the host: one host-mapped block, one field per
// use, so no two stages share a slot.  The fields come back by stream-ordered
// copies, except those a kernel writes itself by a system-scope store.
struct HostSlots {
    int i32;                       // read_i32
    long long i64;                 // read_i64
    int b_unsorted;                // B's sortedness flag (written by kernels: dev_rows_sorted_*)
    int nnz_c;                     // nnz(C) of the rows and band paths (written by the fused row-pointer scan)
    long long scan_total, scan_extra;  // scan_exclusive_i32_total and the value read with it
    int tile_units;                // the tile pipeline: step 2's units,
    long long tile_entries;        //   its element split entries,
    int tile_nnz_c;                //   nnz(C) of its CSR output
    int ctiles_fail;               // dev_ctiles_from_csr: an entry outside the structure
    int ctiles_nnz;                //   and nnz(C) on its way to the device
    BandStats band;                // dev_band_check
    RowsCounters rows;             // dev_rows_setup_async (its first kReadBytes)
    HubCounters hub;               // rows_hub_plan: the counters,
    int hub_units, hub_chunks;     //   the unit and chunk lists' sizes,
    long long hub_nmat;            //   the chunk x window offset matrix's
    unsigned long long fill_sizes; // the windowed fill lists' sizes (fill_sizes_pack)
    SymCounters sym;               // dev_symbolic: the class counts and unit totals
    int ew_nlist[4];               // dev_ewise: the rows per launch list (kEwLists of them)
    int unsorted[3];               // the patterns' validation: one sortedness flag per pattern (written by kernels)
};

struct Context {
    int device = 0;
    DevicePool pool;
    HostSlots *slots = nullptr;   // host pinned, for size read-backs
    HostSlots *dslots = nullptr;  // its device view (kernels report small results there by system-scope stores)
    hipEvent_t ev[16];
    bool stage_ev = false;         // the stage events too (TSG_STAGE_EVENTS=1), not just the kernel bracket
    Knobs knobs;                   // the call's run-time knobs (read_knobs, tsg_api.cpp)
    bool ev_ready = false;
    int init(int dev);
    void destroy();
    template <class T> int get(T **p, size_t count) {
        void *v = nullptr;
        int rc = pool.alloc(&v, count * sizeof(T) + 16);
        *p = static_cast<T *>(v);
        return rc;
    }
    void put(void *p) { if (p) pool.release(p); }
};

// A host function's pool blocks: whatever it got (or adopted) and neither put
// back early nor kept returns to the pool when the scope ends, so an early
// return (TSG_TRY / TSG_HIP) leaks nothing.  The pool reuses blocks in stream
// order on the call's one stream, so a block may return while kernels that
// read it are still queued, exactly as with an early put().  No heap
// allocation: a fixed table, sized for the largest user (dev_spgemm16: three
// tilings of 13 arrays, C, the shares, a plan; dev_rows_run: ~40 arrays) and
// checked in get().
class PoolScope {
  public:
    static constexpr int kMaxBlocks = 96;
    explicit PoolScope(Context &cx) : cx_(cx) {}
    PoolScope(const PoolScope &) = delete;
    PoolScope &operator=(const PoolScope &) = delete;
    ~PoolScope() {
        for (int i = 0; i < n_; ++i) cx_.put(p_[i]);
    }
    template <class T> int get(T **p, size_t count) {
        *p = nullptr;
        if (n_ == kMaxBlocks) return TSG_ERR_INVALID;
        TSG_TRY(cx_.get(p, count));
        p_[n_++] = *p;
        return TSG_OK;
    }
    // a block another function kept for this one (a struct's member) becomes this scope's
    void adopt(void *p) {
        if (p && n_ < kMaxBlocks) p_[n_++] = p;
    }
    // returns the block now (null, or not this scope's: nothing)
    void put(void *p) {
        if (forget(p)) cx_.put(p);
    }
    // hands the block out of the scope: an output, or a member of a struct the caller owns
    template <class T> T *keep(T *p) {
        forget(p);
        return p;
    }

  private:
    bool forget(void *p) {
        for (int i = 0; i < n_; ++i)
            if (p && p_[i] == p) {
                p_[i] = p_[--n_];
                return true;
            }
        return false;
    }
    Context &cx_;
    void *p_[kMaxBlocks];
    int n_ = 0;
};

// ---- launchers (all stream-ordered, no sync; in tsg_device.hip unless a
// comment names tsg_band, tsg_rows, tsg_ctiles, tsg_tile_steps, tsg_numeric, tsg_masked, tsg_symbolic or tsg_ewise) ----
// Exclusive scan in place over n elements (a[n-1] ends up = sum of a[0..n-2]
// when the caller stored 0 there, i.e. the reference's "n+1 scan" idiom): the
// generic three stages.
int scan_exclusive_i32(Context &cx, int *a, long n, hipStream_t s);
int scan_exclusive_i64(Context &cx, long long *a, long n, hipStream_t s);
// exclusive scan (n+1 idiom) whose total is read back
int scan_exclusive_i32_total(Context &cx, int *a, long n, hipStream_t s, long long *total);
// The same scans in the two-launch fused form where scan_fuses(n)
// (tsg_dev_common.h), else generic.  Row pointers (n = m + 1): the fused form
// also stores nnz(C) into the host-mapped *hnnz_dev and fills cfirst (optional:
// the row-merge compaction's chunk table); *fused (optional) reports whether it
// ran -- the generic form does neither.
int dev_scan_i64(Context &cx, long long *a, long n, hipStream_t s);
int dev_scan_rows(Context &cx, int *rp, int m, int *cfirst, int *hnnz_dev, hipStream_t s, bool *fused = nullptr);
// the fused form's second launch alone, for a caller whose own kernel produced
// the tile sums (k_rows_entries_sum)
int scan_apply_fused_i64(long long *a, long n, const long long *part, hipStream_t s);
// per A entry its B row's [start, end) (nothing queued for an empty A)
int launch_entry_bounds(const tsg_dev_csr &A, const tsg_dev_csr &B, int2 *ebnd, hipStream_t s);
// Sort u64 keys ascending inside each segment [seg[i], seg[i+1]) in place.
int segmented_sort_u64(Context &cx, unsigned long long *keys, const int *seg, int nseg,
                       long total, hipStream_t s);

int launch_nnzcub(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B,
                  unsigned long long *d_out, hipStream_t s);
int dev_transpose(Context &cx, const tsg_dev_csr &A, tsg_dev_csr &out, hipStream_t s);
int dev_csr2tile_row_major(Context &cx, const tsg_dev_csr &A, int tm, int tn, tsg_dev_tiles &out,
                           hipStream_t s);
int dev_csr2tile_col_major(Context &cx, const tsg_dev_csr &B, int tm, int tn, tsg_dev_tiles &out,
                           hipStream_t s);
// csr_out != nullptr: step 3 also scatters C into CSR (tile2csr fused into its epilogue).
// Acsr/Bcsr (nullable; B's rows column-sorted): the CSR operands, enabling the
// element-streaming passes -- step 3's values always, step 2's masks when
// step2_elem.  A and B then only need their tile structure (tile_ptr,
// tile_columnidx) unless some step still reads the tile payloads.
int dev_tilespgemm(Context &cx, const tsg_dev_tiles &A, const tsg_dev_tiles &B, tsg_dev_tiles &C,
                   tsg_stats *st, hipStream_t s, hipEvent_t *ev_marks, tsg_dev_csr *csr_out,
                   const tsg_dev_csr *Acsr = nullptr, const tsg_dev_csr *Bcsr = nullptr,
                   bool step2_elem = false);
// step 1 alone: C tile structure (tile_ptr, tile_columnidx, numtile) of any tile size
int dev_step1(Context &cx, const tsg_dev_tiles &A, const tsg_dev_tiles &B, tsg_dev_tiles &C,
              long long *tile_products, hipStream_t s, const tsg_dev_csr *Ael = nullptr,
              const tsg_dev_csr *Bel = nullptr, int2 *ebnd = nullptr,
              long long **tbase_out = nullptr, long long *tslots_out = nullptr, bool fill_ebnd = false);
// the reference's tiled C payload (tile_nnz, Ptr, mask, Col, Value) laid onto
// step 1's 16 x 16 structure from a column-sorted CSR C (tsg_ctiles.hip)
int dev_ctiles_from_csr(Context &cx, const tsg_dev_csr &Cc, tsg_dev_tiles &C, hipStream_t s);
// steps 2 + 3 on the reference tiled layout at any tile size (tsg_tile_steps.hip):
// C holds step 1's structure at C.tile_m x C.tile_m; ev (optional) gets ev[1..3]
int dev_tile_steps23(Context &cx, const tsg_dev_tiles &A, const tsg_dev_tiles &B, tsg_dev_tiles &C, hipStream_t s,
                     hipEvent_t *ev);
// tile_ptr + tile_columnidx of a CSR's tiling (tr x tc tiles), no payload;
// tile_columnidx is left null when M.nnz < skip_emit_density * numtile
int dev_tile_structure(Context &cx, const tsg_dev_csr &M, int tr, int tc, tsg_dev_tiles &out, hipStream_t s,
                       double skip_emit_density = 0);
// row masks of a tiling (structure in t) straight from CSR, into a new zeroed array
int dev_tile_masks(Context &cx, const tsg_dev_csr &M, tsg_dev_tiles &t, uint16_t **mask_out, hipStream_t s);
// whether every CSR row is column-sorted (synchronous)
int dev_rows_sorted(Context &cx, const tsg_dev_csr &M, bool *sorted, hipStream_t s);
int dev_rows_sorted_async(Context &cx, const tsg_dev_csr &M, int *host_flag, hipStream_t s);
// the same check with its last step left to the caller: the per-workgroup shares
// (pool-owned part, nb of them) are summed either by dev_rows_sorted_finish or
// inside the row-merge setup's binning kernel (one launch fewer)
struct SortedShares {
    int *part = nullptr;
    int nb = 0;
    int *dflag = nullptr;  // device view of the host flag
};
int dev_rows_sorted_shares(Context &cx, const tsg_dev_csr &M, int *host_flag, SortedShares *sh, hipStream_t s);
int dev_rows_sorted_finish(Context &cx, const SortedShares &sh, hipStream_t s);
// the same for the B rows A references only (row-merge / band paths)
int dev_rows_sorted_shares_ref(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, int *host_flag,
                               SortedShares *sh, hipStream_t s);
int dev_tile2csr(Context &cx, const tsg_dev_tiles &C, tsg_dev_csr &out, hipStream_t s);
// banded path (tsg_band.hip): every C row's reachable columns within one
// window of <= 2,048 columns, the windows holding at least as many products as
// columns in all (FEM-like operands; force: any density).  BandWin holds the
// check's results for the product (caller-owned device arrays: win, width).
struct BandWin {
    int2 *win = nullptr;         // per row: first and last reachable column
    long long *width = nullptr;  // per row: window width (+1 slot), scanned into staging offsets
    long long products = 0;      // element products (nnzCub)
    long long wcols = 0;         // window columns in all (bounds nnz(C))
    int2 *ebnd = nullptr;        // per A entry: its B row's [start, end) (the statistics kernel's by-product)
};
// sh (optional): B's sortedness shares, summed by the check's last kernel (the caller releases them after it)
int dev_band_check(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, bool force, bool *ok, BandWin *bw,
                   hipStream_t s, SortedShares *sh = nullptr);
int dev_spgemm_band(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, const BandWin &bw, tsg_dev_csr &C,
                    tsg_stats *st, hipStream_t s, hipEvent_t *ev);
// row-merge path (tsg_rows.hip): CSR in -> CSR out, B's rows column-sorted;
// rows binned by element products, each row's B rows merged (or, for the
// longest rows, marked in an LDS column bitmap).  Two halves around the
// caller's one host round trip: the setup (entry table, classes, routing
// statistics), then the run.
struct RowsPlan {
    int2 *ebnd = nullptr;      // per A entry: its B row's [start, end)
    long long *E = nullptr;    // per A entry: prefix of the element products
    int4 *lists = nullptr;     // the classes' rows: (row, its first A entry, its A entries, -)
    long long *soff = nullptr; // per row: staging offset
    RowsCounters *cls = nullptr;  // class counts, statistics, cursors (device)
    int *rowpointer = nullptr; // C's row pointers (row counts until the scan)
    int ncls[8] = {};
    long long products = 0, hprod = 0, pmax = 0;  // all / class-H rows' products, the longest row's
    long long hubprod = 0;     // hub rows' products (past kRowsHubProducts)
    long long hk = 0;          // class-H rows with more runs than the one-walk kernel takes
    long long hbig = 0;        // class-H rows' products past the one-walk register share (their scratch)
};
// Class-H rows past kRowsHubProducts products are hub rows: one run holding all
// but 4,096 of them -> the dominant-run kernels (k_rows_dr_*); the other hub
// rows and the rows past the one-walk kernel's runs or column span -> the
// windowed kernels (k_rows_w*: (row, column window) units); the rest the
// one-walk bitmap kernel (k_rows_bitmap).
constexpr long long kRowsHubProducts = 65536;
// the row-merge path sizes C by the products (no read-back of nnz(C) before the
// compaction) while their 12 B each stay within this; past it C is sized exactly
// (peak device memory of the path: 12 B per product of staging + C + the A
// entry table)
constexpr long long kRowsProductSizedC = 8LL << 30;
// sh (optional): B's sortedness shares, summed by the binning kernel (the caller releases them after it)
int dev_rows_setup_async(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, RowsPlan &p, hipStream_t s,
                         SortedShares *sh = nullptr);
void dev_rows_setup_read(Context &cx, RowsPlan &p);  // after the stream synchronised
bool dev_rows_accept(const RowsPlan &p);

// The pool arrays of the structs that pass between host functions, listed once.
// A function keeps its result's arrays when it succeeds; the caller's scope
// adopts them (a temporary) or leaves them to the context (an output).
template <class F> void each_block(tsg_dev_csr &c, F f) { f(c.rowpointer), f(c.columnindex), f(c.value); }
template <class F> void each_block(tsg_dev_tiles &t, F f) {
    f(t.tile_ptr), f(t.tile_columnidx), f(t.tile_rowidx), f(t.tile_nnz), f(t.tile_csr_Ptr), f(t.tile_csr_Col),
        f(t.tile_csr_Value), f(t.mask), f(t.csc_tile_ptr), f(t.csc_tile_rowidx), f(t.tile_rm2csc), f(t.rm_mask),
        f(t.rm_rowstart);
}
template <class F> void each_block(SortedShares &sh, F f) { f(sh.part); }
template <class F> void each_block(BandWin &bw, F f) { f(bw.win), f(bw.width), f(bw.ebnd); }
template <class F> void each_block(RowsPlan &p, F f) {
    f(p.ebnd), f(p.E), f(p.lists), f(p.soff), f(p.cls), f(p.rowpointer);
}
template <class S> void keep_blocks(PoolScope &ws, S &st) {
    each_block(st, [&](void *p) { ws.keep(p); });
}
template <class S> void adopt_blocks(PoolScope &ws, S &st) {
    each_block(st, [&](void *p) { ws.adopt(p); });
}
template <class S> void put_blocks(PoolScope &ws, S &st) {  // returns them now and clears the struct
    each_block(st, [&](void *p) { ws.put(p); });
    st = S{};
}
// ev (optional): 1 set up | 4..5 the row kernels | 3 end
int dev_rows_run(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, const RowsPlan &p, tsg_dev_csr &C,
                 tsg_stats *st, hipStream_t s, hipEvent_t *ev);

// numeric-only product on a known C pattern (tsg_numeric.hip, DESIGN.md section
// 3.7).  Rows are classed at plan time by len_C (the row's pattern entries) and
// P (its element products); a row takes the first class both of whose caps it
// fits, else it is split:
//   0 packed     len_C <= 32    and P <= 512    16 lanes per row
//   1 wave       len_C <= 512   and P <= 8,192  one wave per row (6 KiB of LDS), or a
//                workgroup on a dense LDS window of the row's column span
//   2 workgroup  len_C <= 4,096 and P <= 65,536 one workgroup per row (48 KiB of
//                LDS: columns + fp64 sums at 12 B per entry, 3 workgroups per CU)
//   3 split      the rest, in units of at most kNumUnitProducts products
constexpr int kNumPackedLen = 32, kNumWaveLen = 512, kNumWgLen = 4096;
constexpr long long kNumPackedProducts = 512, kNumWaveProducts = 8192, kNumWgProducts = 65536;
constexpr int kNumUnitProducts = 4096;   // a split unit's products at most (16 per thread: the unit is one
                                         //   chain of searches in global memory, its length is the run's tail)
constexpr int kNumUnitEntries = 4096;    // and its A entries
// the launch lists: a class's rows.  The wave class's rows of at least
// kNumWindowProducts products whose columns span at most kNumWindow take the
// dense-window kernel, the others the search; the searched wave and workgroup
// rows of few pattern entries (most of them: the classes' lengths follow the
// operands' power law) take an instantiation with a quarter of the LDS, so
// that every wave slot of a CU is filled -- a row is a chain of dependent
// loads, and the rows in flight are what hides it
constexpr int kNumWindow = 2048;
constexpr long long kNumWindowProducts = 1024;
constexpr int kNumWaveSmallLen = 128, kNumWgSmallLen = 1024;
enum { kNumListPacked = 0, kNumListWaveSmall, kNumListWave, kNumListWaveWin, kNumListWgSmall, kNumListWg,
       kNumListSplit, kNumLists };
inline int numeric_row_class(long long len_c, long long products) {
    if (len_c <= kNumPackedLen && products <= kNumPackedProducts) return 0;
    if (len_c <= kNumWaveLen && products <= kNumWaveProducts) return 1;
    if (len_c <= kNumWgLen && products <= kNumWgProducts) return 2;
    return 3;
}
// one launch's workgroups at most where the grid is a unit count: a grid's threads
// (workgroups x 256) must stay below 2^32
constexpr int kMaxGridBlocks = 1 << 23;
struct NumericPlan {
    tsg_dev_csr A{}, B{}, C{};  // the caller's pattern arrays (values unused)
    void *block = nullptr;      // the plan's own hipMalloc block (not the pool's: survives a reset)
    size_t bytes = 0;
    int cnt[4] = {};            // rows per class (the info's counts)
    int *rows = nullptr;        // the launch lists, list l at loff[l], lcnt[l] rows, ascending; the last
                                //   (kNumLists) holds the rows with nothing to do
    int lcnt[kNumLists + 1] = {}, loff[kNumLists + 1] = {};
    int4 *units = nullptr;      // split units: (row, first A entry, A entries, B row offset or -1)
    int nunits = 0;
    int *miss = nullptr;        // device counter of products outside the pattern
    int *hmiss = nullptr;       // its pinned host copy (the run's one D2H copy)
    tsg_numeric_info info{};
};
// the plan's validation on its own (synchronous): shapes, row pointers, columns
// in range, Cp's columns strictly ascending per row; *b_sorted: whether B's are
int dev_numeric_validate(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, const tsg_dev_csr &Cp,
                         bool *b_sorted, hipStream_t s);
// the same for the operands alone (the symbolic pass: there is no C pattern yet)
int dev_operands_validate(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, bool *b_sorted, hipStream_t s);
// skip (optional, host, one byte per row): rows with a non-zero byte go to the
// never-launched list kNumLists whatever their class -- a run leaves their
// c_val alone (the masked plan's rows of the dot leg).  validated (optional):
// the caller ran dev_numeric_validate on these patterns and passes what it
// found for B; null: validated here.
int dev_numeric_plan_create(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, const tsg_dev_csr &Cp,
                            NumericPlan &p, hipStream_t s, const unsigned char *skip = nullptr,
                            const bool *validated = nullptr);
// semiring: a TSG_SEMIRING_* value (tsg_semiring.h has the traits the kernels
// are instantiated on); an unknown one returns TSG_ERR_INVALID with nothing queued
bool semiring_known(int semiring);
int semiring_identity(int semiring, double *identity);  // (host code: the traits' identity, no device touched)
int dev_numeric_run(Context &cx, NumericPlan &p, int semiring, const double *a_val, const double *b_val,
                    double *c_val, hipStream_t s, hipEvent_t *ev, int *missed);
void dev_numeric_plan_free(NumericPlan &p);

// masked product C<M> = A*B on the mask's pattern only (tsg_masked.hip,
// DESIGN.md section 3.8).  Each row with mask entries takes one of two legs:
//   row-wise  an internal NumericPlan over the mask as the C pattern (a product
//             whose column the mask lacks misses its lookup and is dropped)
//   dot       per mask entry (i, j) the intersection of A's row i with B^T's
//             row j; work units of (row, a range of its mask entries)
// A unit's work -- the sum over its entries of min(len A_i, len B^T_j) -- is at
// most kMskUnitWork (an entry heavier than that is a unit of its own) and it
// has at most kMskUnitEntries entries; A rows of at most kMskRowLds entries are
// copied to LDS.  AUTO sends a row to the dot leg when kMskDotCost * D_i < P_i
// (D_i: the row's dot work, P_i: its element products).
constexpr int kMskUnitWork = 4096, kMskUnitEntries = 256, kMskRowLds = 2048;
constexpr long long kMskDotCost = 1;
struct MaskedPlan {
    NumericPlan rows;            // the row-wise leg (the dot leg's rows and the rows without mask entries skipped)
    tsg_dev_csr A{}, B{}, M{};   // the caller's pattern arrays (values unused)
    void *block = nullptr;       // the plan's own hipMalloc block: B^T, the gathered values, the units
    size_t bytes = 0;
    int *bt_rp = nullptr, *bt_ci = nullptr, *bt_pos = nullptr;  // B^T: row pointers, columns (= B's rows,
                                                                 //   ascending), each entry's position in B
    double *bt_val = nullptr;    // b_val in B^T's order, gathered by every run
    int4 *units = nullptr;       // dot units: (row, first mask entry, entries, -)
    int nunits = 0;
    tsg_masked_info info{};
};
int dev_masked_plan_create(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, const tsg_dev_csr &M, int mode,
                           MaskedPlan &p, hipStream_t s);
// ev (optional): ev[6] before the first kernel, ev[5] after the last
int dev_masked_run(Context &cx, MaskedPlan &p, int semiring, const double *a_val, const double *b_val,
                   double *c_val, hipStream_t s, hipEvent_t *ev);
void dev_masked_plan_free(MaskedPlan &p);

// symbolic product (tsg_symbolic.hip): C's row pointers
// and, in TSG_SYMBOLIC_PATTERN mode, its columns, count-first: count per row,
// scan, then every column written once at its final place.  No values, no
// product-sized staging.  Rows are classed at call time by P, their element
// products (an upper bound of the row's length); rows without products are in
// no class:
//   0 packed  P <= kSymPackedProducts  16 lanes per row: the products' columns in a
//             32-int LDS slice, repeats dropped and survivors ranked by comparison
//   1 set     P <= kSymSetProducts     an LDS hash set of 2 P slots, sorted by the
//             fill: a wave per row up to kSymSetWaveProducts (4 KiB of LDS per
//             row), a workgroup per row past it (32 KiB)
//   2 window  P <= kSymWindowProducts  units of (row, window of kSymWindow columns):
//             a kSymWindow / 8-byte LDS bitmap per unit (16 KiB: 8 workgroups, every
//             wave slot of a CU), popcount = the unit's count, bit rank = position
//   3 hub     the rest: chunks of at most kSymHubUnitProducts products set bits in an
//             n-bit bitmap per row in global memory; the rows go in batches whose
//             bitmaps stay within kSymHubBitmapBytes (one row's, where that is larger)
constexpr long long kSymPackedProducts = 32, kSymSetWaveProducts = 512, kSymSetProducts = 4096,
                    kSymWindowProducts = 65536;
constexpr int kSymWindow = 131072;
constexpr int kSymHubUnitProducts = 4096;
constexpr long long kSymHubBitmapBytes = 64ll << 20;
constexpr long long kSymMaxWinUnits = 1ll << 30;  // (row, window) units at most: TSG_ERR_OVERFLOW past it
enum { kSymListPacked = 0, kSymListSetWave, kSymListSetWg, kSymListWindow, kSymListHub, kSymLists };
__host__ __device__ inline int symbolic_row_list(long long products) {  // -1: no products, nothing to launch
    return products <= 0                     ? -1
           : products <= kSymPackedProducts  ? kSymListPacked
           : products <= kSymSetWaveProducts ? kSymListSetWave
           : products <= kSymSetProducts     ? kSymListSetWg
           : products <= kSymWindowProducts  ? kSymListWindow
                                             : kSymListHub;
}
// Validates A and B as the numeric plan does, then runs the pass; synchronous.
// On TSG_ERR_OVERFLOW (nnz(C) past int32) info->nnzC still holds the exact
// count.  ev: [4]..[5] bracket the count kernels, [6]..[7] the fill kernels
// (recorded in both modes).
int dev_symbolic(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, int mode, tsg_dev_csr &C,
                 tsg_symbolic_info &info, hipStream_t s, hipEvent_t *ev);
// The masked pass: the pattern of A*B restricted to the
// structural mask M (comp = 0) or to its complement (comp = 1).  M is validated
// with A and B as the masked plan validates its mask; its values are not read.
// Classes, units and batches are dev_symbolic's (P still bounds a row's length);
// info: products, rows_class and units of the unmasked product, nnzC the masked
// count, on which TSG_ERR_OVERFLOW is decided.
int dev_symbolic_masked(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, const tsg_dev_csr &M, int comp,
                        int mode, tsg_dev_csr &C, tsg_symbolic_info &info, hipStream_t s, hipEvent_t *ev);

// element-wise union / intersection / difference of two CSRs (tsg_ewise.hip,
// DESIGN.md section 3.12), count-first: the entries stored in both operands
// counted per row or unit, a scan, then every column and value written once at
// its final place.  Rows are classed at call time by L = len A_i + len B_i;
// rows without an entry are in no class:
//   0 packed  L <= kEwisePackedLen  16 lanes per row, two entries a lane at most
//   1 wave    L <= kEwiseWaveLen    a wave per row, both rows staged in LDS
//   2 tile    the rest: the row's merge path cut into units of kEwiseTile merged
//             entries, a workgroup per unit (a cut beside a pair a == b is moved
//             past the pair's B half: a unit holds one entry more at most)
constexpr int kEwisePackedLen = 32, kEwiseWaveLen = 512, kEwiseTile = 2048;
enum { kEwListPacked = 0, kEwListWave, kEwListTile, kEwLists };
__host__ __device__ inline int ewise_row_list(long long len) {  // -1: no entry, nothing to launch
    return len <= 0 ? -1 : len <= kEwisePackedLen ? kEwListPacked : len <= kEwiseWaveLen ? kEwListWave : kEwListTile;
}
// row pointers, columns in [0, n) and strictly ascending rows of each pattern, on
// the device before anything indexes with them (tsg_numeric.hip: the plans'
// checks, for operands that are not a product's); synchronous
int dev_sorted_patterns_validate(Context &cx, const tsg_dev_csr *const *mats, int nmat, hipStream_t s);
bool ewise_mode_known(int mode);
bool binop_known(int op);
// whether the call reads B's values (a valued call: A.value non-null)
bool ewise_reads_b_values(int mode, int op);
// Validates both operands, then runs the pass; synchronous.  A.value null: the
// structural call.  On TSG_ERR_OVERFLOW (nnz(C) past int32) info.nnzC still
// holds the exact count.  ev: [4]..[5] bracket the count kernels, [6]..[7] the
// fill kernels.
int dev_ewise(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, int mode, int op, double alpha, double beta,
              tsg_dev_csr &C, tsg_ewise_info &info, hipStream_t s, hipEvent_t *ev);

// read a device int / long long synchronously through pinned memory
int read_i32(Context &cx, const int *d, int *h, hipStream_t s);
int read_i64(Context &cx, const long long *d, long long *h, hipStream_t s);

bool tile_size_supported(int tm, int tn);  // the SpGEMM steps (16x16)
bool tile_side_supported(int t);         // csr2tile / tile2csr sides: 16, 32, 48, 64

}  // namespace tsg
