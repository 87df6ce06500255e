// tsg_numeric.hip -- numeric-only SpGEMM on a known C pattern (gfx950, wave64).
//
// c_val := values of A*B laid onto a C pattern the caller already holds (from
// an earlier full product, or any superset of A*B's structure).  Nothing of the
// full routes' symbolic work runs: no staging, no scan, no compaction, no
// column writes, no host read-back.  One Gustavson pass per C row: for each A
// entry (k, a) and each B entry (j, b) of row k, j is searched in the C row's
// ascending column list and a*b is added there.
//
// The plan (built once per pattern triple) validates the three patterns, bins
// the rows by (len_C, products) into four classes (numeric_row_class,
// tsg_internal.h) and cuts the split class into units:
//   packed     16 lanes per row, 16 rows per workgroup   columns + sums in LDS
//   wave       one wave per row, 4 rows per workgroup     columns + sums in LDS;
//              FEM-like rows (many products, narrow column span): a workgroup
//              per row, sums in a dense LDS window, no search (k_num_row_win)
//   workgroup  one workgroup per row                      columns + sums in LDS
//   split      (row, chunk of A entries | piece of one B row) units of at most
//              kNumUnitProducts products: the C row's columns searched in global
//              memory, fp64 atomicAdd into the row's c_val segment, which a
//              kernel zeroes at the start of the run
// Every lookup is bounded by the row's own range -- a binary search over
// [rowpointer[i], rowpointer[i+1]) or its LDS copy, or a bitmap of the row's
// own column window -- so a product whose column the pattern lacks can only
// miss: it is counted, never stored.  B's rows need not be sorted and may
// repeat a column: all sums are atomic adds (LDS: ds_add_f64; global: the plain
// atomicAdd(double *), correct on fine-grained memory too -- c_val is the
// caller's, its kind unknown).  DESIGN.md section 3.7 has the measurements.
//
// The arithmetic is a semiring's (tsg_semiring.h): the
// run-time kernels are templated on its traits -- "a*b" above is mul, "added"
// the semiring's atomic (+), "zeroes" a fill with its identity -- and
// dev_numeric_run picks the instantiation; the plan knows nothing of it.
#include <algorithm>
#include <vector>

#include "tsg_dev_common.h"
#include "tsg_semiring.h"

namespace tsg {

// ---------------------------------------------------------------------------
// plan-time kernels
// ---------------------------------------------------------------------------
// rowpointer[0] == 0, non-decreasing, rowpointer[m] == nnz (reads rp[0..m] only)
__global__ __launch_bounds__(WG) void k_num_check_rp(const int *rp, int m, int nnz, int *bad) {
    int v = 0;
    for (long i = (long)blockIdx.x * WG + threadIdx.x; i <= m; i += (long)gridDim.x * WG) {
        const int r = rp[i];
        if (i == 0 && r != 0) v = 1;
        if (i == m && r != nnz) v = 1;
        if (i < m && rp[i + 1] < r) v = 1;
    }
    if (v) atomicOr(bad, 1);
}

// columnindex[0..nnz) in [0, n)
__global__ __launch_bounds__(WG) void k_num_check_cols(const int *ci, int nnz, int n, int *bad) {
    int v = 0;
    for (long p = (long)blockIdx.x * WG + threadIdx.x; p < nnz; p += (long)gridDim.x * WG)
        v |= (unsigned)ci[p] >= (unsigned)n;
    if (v) atomicOr(bad, 1);
}

// per row: its element products and its C row's column span (a wave per row;
// validated patterns only)
__global__ __launch_bounds__(WG) void k_num_rowstats(const int *rpA, const int *ciA, const int *rpB, const int *rpC,
                                                     const int *ciC, int m, long long *P, int *span) {
    for (long row = (long)blockIdx.x * WAVES + wave_id(); row < m; row += (long)gridDim.x * WAVES) {
        long long s = 0;
        const int e1 = rpA[row + 1];
        for (int e = rpA[row] + lane_id(); e < e1; e += 64) {
            const int k = ciA[e];
            s += rpB[k + 1] - rpB[k];
        }
        s = wave_sum(s);
        if (lane_id() == 0) {
            P[row] = s;
            const int c0 = rpC[row], c1 = rpC[row + 1];
            span[row] = c1 > c0 ? ciC[c1 - 1] - ciC[c0] + 1 : 0;
        }
    }
}

// ---------------------------------------------------------------------------
// run-time kernels
// ---------------------------------------------------------------------------
struct NumOps {
    const int *rpA, *ciA, *rpB, *ciB, *rpC, *ciC;
    const double *a_val, *b_val;
    double *c_val;
    int *miss;
};

constexpr int NUM_G = 16;  // lanes striding one B row in the strided walks

// A group of T threads (16: a packed row's lanes, 64: one wave, 256: the
// workgroup) walks the products of
// the A entries [e0, e1), T entries at a time: each thread loads one entry (its
// B row's start and length, its value) into LDS, a scan gives the entries'
// product offsets, then the threads take the batch's products round-robin and
// find each product's entry by a search over the offsets -- every lane busy
// whatever the B rows' lengths (one 1,495-entry B row among 3-entry ones is
// webbase's usual hub case).  A wave whose batch holds only B rows of at most
// NUM_STRIDE_MAX entries, 8 on average or more (FEM: cant's rows are 72-81
// entries against B rows as long) skips the search: its four 16-lane groups
// take the entries round-robin and stride their B rows.
// s_off: T + 1 ints, s_bs: T ints, s_a: T doubles (the group's own); red: the
// workgroup scan's WAVES ints (T == WG only).  The group's threads must all call.
constexpr int NUM_STRIDE_MAX = 128;
constexpr int NUM_ILP = 4;  // products per lane in flight in the searched walk

// owner_search with a trip count that depends on n alone (wave-uniform): no
// exec-mask bookkeeping, so NUM_ILP of them interleave in one basic block
__device__ __forceinline__ int owner_search_u(const int *off, int n, int it) {
    int base = 0, len = n;
    while (len > 1) {
        const int half = len >> 1;
        base = (off[base + half] <= it) ? base + half : base;
        len -= half;
    }
    return base;
}

// add(q, a, commit): the product of B entry q with the A value a; everything up
// to the sum itself runs for commit == false too (q is then some valid entry).
// A semiring that reads no values (SR::kValues false) loads no a_val: a is 1.0.
template <int T, class SR, class F>
__device__ __forceinline__ void for_products(const NumOps &o, int e0, int e1, int t, int *s_off, int *s_bs,
                                             double *s_a, int *red, F add) {
    for (int eb = e0; eb < e1; eb += T) {
        const int e = eb + t;
        int bs = 0, bl = 0;
        double a = 0.0;
        if (e < e1) {
            const int k = o.ciA[e];
            bs = o.rpB[k];
            bl = o.rpB[k + 1] - bs;
            a = sr_load<SR>(o.a_val, e);
        }
        const int nv = min(T, e1 - eb);
        int total, off;
        bool stride = false;
        if constexpr (T == 64) {
            const int inc = wave_incl_scan_dpp(bl);
            total = wave_last(inc);
            off = inc - bl;
            stride = wave_last(wave_incl_max(bl)) <= NUM_STRIDE_MAX && nv >= 64 / NUM_G && total >= 8 * nv;
        } else if constexpr (T == NUM_G) {  // a 16-lane group is one DPP row, wholly active or not at all
            int inc = bl;
            inc += dpp_mov<0x111, 0xf>(0, inc);  // row_shr:1
            inc += dpp_mov<0x112, 0xf>(0, inc);  // row_shr:2
            inc += dpp_mov<0x114, 0xf>(0, inc);  // row_shr:4
            inc += dpp_mov<0x118, 0xf>(0, inc);  // row_shr:8
            total = __shfl(inc, NUM_G - 1, NUM_G);
            off = inc - bl;
        } else {
            off = block_excl_scan(bl, &total, red);
        }
        s_off[t] = off;
        s_bs[t] = bs;
        if constexpr (SR::kValues) s_a[t] = a;
        if (t == T - 1) s_off[T] = total;
        if constexpr (T == WG) __syncthreads(); else wave_lds_sync();
        if (stride) {
            const int g = t / NUM_G, l = t % NUM_G;
            for (int x = g; x < nv; x += T / NUM_G) {
                const int b0 = s_bs[x], n = s_off[x + 1] - s_off[x];
                const double ax = sr_load<SR>(s_a, x);
                for (int q = l; q < n; q += NUM_G) add(b0 + q, ax, true);
            }
        } else {
            // (the latency chain of one product -- owner search, B loads, column
            // search -- is ~20 dependent LDS / L2 round trips: NUM_ILP independent
            // ones per lane fill it)
            for (int it0 = t; it0 < total; it0 += NUM_ILP * T) {
                int x[NUM_ILP], it[NUM_ILP];
#pragma unroll
                for (int u = 0; u < NUM_ILP; ++u) {
                    it[u] = min(it0 + u * T, total - 1);
                    x[u] = owner_search_u(s_off, nv, it[u]);
                }
#pragma unroll
                for (int u = 0; u < NUM_ILP; ++u)
                    add(s_bs[x[u]] + (it[u] - s_off[x[u]]), sr_load<SR>(s_a, x[u]), it0 + u * T < total);
            }
        }
        if constexpr (T == WG) __syncthreads(); else wave_lds_sync();
    }
}

// T threads per row (16: packed, 64: wave, 256: workgroup), CAP pattern entries
// at most (the class's len_C cap; the length is clamped to it, so LDS indices
// stay in range whatever the list holds).  The row's columns and its sums,
// started at the semiring's identity, sit in LDS; a product's column is found by
// a binary search there.
template <class SR, int T, int CAP>
__global__ __launch_bounds__(WG) void k_num_rows(const int *list, int nrows, NumOps o) {
    constexpr int SLOTS = WG / T, WALK = T;
    __shared__ int s_col[SLOTS][CAP];
    __shared__ double s_acc[SLOTS][CAP];
    __shared__ int s_off[SLOTS][WALK + 1], s_bs[SLOTS][WALK + 1], s_red[WAVES];
    __shared__ double s_a[SLOTS][WALK + 1];
    const int slot = threadIdx.x / T, t = threadIdx.x % T;
    const long li = (long)blockIdx.x * SLOTS + slot;
    const bool have = li < nrows;
    const int row = have ? list[li] : 0;
    int c0 = 0, len = 0, e0 = 0, e1 = 0;
    if (have) {
        c0 = o.rpC[row];
        len = min(o.rpC[row + 1] - c0, CAP);
        e0 = o.rpA[row];
        e1 = o.rpA[row + 1];
    }
    int *col = s_col[slot];
    double *acc = s_acc[slot];
    for (int q = t; q < len; q += T) {
        col[q] = o.ciC[c0 + q];
        acc[q] = SR::identity();
    }
    if constexpr (T == WG) __syncthreads(); else wave_lds_sync();
    int bad = 0;
    auto add = [&](int q, double a, bool commit) {
        const int j = o.ciB[q];
        const double x = SR::mul(a, sr_load<SR>(o.b_val, q));
        const int pos = lower_bound_u(col, 0, len, j);
        const bool hit = pos < len && col[pos] == j;
        if (commit) {
            if (hit) SR::atomic(&acc[pos], x);
            else bad = 1;
        }
    };
    for_products<T, SR>(o, e0, e1, t, s_off[slot], s_bs[slot], s_a[slot], s_red, add);
    if constexpr (T == WG) __syncthreads(); else wave_lds_sync();
    for (int q = t; q < len; q += T) o.c_val[c0 + q] = acc[q];
    if (bad) atomicAdd(o.miss, 1);
}

// Wave-class rows of at least kNumWindowProducts products whose columns span at
// most NUM_WIN (FEM-like rows: cant's hold ~4,400 products on ~280 columns
// within 1,095): no search.  The sums are a dense LDS window over [first column,
// last column], a bitmap of the window says which of its columns the pattern
// holds (a product on any other is a miss), and the pattern's entries are
// gathered from the window at the end.  A workgroup per row (16.3 KiB of LDS:
// 8 workgroups, every wave slot of the CU); each wave takes a contiguous share
// of the row's A entries -- loaded one per lane, then broadcast entry by entry
// -- and its 64 lanes take the entry's B row.
constexpr int NUM_WIN = kNumWindow;
template <class SR>
__global__ __launch_bounds__(WG) void k_num_row_win(const int *list, int nrows, NumOps o) {
    __shared__ double acc[NUM_WIN];
    __shared__ u32 bits[NUM_WIN / 32];
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const int row = list[xcd_item(blockIdx.x, nrows)];  // (neighbouring rows, whose B rows overlap, on one XCD's L2)
    const int c0 = o.rpC[row], len = o.rpC[row + 1] - c0;
    int cmin = 0, span = 0;
    if (len > 0) {
        cmin = o.ciC[c0];
        span = max(min(o.ciC[c0 + len - 1] - cmin + 1, NUM_WIN), 0);  // (clamped: LDS indices stay in range)
    }
    for (int q = tid; q < span; q += WG) acc[q] = SR::identity();
    for (int q = tid; q < (span + 31) / 32; q += WG) bits[q] = 0u;
    __syncthreads();
    for (int q = tid; q < len; q += WG) {
        const int d = o.ciC[c0 + q] - cmin;
        if ((unsigned)d < (unsigned)span) atomicOr(&bits[d >> 5], 1u << (d & 31));
    }
    __syncthreads();
    const int a0 = o.rpA[row], a1 = o.rpA[row + 1];
    const int per = (a1 - a0 + WAVES - 1) / WAVES;
    const int e0 = min(a1, a0 + wv * per), e1 = min(a1, a0 + (wv + 1) * per);
    // Lane l holds entries l and l + 64 of the current B row (rows of at most 128
    // entries).  While the next B row has the same length and, on every lane, the
    // same columns (one ballot) -- in FEM operands the dof rows of one node:
    // cant's rows 3u, 3u+1, 3u+2 -- its a*b is added in registers (a (x) b and (+)
    // of the semiring); only a change
    // of pattern sends the sums to the window: one ds_add_f64 per column per run
    // of equal B rows instead of one per product (the banded path's walk).
    constexpr int NONE = INT_MIN;  // (no column: col - cmin of valid columns is never this)
    int bad = 0, pc0 = NONE, pc1 = NONE, plen = -1;
    double px0 = 0.0, px1 = 0.0;
    auto put = [&](int d, double x) {
        if ((unsigned)d < (unsigned)span && (bits[d >> 5] >> (d & 31) & 1u)) SR::atomic(&acc[d], x);
        else bad = 1;
    };
    auto flush = [&]() {
        if (pc0 != NONE) put(pc0, px0);
        if (pc1 != NONE) put(pc1, px1);
    };
    for (int base = e0; base < e1; base += 64) {  // wave-uniform
        const int my = base + lane;
        int bs = 0, be = 0;
        double av = 0.0;
        if (my < e1) {
            const int k = o.ciA[my];
            bs = o.rpB[k];
            be = o.rpB[k + 1];
            av = sr_load<SR>(o.a_val, my);
        }
        const int nj = min(64, e1 - base);
        for (int j = 0; j < nj; ++j) {
            const int s = __builtin_amdgcn_readlane(bs, j), e = __builtin_amdgcn_readlane(be, j);
            const double a = __shfl(av, j, 64);
            const int n = e - s;
            if (n > 128) {  // a long B row: straight to the window
                flush();
                pc0 = pc1 = NONE;
                plen = -1;
                for (int q = s + lane; q < e; q += 64) put(o.ciB[q] - cmin, SR::mul(a, sr_load<SR>(o.b_val, q)));
                continue;
            }
            int d0 = NONE, d1 = NONE;
            double x0 = 0.0, x1 = 0.0;
            if (s + lane < e) {
                d0 = o.ciB[s + lane] - cmin;
                x0 = SR::mul(a, sr_load<SR>(o.b_val, s + lane));
            }
            if (s + 64 + lane < e) {
                d1 = o.ciB[s + 64 + lane] - cmin;
                x1 = SR::mul(a, sr_load<SR>(o.b_val, s + 64 + lane));
            }
            if (n == plen && __ballot(d0 != pc0 || d1 != pc1) == 0ull) {
                px0 = SR::add(px0, x0);
                px1 = SR::add(px1, x1);
            } else {
                flush();
                pc0 = d0;
                pc1 = d1;
                px0 = x0;
                px1 = x1;
                plen = n;
            }
        }
    }
    flush();
    __syncthreads();
    for (int q = tid; q < len; q += WG) {
        const int d = o.ciC[c0 + q] - cmin;
        o.c_val[c0 + q] = (unsigned)d < (unsigned)span ? acc[d] : SR::identity();
    }
    if (bad) atomicAdd(o.miss, 1);
}

// the split rows' c_val segments := the run's semiring's identity (a workgroup per row)
__global__ __launch_bounds__(WG) void k_num_fill(const int *list, int nrows, const int *rpC, double *c_val,
                                                 double identity) {
    const int row = list[blockIdx.x];
    const int c1 = rpC[row + 1];
    for (int q = rpC[row] + threadIdx.x; q < c1; q += WG) c_val[q] = identity;
}

// one split unit per workgroup: (row, first A entry, A entries, w); w >= 0: the
// one entry's B row from its w-th entry on, kNumUnitProducts entries at most;
// w < 0: the entries' whole B rows
template <class SR>
__global__ __launch_bounds__(WG) void k_num_split(const int4 *units, NumOps o) {
    __shared__ int s_off[WG + 1], s_bs[WG], s_red[WAVES];
    __shared__ double s_a[WG];
    const int4 u = units[blockIdx.x];
    const int c0 = o.rpC[u.x], c1 = o.rpC[u.x + 1];
    int bad = 0;
    auto add = [&](int q, double a, bool commit) {
        const int j = o.ciB[q];
        const double x = SR::mul(a, sr_load<SR>(o.b_val, q));
        const int pos = lower_bound_u(o.ciC, c0, c1, j);  // (c0, c1: the workgroup's own)
        const bool hit = pos < c1 && o.ciC[pos] == j;
        if (commit) {
            if (hit) SR::atomic(&o.c_val[pos], x);
            else bad = 1;
        }
    };
    if (u.w >= 0) {
        const int k = o.ciA[u.y];
        const double a = sr_load<SR>(o.a_val, u.y);
        const int b1 = o.rpB[k + 1], q0 = o.rpB[k] + u.w;
        const int q1 = b1 - q0 > kNumUnitProducts ? q0 + kNumUnitProducts : b1;
        for (int q = q0 + (int)threadIdx.x; q < q1; q += WG) add(q, a, true);
    } else {
        for_products<WG, SR>(o, u.y, u.y + u.z, (int)threadIdx.x, s_off, s_bs, s_a, s_red, add);
    }
    if (bad) atomicAdd(o.miss, 1);
}

// ---------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------
static bool shape_ok(const tsg_dev_csr &M) {
    return M.m >= 0 && M.n >= 0 && M.nnz >= 0 && M.rowpointer && (M.nnz == 0 || M.columnindex);
}

void dev_numeric_plan_free(NumericPlan &p) {
    if (p.block) (void)hipFree(p.block);
    if (p.hmiss) (void)hipHostFree(p.hmiss);
    p.block = nullptr;
    p.hmiss = nullptr;
}

// The device checks of up to three patterns, in two host round trips: every
// row pointer array first (before anything indexes with it), then the columns
// in range and the rows' order.  order[i]: kOrderAny (rows unchecked),
// kOrderStrict (strictly ascending or TSG_ERR_INVALID) or kOrderReport (whether
// they are goes to *reported).  The sortedness checks are queued with a flag
// each (HostSlots::unsorted), so one wait covers them and the column check.
enum { kOrderAny = 0, kOrderStrict, kOrderReport };
static int validate_mats(Context &cx, const tsg_dev_csr *const *mats, const int *order, int nmat, bool *reported,
                         hipStream_t s) {
    for (int i = 0; i < nmat; ++i)
        if (!shape_ok(*mats[i])) return TSG_ERR_INVALID;
    PoolScope ws(cx);  // (the temporaries: returned to the pool on every way out)
    int *bad = nullptr;
    TSG_TRY(ws.get(&bad, 4));
    int hbad[2] = {0, 0};
    TSG_HIP(hipMemsetAsync(bad, 0, 4 * sizeof(int), s));
    // 1. row pointers
    for (int i = 0; i < nmat; ++i) {
        const tsg_dev_csr *M = mats[i];
        k_num_check_rp<<<grid_for((long)M->m + 1, WG, 2048), WG, 0, s>>>(M->rowpointer, M->m, M->nnz, bad);
    }
    TSG_HIP(hipGetLastError());
    TSG_HIP(hipMemcpyAsync(hbad, bad, sizeof(int), hipMemcpyDeviceToHost, s));
    TSG_TRY(stream_wait(s));
    if (hbad[0]) return TSG_ERR_INVALID;
    // 2. columns in range; the rows' order where it is asked for
    for (int i = 0; i < nmat; ++i) {
        const tsg_dev_csr *M = mats[i];
        if (M->nnz) k_num_check_cols<<<grid_for(M->nnz, WG, 2048), WG, 0, s>>>(M->columnindex, M->nnz, M->n, bad + 1);
        TSG_HIP(hipGetLastError());
        if (order[i] != kOrderAny) TSG_TRY(dev_rows_sorted_async(cx, *M, &cx.slots->unsorted[i], s));
    }
    TSG_HIP(hipMemcpyAsync(hbad + 1, bad + 1, sizeof(int), hipMemcpyDeviceToHost, s));
    TSG_TRY(stream_wait(s));
    if (hbad[1]) return TSG_ERR_INVALID;
    for (int i = 0; i < nmat; ++i) {
        const bool sorted = order[i] == kOrderAny || cx.slots->unsorted[i] == 0;
        if (order[i] == kOrderStrict && !sorted) return TSG_ERR_INVALID;
        if (order[i] == kOrderReport) *reported = sorted;
    }
    return TSG_OK;
}

// the validation of A and B, and of a C pattern where there is one (Cp null: the
// symbolic pass, which has none yet): C's rows strictly ascending, whether B's are
static int validate_patterns(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, const tsg_dev_csr *Cp,
                             bool *b_sorted, hipStream_t s) {
    if (A.n != B.m || (Cp && (Cp->m != A.m || Cp->n != B.n))) return TSG_ERR_INVALID;
    const tsg_dev_csr *mats[3] = {&A, &B, Cp};
    const int order[3] = {kOrderAny, kOrderReport, kOrderStrict};
    return validate_mats(cx, mats, order, Cp ? 3 : 2, b_sorted, s);
}

int dev_numeric_validate(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, const tsg_dev_csr &Cp,
                         bool *b_sorted, hipStream_t s) {
    return validate_patterns(cx, A, B, &Cp, b_sorted, s);
}

int dev_operands_validate(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, bool *b_sorted, hipStream_t s) {
    return validate_patterns(cx, A, B, nullptr, b_sorted, s);
}

// the same checks for patterns that are not a product's (the element-wise pass's
// operands, three at most): every one's rows strictly ascending
int dev_sorted_patterns_validate(Context &cx, const tsg_dev_csr *const *mats, int nmat, hipStream_t s) {
    if (nmat > 3) return TSG_ERR_INVALID;
    const int order[3] = {kOrderStrict, kOrderStrict, kOrderStrict};
    return validate_mats(cx, mats, order, nmat, nullptr, s);
}

// Synchronous (the one-off cost): validation, then the binning on the host from
// the per-row products the device counted.  Temporaries come from the pool and
// go back to it; what the plan keeps is one hipMalloc block of its own.
int dev_numeric_plan_create(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, const tsg_dev_csr &Cp,
                            NumericPlan &p, hipStream_t s, const unsigned char *skip, const bool *validated) {
    p = NumericPlan{};
    bool bsorted = false;
    if (validated) bsorted = *validated;
    else TSG_TRY(dev_numeric_validate(cx, A, B, Cp, &bsorted, s));
    const int m = A.m;
    PoolScope ws(cx);  // (the temporaries: returned to the pool on every way out)
    int *span = nullptr;
    long long *P = nullptr;
    // 3. products per row, classes, lists, units
    std::vector<long long> hP((size_t)m);
    std::vector<int> rpC((size_t)m + 1), hspan((size_t)m);
    if (m) {
        TSG_TRY(ws.get(&P, (size_t)m));
        TSG_TRY(ws.get(&span, (size_t)m));
        k_num_rowstats<<<grid_for(m, WAVES, 4096), WG, 0, s>>>(A.rowpointer, A.columnindex, B.rowpointer,
                                                              Cp.rowpointer, Cp.columnindex, m, P, span);
        TSG_HIP(hipGetLastError());
        TSG_HIP(hipMemcpyAsync(hP.data(), P, (size_t)m * sizeof(long long), hipMemcpyDeviceToHost, s));
        TSG_HIP(hipMemcpyAsync(hspan.data(), span, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    TSG_HIP(hipMemcpyAsync(rpC.data(), Cp.rowpointer, ((size_t)m + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
    TSG_TRY(stream_wait(s));
    // launch lists: packed | wave, searched | wave, windowed | workgroup | split |
    // rows with neither pattern entries nor products (packed by class, never launched)
    std::vector<unsigned char> lst((size_t)m);
    long long products = 0;
    for (int c = 0; c < 4; ++c) p.cnt[c] = 0;
    for (int l = 0; l < kNumLists + 1; ++l) p.lcnt[l] = 0;
    for (int i = 0; i < m; ++i) {
        const int len_c = rpC[i + 1] - rpC[i];
        const int c = numeric_row_class(len_c, hP[i]);
        ++p.cnt[c];
        products += hP[i];
        int l = c == 0   ? kNumListPacked
                : c == 1 ? (len_c <= kNumWaveSmallLen ? kNumListWaveSmall : kNumListWave)
                : c == 2 ? (len_c <= kNumWgSmallLen ? kNumListWgSmall : kNumListWg)
                         : kNumListSplit;
        if (c == 1 && len_c > 0 && hspan[i] <= kNumWindow && hP[i] >= kNumWindowProducts) l = kNumListWaveWin;
        if (c == 0 && len_c == 0 && hP[i] == 0) l = kNumLists;
        if (skip && skip[i]) l = kNumLists;  // (another leg's row: counted in its class, never launched)
        lst[i] = (unsigned char)l;
        ++p.lcnt[l];
    }
    p.loff[0] = 0;
    for (int l = 1; l < kNumLists + 1; ++l) p.loff[l] = p.loff[l - 1] + p.lcnt[l - 1];
    std::vector<int> rows((size_t)m);
    {
        int fill[kNumLists + 1];
        for (int l = 0; l < kNumLists + 1; ++l) fill[l] = p.loff[l];
        for (int i = 0; i < m; ++i) rows[fill[lst[i]]++] = i;
    }
    const int nsplit = p.lcnt[kNumListSplit], osplit = p.loff[kNumListSplit];
    std::vector<int4> units;
    if (nsplit) {  // the split rows' A entries against B's row lengths
        std::vector<int> rpA((size_t)m + 1), rpB((size_t)B.m + 1), ciA((size_t)A.nnz);
        TSG_HIP(hipMemcpyAsync(rpA.data(), A.rowpointer, rpA.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        TSG_HIP(hipMemcpyAsync(rpB.data(), B.rowpointer, rpB.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        if (A.nnz)
            TSG_HIP(hipMemcpyAsync(ciA.data(), A.columnindex, ciA.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        TSG_TRY(stream_wait(s));
        for (int r = 0; r < nsplit; ++r) {
            const int i = rows[osplit + r];
            int e0 = rpA[i], ne = 0;
            long long cur = 0;
            for (int e = rpA[i]; e < rpA[i + 1]; ++e) {
                const int bl = rpB[ciA[e] + 1] - rpB[ciA[e]];
                if (bl > kNumUnitProducts || cur + bl > kNumUnitProducts || ne == kNumUnitEntries) {
                    if (ne) units.push_back(make_int4(i, e0, ne, -1));
                    e0 = e;
                    ne = 0;
                    cur = 0;
                }
                if (bl > kNumUnitProducts) {  // one long B row: pieces of it
                    for (int w = 0; w < bl; w += kNumUnitProducts) units.push_back(make_int4(i, e, 1, w));
                    e0 = e + 1;
                } else {
                    ++ne;
                    cur += bl;
                }
            }
            if (ne) units.push_back(make_int4(i, e0, ne, -1));
        }
    }
    if (units.size() > (size_t)INT_MAX) return TSG_ERR_OVERFLOW;
    // 4. the plan's own block: class lists | units | miss counter
    const size_t b_rows = (((size_t)m * sizeof(int)) + 255) & ~(size_t)255;
    const size_t b_units = ((units.size() * sizeof(int4)) + 255) & ~(size_t)255;
    p.bytes = b_rows + b_units + 256;
    {
        const hipError_t e = hipMalloc(&p.block, p.bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p.block = nullptr;
            return TSG_ERR_OOM;
        }
    }
    p.rows = (int *)p.block;
    p.units = (int4 *)((char *)p.block + b_rows);
    p.miss = (int *)((char *)p.block + b_rows + b_units);
    p.nunits = (int)units.size();
    int rc = TSG_OK;
    if (hipHostMalloc((void **)&p.hmiss, 64, hipHostMallocDefault) != hipSuccess) rc = TSG_ERR_OOM;
    if (rc == TSG_OK && m &&
        hipMemcpyAsync(p.rows, rows.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess)
        rc = TSG_ERR_HIP;
    if (rc == TSG_OK && p.nunits &&
        hipMemcpyAsync(p.units, units.data(), units.size() * sizeof(int4), hipMemcpyHostToDevice, s) != hipSuccess)
        rc = TSG_ERR_HIP;
    if (rc == TSG_OK) rc = stream_wait(s);
    if (rc != TSG_OK) {
        (void)hipGetLastError();
        dev_numeric_plan_free(p);
        return rc;
    }
    p.A = A;
    p.B = B;
    p.C = Cp;
    p.A.value = p.B.value = p.C.value = nullptr;
    p.info.products = products;
    p.info.nnzC = Cp.nnz;
    for (int c = 0; c < 4; ++c) p.info.rows_class[c] = p.cnt[c];
    p.info.split_units = p.nunits;
    p.info.b_rows_sorted = bsorted ? 1 : 0;
    return TSG_OK;
}

// the run's launches for one semiring (dev_numeric_run's order)
template <class SR> static void numeric_launch(const NumericPlan &p, const NumOps &o, hipStream_t s) {
    const auto list = [&](int l) { return p.rows + p.loff[l]; };
    const auto n = [&](int l) { return p.lcnt[l]; };
    // (the long rows first: their tails overlap the short rows' kernels)
    if (n(kNumListSplit))
        k_num_fill<<<n(kNumListSplit), WG, 0, s>>>(list(kNumListSplit), n(kNumListSplit), p.C.rowpointer, o.c_val,
                                                   SR::identity());
    // (a grid holds fewer than 2^32 threads: past kMaxGridBlocks units -- a LiveJournal-sized pattern's
    // 3 * 10^7 -- the units go in several launches)
    for (int u0 = 0; u0 < p.nunits; u0 += kMaxGridBlocks)
        k_num_split<SR><<<std::min(p.nunits - u0, kMaxGridBlocks), WG, 0, s>>>(p.units + u0, o);
    if (n(kNumListWg)) k_num_rows<SR, WG, kNumWgLen><<<n(kNumListWg), WG, 0, s>>>(list(kNumListWg), n(kNumListWg), o);
    if (n(kNumListWgSmall))
        k_num_rows<SR, WG, kNumWgSmallLen><<<n(kNumListWgSmall), WG, 0, s>>>(list(kNumListWgSmall), n(kNumListWgSmall), o);
    if (n(kNumListWaveSmall))
        k_num_rows<SR, 64, kNumWaveSmallLen><<<(n(kNumListWaveSmall) + 3) / 4, WG, 0, s>>>(list(kNumListWaveSmall), n(kNumListWaveSmall), o);
    if (n(kNumListWave))
        k_num_rows<SR, 64, kNumWaveLen><<<(n(kNumListWave) + 3) / 4, WG, 0, s>>>(list(kNumListWave), n(kNumListWave), o);
    if (n(kNumListWaveWin))
        k_num_row_win<SR><<<n(kNumListWaveWin), WG, 0, s>>>(list(kNumListWaveWin), n(kNumListWaveWin), o);
    if (n(kNumListPacked))
        k_num_rows<SR, 16, kNumPackedLen><<<(n(kNumListPacked) + 15) / 16, WG, 0, s>>>(list(kNumListPacked), n(kNumListPacked), o);
}

int semiring_identity(int semiring, double *identity) {
    return semiring_dispatch(semiring, [&](auto sr) {
        *identity = decltype(sr)::identity();
        return TSG_OK;
    });
}

bool semiring_known(int semiring) {
    double id;
    return semiring_identity(semiring, &id) == TSG_OK;
}

// Queued on s and waited for: no allocation, no read-back before the final
// wait, every geometry from the plan.  ev (optional): ev[4]..ev[5] bracket the
// numeric kernels.  *missed: products whose column the pattern lacks.  An
// unknown semiring: TSG_ERR_INVALID, nothing queued.
int dev_numeric_run(Context &cx, NumericPlan &p, int semiring, const double *a_val, const double *b_val,
                    double *c_val, hipStream_t s, hipEvent_t *ev, int *missed) {
    (void)cx;
    if (!semiring_known(semiring)) return TSG_ERR_INVALID;
    const NumOps o{p.A.rowpointer, p.A.columnindex, p.B.rowpointer, p.B.columnindex, p.C.rowpointer,
                   p.C.columnindex, a_val, b_val, c_val, p.miss};
    TSG_HIP(hipMemsetAsync(p.miss, 0, sizeof(int), s));
    if (ev) TSG_HIP(hipEventRecord(ev[4], s));
    (void)semiring_dispatch(semiring, [&](auto sr) {
        numeric_launch<decltype(sr)>(p, o, s);
        return TSG_OK;
    });
    TSG_HIP(hipGetLastError());
    if (ev) TSG_HIP(hipEventRecord(ev[5], s));
    TSG_HIP(hipMemcpyAsync(p.hmiss, p.miss, sizeof(int), hipMemcpyDeviceToHost, s));
    TSG_TRY(stream_wait(s));
    *missed = *p.hmiss;
    return TSG_OK;
}

}  // namespace tsg
