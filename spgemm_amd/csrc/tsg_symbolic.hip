// tsg_symbolic.hip -- symbolic SpGEMM: C's row pointers and columns without
// values (gfx950, wave64).  DESIGN.md section 3.9.
//
// Count-first: every row's length is counted, the counts are scanned into the
// row pointers, then each column is written once at its final place.  Nothing
// is sized by the products: no staging, no values, no compaction.  Both phases
// walk the same products; what a row keeps between them is its count alone.
//
// Rows are binned by P, their element products (symbolic_row_list,
// tsg_internal.h; P bounds the row's length):
//   packed  P <= 32      16 lanes per row, 16 rows per workgroup.  The products'
//                        columns land in a 32-int LDS slice in any order; a column
//                        survives at its first position, and a survivor's rank --
//                        the survivors below it -- is its place in the row
//   set     P <= 4,096   an LDS hash set of 2 * cap slots (linear probing,
//                        atomicCAS).  Count: the successful insertions.  Fill: the
//                        table is sorted (bitonic, empty slots last) and its head
//                        written out.  A wave per row up to 512 products (1,024
//                        slots, 4 KiB; 4 rows per workgroup), a workgroup per row
//                        past it (8,192 slots, 32 KiB)
//   window  P <= 65,536  (row, window of kSymWindow = 131,072 columns) units over
//                        the row's column span (all of [0, n) for an unsorted B).
//                        A unit marks its columns in a 16 KiB LDS bitmap; its
//                        popcount is its count, a bit's rank within the window
//                        plus the unit's offset within the row is its position:
//                        ascending with no sort.  With a sorted B each B row's
//                        start inside the window is a binary search, else the
//                        unit walks whole B rows and drops what lies outside
//   hub     the rest     units of at most 4,096 products set bits in an n-bit
//                        bitmap per row in global memory; segments of 4,096 words
//                        are popcounted and ranked.  Rows go in batches of bitmaps
//                        within kSymHubBitmapBytes
// Every walk reads the A entries' B-row bounds from one table (launch_entry_bounds)
// and gives each A entry a group of lanes: 8 or more in the bitmap classes, down
// to 2 in the set class where the B rows are short (sym_walk) -- more where the
// entries are fewer than the groups.  Nothing needs B's or A's rows sorted: a
// bitmap and a set are unions.  All indices come from validated operands (dev_operands_validate
// runs first), LDS indices are bounded by the classes' caps, which the classify
// kernel applies to the device's own product counts.
//
// The masked pass (dev_symbolic_masked) keeps of every
// row the columns in a structural mask's row, or those outside it.  It is the
// MASKED instantiation of the count and fill kernels; classes, units and
// batches are the same, since P still bounds a row's length.  packed and set
// test a column against the mask row by a bounded search, once per distinct
// column; the bitmap classes build the mask row's bits for a thread's 512
// columns in registers (sym_mask_words) and cut its words down before they are
// popcounted or ranked.  The mask is validated with the operands.
#include <algorithm>
#include <type_traits>

#include "tsg_dev_common.h"

namespace tsg {

constexpr int SYM_G = 8;                    // lanes per A entry at least
constexpr int SYM_WPT = 16;                 // bitmap words per thread in the popcount / rank passes
constexpr int SYM_SEG = WG * SYM_WPT;       // words per hub segment (4,096)
static_assert(kSymWindow / 32 == SYM_SEG, "a window is one workgroup's words: 16 per thread");
static_assert(kSymPackedProducts == 32, "the packed slice: two products per lane of a 16-lane group");

struct SymOps {
    const int *rpA;
    const int2 *ebnd;  // per A entry: its B row's [start, end)
    const long long *E;  // per A entry: the products before it (nnz(A) + 1 values)
    const int *ciB;
    int *rp;           // C's row pointers: counts before the scan
    int *ci;           // C's columns (fill)
};
// the masked pass's (section 3.11): the structural mask and the sense beside them.  The
// MASKED instantiations take this one; the others keep SymOps, so their argument
// layout -- and with it their code -- is what it was before there was a mask
struct SymOpsMasked : SymOps {
    const int *rpM, *ciM;
    int comp;          // 0: keep the columns in the mask's row, 1: those outside it
};
template <bool MASKED> using SymOpsFor = std::conditional_t<MASKED, SymOpsMasked, SymOps>;

// whether the masked pass keeps column c of a row whose mask row is ciM[m0, m1) (strictly ascending)
__device__ __forceinline__ bool sym_keep(const SymOpsMasked &o, int m0, int m1, int c) {
    const int p = lower_bound_dev(o.ciM, m0, m1, c);
    return (p < m1 && o.ciM[p] == c) != (o.comp != 0);
}
// a row no column of which can be kept: the plain sense on an empty mask row
__device__ __forceinline__ bool sym_row_dead(const SymOpsMasked &o, int m0, int m1) { return !o.comp && m0 == m1; }

// the lanes per A entry for ne entries among T threads: as few groups as entries
__device__ __forceinline__ int sym_group(int T, int ne) {
    int g = T;
    while (g > SYM_G && T / g < ne) g >>= 1;
    return g;
}

// f(column) for every product of the A entries [a0, a1), T threads together.
// Lanes per entry: halved from T while the groups are fewer than the entries
// and a group is still wider than the B rows are long on average (P products
// in all; webbase's B rows hold 3 entries) -- 2 at least.  SYM_ILP entries per
// group are in flight at once: a product is two dependent loads (the entry's
// bounds, then the column), and a short B row leaves nothing else to overlap.
constexpr int SYM_ILP = 4;
template <class F>
__device__ __forceinline__ void sym_walk(const SymOps &o, int a0, int a1, long long P, int t, int T, F f) {
    const int ne = a1 - a0;
    if (ne <= 0) return;
    const long long avg = (P + ne - 1) / ne;
    int G = T;
    while (G > 2 && T / G < ne && G > avg) G >>= 1;
    const int ng = T / G, l = t % G;
    for (int e = a0 + t / G; e < a1; e += SYM_ILP * ng) {
        int2 b[SYM_ILP];
        int c[SYM_ILP];
#pragma unroll
        for (int u = 0; u < SYM_ILP; ++u) b[u] = e + u * ng < a1 ? o.ebnd[e + u * ng] : make_int2(0, 0);
#pragma unroll
        for (int u = 0; u < SYM_ILP; ++u) c[u] = b[u].x + l < b[u].y ? o.ciB[b[u].x + l] : -1;
#pragma unroll
        for (int u = 0; u < SYM_ILP; ++u) {
            if (c[u] >= 0) f(c[u]);
            for (int q = b[u].x + l + G; q < b[u].y; q += G) f(o.ciB[q]);
        }
    }
}

template <int T> __device__ __forceinline__ void sym_sync() {
    if constexpr (T == WG) __syncthreads(); else wave_lds_sync();
}

// ---------------------------------------------------------------------------
// setup kernels
// ---------------------------------------------------------------------------
// per A entry its B row's length; the scan makes them the products' prefix E
__global__ __launch_bounds__(WG) void k_sym_entry_len(const int2 *ebnd, long nnzA, long long *E) {
    for (long p = (long)blockIdx.x * WG + threadIdx.x; p <= nnzA; p += (long)gridDim.x * WG) {
        long long v = 0;
        if (p < nnzA) {
            const int2 b = ebnd[p];
            v = b.y - b.x;
        }
        E[p] = v;
    }
}

// SYM_CPT rows per thread: their products, their lists, the totals.  A list's
// places go by one LDS atomic per wave and one global atomic per workgroup (a
// global atomic per wave on five hot words measured 0.58 ms on webbase's 1 M
// rows).  Rows without products get their count (0) here.
constexpr int SYM_CPT = 8;
__global__ __launch_bounds__(WG) void k_sym_classify(const int *rpA, const long long *E, int m, int *rp, int *lists,
                                                     SymCounters *cnt) {
    __shared__ long long red[WAVES];
    __shared__ int s_n[kSymLists], s_base[kSymLists];
    const int lane = lane_id();
    const u64 below = (1ull << lane) - 1ull;
    long long prod = 0, hubu = 0;
    for (long base = (long)blockIdx.x * WG * SYM_CPT; base < m; base += (long)gridDim.x * WG * SYM_CPT) {
        if (threadIdx.x < kSymLists) s_n[threadIdx.x] = 0;
        __syncthreads();
        int l[SYM_CPT], pos[SYM_CPT];
#pragma unroll
        for (int k = 0; k < SYM_CPT; ++k) {
            const long row = base + k * WG + threadIdx.x;
            l[k] = -1;
            pos[k] = 0;
            if (row < m) {
                const long long P = E[rpA[row + 1]] - E[rpA[row]];
                l[k] = symbolic_row_list(P);
                prod += P;
                if (l[k] == kSymListHub) hubu += (P + kSymHubUnitProducts - 1) / kSymHubUnitProducts;
                if (l[k] < 0) rp[row] = 0;
            }
#pragma unroll
            for (int t = 0; t < kSymLists; ++t) {
                const u64 msk = __ballot(l[k] == t);
                if (!msk) continue;
                const int leader = __ffsll((long long)msk) - 1;
                int p0 = 0;
                if (lane == leader) p0 = atomicAdd(&s_n[t], __popcll(msk));
                p0 = __builtin_amdgcn_readlane(p0, leader);
                if (l[k] == t) pos[k] = p0 + __popcll(msk & below);
            }
        }
        __syncthreads();
        if (threadIdx.x < kSymLists && s_n[threadIdx.x])
            s_base[threadIdx.x] = atomicAdd(&cnt->nlist[threadIdx.x], s_n[threadIdx.x]);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SYM_CPT; ++k)
            if (l[k] >= 0) lists[(long)l[k] * m + s_base[l[k]] + pos[k]] = (int)(base + k * WG + threadIdx.x);
        __syncthreads();
    }
    prod = block_sum(prod, red);
    hubu = block_sum(hubu, red);
    if (threadIdx.x == 0) {
        if (prod) atomicAdd(&cnt->products, (u64)prod);
        if (hubu) atomicAdd(&cnt->hub_units, (u64)hubu);
        if (blockIdx.x == 0) rp[m] = 0;
    }
}

// a wave per window-class row: its column span (sorted B: from the B rows' first
// and last entries; else all of [0, n)), cut into windows.  win[i] (i: the row's
// place in its list): (first window's first column, windows, last column, -);
// nwin[i]: the windows again, for the scan that gives the row's first unit
// (zeroed past the list's end by the host).
__global__ __launch_bounds__(WG) void k_sym_spans(const int *list, SymOps o, int n, int bsorted, int4 *win,
                                                  long long *nwin, const SymCounters *cnt) {
    const int nrows = cnt->nlist[kSymListWindow], lane = lane_id();
    for (long i = (long)blockIdx.x * WAVES + wave_id(); i < nrows; i += (long)gridDim.x * WAVES) {
        const int row = list[i];
        int lo = 0, hi = n - 1;
        if (bsorted) {
            lo = INT_MAX;
            hi = -1;
            const int a1 = o.rpA[row + 1];
            for (int e = o.rpA[row] + lane; e < a1; e += 64) {
                const int2 b = o.ebnd[e];
                if (b.y > b.x) {
                    lo = min(lo, o.ciB[b.x]);
                    hi = max(hi, o.ciB[b.y - 1]);
                }
            }
            lo = wave_last(wave_incl_dpp(lo, INT_MAX, OpMin{}));
            hi = wave_last(wave_incl_dpp(hi, INT_MIN, OpMax{}));
        }
        if (lane == 0) {
            const int w0 = lo & ~31;  // (the row has products: lo <= hi)
            const int nw = (hi - w0) / kSymWindow + 1;
            win[i] = make_int4(w0, nw, hi, 0);
            nwin[i] = nw;
        }
    }
}

// the unit list: (row, the window's first column, its columns, -).  ubase[i]:
// the row's first unit (fits an int: the host refuses more than kSymMaxWinUnits)
__global__ __launch_bounds__(WG) void k_sym_units(const int *list, int nrows, const int4 *win, const long long *ubase,
                                                  int4 *units) {
    for (long i = (long)blockIdx.x * WAVES + wave_id(); i < nrows; i += (long)gridDim.x * WAVES) {
        const int4 w = win[i];
        const int row = list[i], u0 = (int)ubase[i];
        for (int k = lane_id(); k < w.y; k += 64) {
            const int wlo = w.x + k * kSymWindow;
            units[u0 + k] = make_int4(row, wlo, min(kSymWindow, w.z + 1 - wlo), 0);
        }
    }
}

// ---------------------------------------------------------------------------
// packed class
// ---------------------------------------------------------------------------
template <bool FILL, bool MASKED>
__global__ __launch_bounds__(WG) void k_sym_packed(const int *list, int nrows, SymOpsFor<MASKED> o) {
    constexpr int CAP = (int)kSymPackedProducts, L = 16;
    __shared__ int s_key[WG / L][CAP], s_uni[WG / L][CAP], s_n[WG / L];
    const int g = threadIdx.x / L, l = threadIdx.x % L;
    const long li = (long)blockIdx.x * (WG / L) + g;
    const bool have = li < nrows;
    const int row = have ? list[li] : 0;
    const int a0 = have ? o.rpA[row] : 0;
    int a1 = have ? o.rpA[row + 1] : 0;
    int m0 = 0, m1 = 0;
    if constexpr (MASKED) {
        m0 = have ? o.rpM[row] : 0, m1 = have ? o.rpM[row + 1] : 0;
        if (sym_row_dead(o, m0, m1)) a1 = a0;  // (no products gathered: the count is 0)
    }
    int *key = s_key[g], *uni = s_uni[g];
    if (l == 0) s_n[g] = 0;
    wave_lds_sync();
    for (int e = a0 + l; e < a1; e += L) {
        const int2 b = o.ebnd[e];
        const int len = b.y - b.x;
        if (len > 0) {
            const int pos = atomicAdd(&s_n[g], len);
            for (int q = 0; q < len; ++q)
                if (pos + q < CAP) key[pos + q] = o.ciB[b.x + q];
        }
    }
    wave_lds_sync();
    const int P = min(s_n[g], CAP);
    int mine = 0;
#pragma unroll
    for (int h = 0; h < CAP / L; ++h) {
        const int p = l + h * L;
        if (p < P) {
            const int x = key[p];
            bool first = true;
            for (int q = 0; q < p; ++q) first = first && key[q] != x;
            if constexpr (MASKED) first = first && sym_keep(o, m0, m1, x);  // (dropped: as a repeat, ranked by no one)
            uni[p] = first ? x : INT_MAX;  // (no column is INT_MAX: columns lie below n)
            mine += first ? 1 : 0;
        }
    }
    wave_lds_sync();
    if constexpr (!FILL) {
        mine += __shfl_xor(mine, 8, L);
        mine += __shfl_xor(mine, 4, L);
        mine += __shfl_xor(mine, 2, L);
        mine += __shfl_xor(mine, 1, L);
        if (have && l == 0) o.rp[row] = mine;
    } else {
        const int c0 = have ? o.rp[row] : 0;
#pragma unroll
        for (int h = 0; h < CAP / L; ++h) {
            const int p = l + h * L;
            if (p < P) {
                const int x = uni[p];
                if (x != INT_MAX) {
                    int rank = 0;
                    for (int q = 0; q < P; ++q) rank += uni[q] < x ? 1 : 0;
                    o.ci[c0 + rank] = x;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// set class: T threads per row (64: a wave, 256: the workgroup), CAP products at most
// ---------------------------------------------------------------------------
template <int T, int LOG_HS, bool FILL, bool MASKED>
__global__ __launch_bounds__(WG) void k_sym_set(const int *list, int nrows, SymOpsFor<MASKED> o) {
    constexpr int SLOTS = WG / T, HS = 1 << LOG_HS, DN = FILL ? HS / 2 : 1;
    __shared__ int s_tab[SLOTS][HS];
    __shared__ int s_dense[SLOTS][DN];  // (fill) the set's columns, packed, then sorted
    __shared__ int s_cur[SLOTS];
    __shared__ int s_red[WAVES];
    const int slot = threadIdx.x / T, t = threadIdx.x % T;
    const long li = (long)blockIdx.x * SLOTS + slot;
    const bool have = li < nrows;
    const int row = have ? list[li] : 0;
    const int a0 = have ? o.rpA[row] : 0;
    int a1 = have ? o.rpA[row + 1] : 0;
    int m0 = 0, m1 = 0;
    if constexpr (MASKED) {
        m0 = have ? o.rpM[row] : 0, m1 = have ? o.rpM[row + 1] : 0;
        if (sym_row_dead(o, m0, m1)) a1 = a0;  // (nothing walked: the count is 0; uniform over the row's threads)
    }
    // the row's table: the power of two from 2 P slots up (64 at least, HS at most: P is within the class's cap)
    const long long P = have ? o.E[a1] - o.E[a0] : 0;
    int lg = 6;
    while (lg < LOG_HS && (1ll << lg) < 2 * P) ++lg;
    const int hs = 1 << lg;
    int *tab = s_tab[slot];
    for (int q = t; q < hs; q += T) tab[q] = -1;
    if (t == 0) s_cur[slot] = 0;
    sym_sync<T>();
    int added = 0;
    sym_walk(o, a0, a1, P, t, T, [&](int c) {
        u32 h = ((u32)c * 2654435761u) >> (32 - lg);
        // (the row's distinct columns are at most hs / 2: a free slot is always met; the
        // bound only keeps a miscounted row from spinning)
        for (int probe = 0; probe < hs; ++probe) {
            const int old = atomicCAS(&tab[h], -1, c);
            if (old == -1) {  // (once per distinct column: the mask is tested here)
                if constexpr (MASKED) added += sym_keep(o, m0, m1, c) ? 1 : 0;
                else ++added;
                break;
            }
            if (old == c) break;
            h = (h + 1) & (hs - 1);
        }
    });
    sym_sync<T>();
    if constexpr (!FILL) {
        int tot;
        if constexpr (T == WG) tot = block_sum(added, s_red);
        else tot = wave_sum(added);
        if (have && t == 0) o.rp[row] = tot;
    } else {
        // the set's columns packed into dense[0, len), padded to a power of two with
        // keys that sort last, sorted by a bitonic network as unsigned keys
        u32 *k = reinterpret_cast<u32 *>(s_dense[slot]);
        for (int q0 = 0; q0 < hs; q0 += T) {  // (hs is a multiple of 64: whole waves; one atomic per wave and step)
            int v = tab[q0 + t];
            if constexpr (MASKED)
                if (v != -1 && !sym_keep(o, m0, m1, v)) v = -1;  // (the sort sees kept columns only)
            const u64 msk = __ballot(v != -1);
            if (msk) {
                const int leader = __ffsll((long long)msk) - 1;
                int p0 = 0;
                if (lane_id() == leader) p0 = atomicAdd(&s_cur[slot], __popcll(msk));
                p0 = __builtin_amdgcn_readlane(p0, leader);
                const int pos = p0 + __popcll(msk & ((1ull << lane_id()) - 1ull));
                if (v != -1 && pos < DN) k[pos] = (u32)v;
            }
        }
        sym_sync<T>();
        const int len = min(s_cur[slot], DN);
        int N = 2;
        while (N < len) N <<= 1;
        for (int q = len + t; q < N; q += T) k[q] = 0xffffffffu;
        sym_sync<T>();
        for (int span = 2; span <= N; span <<= 1)
            for (int j = span >> 1; j > 0; j >>= 1) {
                for (int i = t; i < N / 2; i += T) {
                    const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a | j;
                    const u32 x = k[a], y = k[b];
                    const bool up = (a & span) == 0;
                    if ((x > y) == up) {
                        k[a] = y;
                        k[b] = x;
                    }
                }
                sym_sync<T>();
            }
        const int c0 = have ? o.rp[row] : 0;
        const int out = have ? min(o.rp[row + 1] - c0, len) : 0;
        for (int q = t; q < out; q += T) o.ci[c0 + q] = (int)k[q];
    }
}

// ---------------------------------------------------------------------------
// bitmaps: set, popcount, rank
// ---------------------------------------------------------------------------
__device__ __forceinline__ void sym_set_bit(u32 *bm, int d) {
    const u32 bit = 1u << (d & 31);
    if (!(bm[d >> 5] & bit)) atomicOr(&bm[d >> 5], bit);  // (a stale read costs one atomic more, nothing else)
}

// this thread's SYM_WPT words, from 16-byte loads
__device__ __forceinline__ int sym_load_words(const u32 *bm, u32 (&w)[SYM_WPT]) {
    const uint4 *v = reinterpret_cast<const uint4 *>(bm) + threadIdx.x * (SYM_WPT / 4);
    int pop = 0;
#pragma unroll
    for (int k = 0; k < SYM_WPT / 4; ++k) {
        const uint4 x = v[k];
        w[4 * k] = x.x, w[4 * k + 1] = x.y, w[4 * k + 2] = x.z, w[4 * k + 3] = x.w;
        pop += __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w);
    }
    return pop;
}

// masked pass: the thread's words, which stand for the columns [col0, col0 + 32 * SYM_WPT),
// cut down to the columns the mask row ciM[m0, m1) keeps; the popcount of what is left.
// One lower bound for col0, then the mask entries consumed while they fall in word k
// (k static: the words stay in registers).  Count and fill, and a hub batch's re-mark,
// apply it to the same words, so their ranks agree.
__device__ __forceinline__ int sym_mask_words(const SymOpsMasked &o, int m0, int m1, int col0, u32 (&w)[SYM_WPT]) {
    constexpr int NC = 32 * SYM_WPT;
    int p = lower_bound_dev(o.ciM, m0, m1, col0);
    int d = p < m1 ? o.ciM[p] - col0 : NC;  // the next mask entry's place among the thread's columns (>= 0)
    int pop = 0;
#pragma unroll
    for (int k = 0; k < SYM_WPT; ++k) {
        u32 mw = 0u;
        while (d < (k + 1) * 32) {
            mw |= 1u << (d - k * 32);
            ++p;
            d = p < m1 ? o.ciM[p] - col0 : NC;
        }
        w[k] &= o.comp ? ~mw : mw;
        pop += __popc(w[k]);
    }
    return pop;
}

// the set bits of the thread's words as columns, ascending, from out on
__device__ __forceinline__ void sym_emit(const u32 (&w)[SYM_WPT], int col0, int *out) {
#pragma unroll
    for (int k = 0; k < SYM_WPT; ++k) {
        u32 x = w[k];
        while (x) {
            *out++ = col0 + k * 32 + (__ffs((int)x) - 1);
            x &= x - 1;
        }
    }
}

// window class: a workgroup per (row, window) unit.  ucnt: the unit's columns;
// uoff: its offset within its row (k_sym_unit_scan)
template <bool FILL, bool MASKED>
__global__ __launch_bounds__(WG) void k_sym_window(const int4 *units, SymOpsFor<MASKED> o, int bsorted, int *ucnt,
                                                   const int *uoff) {
    __shared__ __attribute__((aligned(16))) u32 bm[SYM_SEG];
    __shared__ int s_red[WAVES];
    const int tid = threadIdx.x;
    const int4 u = units[blockIdx.x];
    if (FILL && ucnt[blockIdx.x] == 0) return;  // (block-uniform)
    const int row = u.x, wlo = u.y;
    int m0 = 0, m1 = 0;
    if constexpr (MASKED) {
        m0 = o.rpM[row], m1 = o.rpM[row + 1];
        if (!FILL && sym_row_dead(o, m0, m1)) {  // (block-uniform; the fill has left through ucnt)
            if (tid == 0) ucnt[blockIdx.x] = 0;
            return;
        }
    }
    const int wn = min(u.z, kSymWindow);  // the window's columns: [wlo, wlo + wn), up to the row's last
    // (only the words the row's span reaches, rounded up to whole threads' shares, are zeroed and read)
    const int nwords = min(((wn + 31) / 32 + SYM_WPT - 1) / SYM_WPT * SYM_WPT, SYM_SEG);
    for (int q = tid; q < nwords; q += WG) bm[q] = 0u;
    __syncthreads();
    const int a0 = o.rpA[row], a1 = o.rpA[row + 1];
    const int G = sym_group(WG, a1 - a0);
    for (int e = a0 + tid / G; e < a1; e += WG / G) {
        const int2 b = o.ebnd[e];
        if (bsorted) {
            for (int q = lower_bound_dev(o.ciB, b.x, b.y, wlo) + tid % G; q < b.y; q += G) {
                const int d = o.ciB[q] - wlo;
                if (d >= wn) break;
                sym_set_bit(bm, d);
            }
        } else {
            for (int q = b.x + tid % G; q < b.y; q += G) {
                const int d = o.ciB[q] - wlo;
                if ((unsigned)d < (unsigned)wn) sym_set_bit(bm, d);
            }
        }
    }
    __syncthreads();
    u32 w[SYM_WPT];
    const bool in = tid * SYM_WPT < nwords;
    int pop = in ? sym_load_words(bm, w) : 0;
    if constexpr (MASKED)
        if (pop) pop = sym_mask_words(o, m0, m1, wlo + tid * SYM_WPT * 32, w);
    if constexpr (!FILL) {
        const int tot = block_sum(pop, s_red);
        if (tid == 0) ucnt[blockIdx.x] = tot;
    } else {
        int tot;
        const int off = block_excl_scan(pop, &tot, s_red);
        if (pop) sym_emit(w, wlo + tid * SYM_WPT * 32, o.ci + o.rp[row] + uoff[blockIdx.x] + off);
    }
}

// a wave per window-class row: its units' counts -> offsets within the row, their sum -> the row's count
__global__ __launch_bounds__(WG) void k_sym_unit_scan(const int *list, int nrows, const int4 *win,
                                                      const long long *ubase, const int *ucnt, int *uoff, int *rp) {
    for (long i = (long)blockIdx.x * WAVES + wave_id(); i < nrows; i += (long)gridDim.x * WAVES) {
        const int4 w = win[i];
        const int u0 = (int)ubase[i];
        int run = 0;
        for (int k0 = 0; k0 < w.y; k0 += 64) {
            const int k = k0 + lane_id();
            const int v = k < w.y ? ucnt[u0 + k] : 0;
            const int inc = wave_incl_scan_dpp(v);
            if (k < w.y) uoff[u0 + k] = run + inc - v;
            run += wave_last(inc);
        }
        if (lane_id() == 0) rp[list[i]] = run;
    }
}

// hub class.  grid: (chunks' stride, the batch's rows); bm: the batch's bitmaps, wpr words per row
__global__ __launch_bounds__(WG) void k_sym_hub_set(const int *list, SymOps o, const long long *E, u32 *bm, long wpr) {
    const int tid = threadIdx.x;
    const int row = list[blockIdx.y];
    const int a0 = o.rpA[row], a1 = o.rpA[row + 1];
    const long long pb = E[a0], pe = E[a1];
    const long long nun = (pe - pb + kSymHubUnitProducts - 1) / kSymHubUnitProducts;
    u32 *b = bm + (size_t)blockIdx.y * wpr;
    for (long long un = blockIdx.x; un < nun; un += gridDim.x) {
        const long long p0 = pb + un * kSymHubUnitProducts, p1 = min(p0 + kSymHubUnitProducts, pe);
        // the entries holding products p0 and p1 - 1: the last e of [a0, a1) with E[e] <= p
        int elo, ehi;
        {
            int lo = a0, hi = a1 - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (E[mid] <= p0) lo = mid; else hi = mid - 1;
            }
            elo = lo;
            hi = a1 - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (E[mid] <= p1 - 1) lo = mid; else hi = mid - 1;
            }
            ehi = lo;
        }
        const int G = sym_group(WG, ehi - elo + 1);
        for (int e = elo + tid / G; e <= ehi; e += WG / G) {
            const int2 br = o.ebnd[e];
            const long long Ee = E[e];
            const int q0 = br.x + (int)max(0ll, p0 - Ee);
            const int q1 = (int)min((long long)br.y, br.x + (p1 - Ee));
            for (int q = q0 + tid % G; q < q1; q += G) sym_set_bit(b, o.ciB[q]);
        }
    }
}

// grid: (segments, the batch's rows): the segment's set bits
// (MASKED: of the columns the row's mask keeps; list, o: read by that instantiation alone)
template <bool MASKED>
__global__ __launch_bounds__(WG) void k_sym_hub_seg(const u32 *bm, long wpr, int nseg, int *segcnt, const int *list,
                                                    SymOpsFor<MASKED> o) {
    __shared__ int s_red[WAVES];
    u32 w[SYM_WPT];
    const long w0 = (long)blockIdx.x * SYM_SEG;
    int pop = 0;
    if (w0 + (long)threadIdx.x * SYM_WPT < wpr) pop = sym_load_words(bm + (size_t)blockIdx.y * wpr + w0, w);
    if constexpr (MASKED) {
        if (pop) {
            const int row = list[blockIdx.y];
            pop = sym_mask_words(o, o.rpM[row], o.rpM[row + 1], (int)((w0 + (long)threadIdx.x * SYM_WPT) * 32), w);
        }
    }
    pop = block_sum(pop, s_red);
    if (threadIdx.x == 0) segcnt[(long)blockIdx.y * nseg + blockIdx.x] = pop;
}

// a wave per row of the batch: its segments' counts -> offsets; COUNT: their sum -> the row's count
template <bool COUNT>
__global__ __launch_bounds__(WG) void k_sym_hub_rows(const int *list, int nrows, int nseg, int *segcnt, int *rp) {
    const long i = (long)blockIdx.x * WAVES + wave_id();
    if (i >= nrows) return;  // (wave-uniform)
    int *sc = segcnt + i * nseg;
    int run = 0;
    for (int k0 = 0; k0 < nseg; k0 += 64) {
        const int k = k0 + lane_id();
        const int v = k < nseg ? sc[k] : 0;
        const int inc = wave_incl_scan_dpp(v);
        if (k < nseg) sc[k] = run + inc - v;
        run += wave_last(inc);
    }
    if (COUNT && lane_id() == 0) rp[list[i]] = run;
}

// grid: (segments, the batch's rows): the segment's columns at their ranks
template <bool MASKED>
__global__ __launch_bounds__(WG) void k_sym_hub_fill(const int *list, SymOpsFor<MASKED> o, const u32 *bm, long wpr,
                                                     int nseg, const int *segoff) {
    __shared__ int s_red[WAVES];
    u32 w[SYM_WPT];
    const long w0 = (long)blockIdx.x * SYM_SEG;
    const bool in = w0 + (long)threadIdx.x * SYM_WPT < wpr;
    int pop = 0;
    if (in) pop = sym_load_words(bm + (size_t)blockIdx.y * wpr + w0, w);
    if constexpr (MASKED) {
        if (pop) {  // (the words the count ranked: the same mask again, on a batch's re-mark too)
            const int row = list[blockIdx.y];
            pop = sym_mask_words(o, o.rpM[row], o.rpM[row + 1], (int)((w0 + (long)threadIdx.x * SYM_WPT) * 32), w);
        }
    }
    int tot;
    const int off = block_excl_scan(pop, &tot, s_red);
    if (in && pop)
        sym_emit(w, (int)((w0 + (long)threadIdx.x * SYM_WPT) * 32),
                 o.ci + o.rp[list[blockIdx.y]] + segoff[(long)blockIdx.y * nseg + blockIdx.x] + off);
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
// MK: the masked pass (M, comp: its mask and sense; else M is null) -- the same host
// steps over the kernels' MASKED instantiations
template <bool MK>
static int symbolic_run(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, const tsg_dev_csr *M, int comp,
                        int mode, tsg_dev_csr &C, tsg_symbolic_info &info, hipStream_t s, hipEvent_t *ev) {
    C = tsg_dev_csr{};
    info = tsg_symbolic_info{};
    if (mode != TSG_SYMBOLIC_PATTERN && mode != TSG_SYMBOLIC_COUNT) return TSG_ERR_INVALID;
    bool bsorted = false;
    if constexpr (MK) {
        if (comp != 0 && comp != 1) return TSG_ERR_INVALID;
        TSG_TRY(dev_numeric_validate(cx, A, B, *M, &bsorted, s));  // (the mask as the masked plan validates its own)
    } else {
        TSG_TRY(dev_operands_validate(cx, A, B, &bsorted, s));
    }
    info.b_rows_sorted = bsorted ? 1 : 0;
    const int m = A.m, n = B.n;
    PoolScope ws(cx);  // (temporaries and half-built outputs: back to the pool on every way out)
    int *rp = nullptr;
    TSG_TRY(ws.get(&rp, (size_t)m + 1));
    for (int e = 4; e < 8; ++e) TSG_HIP(hipEventRecord(ev[e], s));  // (an early way out leaves valid brackets)
    if (m == 0 || A.nnz == 0 || B.nnz == 0 || n == 0) {
        TSG_HIP(hipMemsetAsync(rp, 0, ((size_t)m + 1) * sizeof(int), s));
        TSG_TRY(stream_wait(s));
        C = tsg_dev_csr{m, n, 0, ws.keep(rp), nullptr, nullptr};
        return TSG_OK;
    }
    // 1. the entry table, the products' prefix, the classes
    int2 *ebnd = nullptr;
    long long *E = nullptr;
    int *lists = nullptr;
    int4 *win = nullptr;
    SymCounters *cnt = nullptr;
    TSG_TRY(ws.get(&ebnd, (size_t)A.nnz));
    TSG_TRY(ws.get(&E, (size_t)A.nnz + 1));
    TSG_TRY(ws.get(&lists, (size_t)kSymLists * m));
    long long *nwin = nullptr;  // per window-class row (by its place in the list): windows, scanned: first unit
    TSG_TRY(ws.get(&win, (size_t)m));
    TSG_TRY(ws.get(&nwin, (size_t)m + 1));
    TSG_TRY(ws.get(&cnt, 1));
    TSG_HIP(hipMemsetAsync(cnt, 0, sizeof(SymCounters), s));
    TSG_TRY(launch_entry_bounds(A, B, ebnd, s));
    k_sym_entry_len<<<grid_for((long)A.nnz + 1, WG, 16384), WG, 0, s>>>(ebnd, A.nnz, E);
    TSG_HIP(hipGetLastError());
    TSG_TRY(dev_scan_i64(cx, E, (long)A.nnz + 1, s));
    SymOpsFor<MK> o{};
    static_cast<SymOps &>(o) = SymOps{A.rowpointer, ebnd, E, B.columnindex, rp, nullptr};
    if constexpr (MK) o.rpM = M->rowpointer, o.ciM = M->columnindex, o.comp = comp;
    TSG_HIP(hipMemsetAsync(nwin, 0, ((size_t)m + 1) * sizeof(long long), s));
    k_sym_classify<<<grid_for(m, WG * SYM_CPT, 16384), WG, 0, s>>>(A.rowpointer, E, m, rp, lists, cnt);
    k_sym_spans<<<grid_for(m, WAVES, 2048), WG, 0, s>>>(lists + (size_t)kSymListWindow * m, o, n, bsorted ? 1 : 0, win,
                                                        nwin, cnt);
    TSG_HIP(hipGetLastError());
    TSG_TRY(dev_scan_i64(cx, nwin, (long)m + 1, s));  // (nwin[m]: the window units in all)
    TSG_HIP(hipMemcpyAsync(&cx.slots->sym, cnt, sizeof(SymCounters), hipMemcpyDeviceToHost, s));
    TSG_HIP(hipMemcpyAsync(&cx.slots->sym.win_units, nwin + m, sizeof(long long), hipMemcpyDeviceToHost, s));
    TSG_TRY(stream_wait(s));  // (host round trip 1 of 2: the class counts and unit totals)
    const SymCounters h = cx.slots->sym;
    const auto cnt_of = [&](int l) { return h.nlist[l]; };
    const auto list_of = [&](int l) { return lists + (size_t)l * m; };
    info.products = (long long)h.products;
    info.rows_class[0] = cnt_of(kSymListPacked);
    info.rows_class[1] = (long long)cnt_of(kSymListSetWave) + cnt_of(kSymListSetWg);
    info.rows_class[2] = cnt_of(kSymListWindow);
    info.rows_class[3] = cnt_of(kSymListHub);
    info.units = (long long)(h.win_units + h.hub_units);
    if (h.win_units > (u64)kSymMaxWinUnits) return TSG_ERR_OVERFLOW;
    // 2. the units and the hub batches' memory
    const int nwu = (int)h.win_units, nwl = cnt_of(kSymListWindow), nhub = cnt_of(kSymListHub);
    int4 *units = nullptr;
    int *ucnt = nullptr, *uoff = nullptr;
    if (nwu) {
        TSG_TRY(ws.get(&units, (size_t)nwu));
        TSG_TRY(ws.get(&ucnt, (size_t)nwu));
        TSG_TRY(ws.get(&uoff, (size_t)nwu));
        k_sym_units<<<grid_for(nwl, WAVES, 2048), WG, 0, s>>>(list_of(kSymListWindow), nwl, win, nwin, units);
        TSG_HIP(hipGetLastError());
    }
    const long wpr = ((long)n + 32 * SYM_WPT - 1) / (32 * SYM_WPT) * SYM_WPT;  // bitmap words per hub row
    const int nseg = (int)((wpr + SYM_SEG - 1) / SYM_SEG);
    const long long budget = cx.knobs.sym_hub_bytes > 0 ? cx.knobs.sym_hub_bytes : kSymHubBitmapBytes;
    const int batch = (int)std::max(1ll, std::min({budget / (wpr * 4), 32768ll, (long long)nhub}));
    const int nbatch = nhub ? (nhub + batch - 1) / batch : 0;
    u32 *bm = nullptr;
    int *segcnt = nullptr;
    if (nhub) {
        TSG_TRY(ws.get(&bm, (size_t)batch * wpr));
        TSG_TRY(ws.get(&segcnt, (size_t)batch * nseg));
    }
    // a batch's bitmaps: zeroed, set, popcounted per segment, the segments scanned per row
    const auto hub_marks = [&](int r0, int nr, bool count) -> int {
        const int *hl = list_of(kSymListHub) + r0;
        TSG_HIP(hipMemsetAsync(bm, 0, (size_t)nr * wpr * sizeof(u32), s));
        k_sym_hub_set<<<dim3(std::max(1, std::min(256, 4096 / nr)), nr), WG, 0, s>>>(hl, o, E, bm, wpr);
        k_sym_hub_seg<MK><<<dim3(nseg, nr), WG, 0, s>>>(bm, wpr, nseg, segcnt, hl, o);
        if (count) k_sym_hub_rows<true><<<(nr + WAVES - 1) / WAVES, WG, 0, s>>>(hl, nr, nseg, segcnt, rp);
        else k_sym_hub_rows<false><<<(nr + WAVES - 1) / WAVES, WG, 0, s>>>(hl, nr, nseg, segcnt, rp);
        TSG_HIP(hipGetLastError());
        return TSG_OK;
    };
    // a list's rows, per rows to a workgroup, in launches of at most kMaxGridBlocks workgroups
    const auto rows_launch = [&](int l, int per, auto &&launch) {
        const long step = (long)kMaxGridBlocks * per;
        for (long r0 = 0; r0 < cnt_of(l); r0 += step) launch(list_of(l) + r0, (int)std::min(step, cnt_of(l) - r0));
    };
    // 3. count (the long rows first: their tails overlap the short rows' kernels)
    TSG_HIP(hipEventRecord(ev[4], s));
    for (int b = 0; b < nbatch; ++b) TSG_TRY(hub_marks(b * batch, std::min(batch, nhub - b * batch), true));
    for (int u0 = 0; u0 < nwu; u0 += kMaxGridBlocks)
        k_sym_window<false, MK><<<std::min(nwu - u0, kMaxGridBlocks), WG, 0, s>>>(units + u0, o, bsorted ? 1 : 0,
                                                                                 ucnt + u0, uoff + u0);
    if (nwu)
        k_sym_unit_scan<<<grid_for(nwl, WAVES, 2048), WG, 0, s>>>(list_of(kSymListWindow), nwl, win, nwin, ucnt, uoff,
                                                                  rp);
    rows_launch(kSymListSetWg, 1, [&](const int *l, int c) {
        k_sym_set<WG, 13, false, MK><<<c, WG, 0, s>>>(l, c, o);
    });
    rows_launch(kSymListSetWave, WAVES, [&](const int *l, int c) {
        k_sym_set<64, 10, false, MK><<<(c + WAVES - 1) / WAVES, WG, 0, s>>>(l, c, o);
    });
    rows_launch(kSymListPacked, 16, [&](const int *l, int c) {
        k_sym_packed<false, MK><<<(c + 15) / 16, WG, 0, s>>>(l, c, o);
    });
    TSG_HIP(hipGetLastError());
    TSG_HIP(hipEventRecord(ev[5], s));
    TSG_HIP(hipEventRecord(ev[6], s));
    TSG_HIP(hipEventRecord(ev[7], s));
    // 4. the row pointers; nnz(C) in 64 bits before anything is sized by it (host round trip 2 of 2)
    long long total = 0;
    const int rc = scan_exclusive_i32_total(cx, rp, (long)m + 1, s, &total);
    info.nnzC = total;
    TSG_TRY(rc);
    if (mode == TSG_SYMBOLIC_COUNT || total == 0) {
        C = tsg_dev_csr{m, n, (int)total, ws.keep(rp), nullptr, nullptr};
        return TSG_OK;
    }
    // 5. fill: every column once, at its final place
    int *ci = nullptr;
    TSG_TRY(ws.get(&ci, (size_t)total));
    o.ci = ci;
    TSG_HIP(hipEventRecord(ev[6], s));
    for (int b = 0; b < nbatch; ++b) {
        const int r0 = b * batch, nr = std::min(batch, nhub - r0);
        if (nbatch > 1) TSG_TRY(hub_marks(r0, nr, false));  // (one batch: the count's bitmaps and offsets still stand)
        k_sym_hub_fill<MK><<<dim3(nseg, nr), WG, 0, s>>>(list_of(kSymListHub) + r0, o, bm, wpr, nseg, segcnt);
    }
    for (int u0 = 0; u0 < nwu; u0 += kMaxGridBlocks)
        k_sym_window<true, MK><<<std::min(nwu - u0, kMaxGridBlocks), WG, 0, s>>>(units + u0, o, bsorted ? 1 : 0,
                                                                                ucnt + u0, uoff + u0);
    rows_launch(kSymListSetWg, 1, [&](const int *l, int c) {
        k_sym_set<WG, 13, true, MK><<<c, WG, 0, s>>>(l, c, o);
    });
    rows_launch(kSymListSetWave, WAVES, [&](const int *l, int c) {
        k_sym_set<64, 10, true, MK><<<(c + WAVES - 1) / WAVES, WG, 0, s>>>(l, c, o);
    });
    rows_launch(kSymListPacked, 16, [&](const int *l, int c) {
        k_sym_packed<true, MK><<<(c + 15) / 16, WG, 0, s>>>(l, c, o);
    });
    TSG_HIP(hipGetLastError());
    TSG_HIP(hipEventRecord(ev[7], s));
    TSG_TRY(stream_wait(s));
    C = tsg_dev_csr{m, n, (int)total, ws.keep(rp), ws.keep(ci), nullptr};
    return TSG_OK;
}

int dev_symbolic(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, int mode, tsg_dev_csr &C,
                 tsg_symbolic_info &info, hipStream_t s, hipEvent_t *ev) {
    return symbolic_run<false>(cx, A, B, nullptr, 0, mode, C, info, s, ev);
}

int dev_symbolic_masked(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, const tsg_dev_csr &M, int comp,
                        int mode, tsg_dev_csr &C, tsg_symbolic_info &info, hipStream_t s, hipEvent_t *ev) {
    return symbolic_run<true>(cx, A, B, &M, comp, mode, C, info, s, ev);
}

}  // namespace tsg
