// tsg_ewise.hip -- element-wise union, intersection and difference of two CSR
// matrices with strictly ascending rows (gfx950, wave64).  DESIGN.md section 3.12.
//
// Count-first, like the symbolic pass: a first pass reads the columns alone and
// counts, per row or unit, the entries stored in both operands (`both`); every
// mode's length follows from it (union: la + lb - both, intersection: both,
// difference: la - both).  The counts are scanned into the row pointers, then a
// second pass over the same partition writes every column and value once at its
// final place.  Nothing is staged per entry and nothing is compacted.
//
// An entry's place needs no merge loop.  With x the index of an A entry in its
// row (or unit), pb its lower bound among the B entries and mb the matched A
// entries before it:
//   union         x + pb - mb   (every earlier A entry, and the earlier B entries without a partner in A)
//   intersection  mb            (matched entries only)
//   difference    x - mb        (unmatched entries only)
// and for an unmatched B entry of a union, y + pa - (the matched B entries
// before it).  A matched B entry writes nothing: its A partner holds op(alpha a,
// beta b).  So each lane searches the other row for its own entries, and the
// counts of matches before it come from a ballot (packed, wave) or one
// workgroup scan (tile).  Intersection, difference and every count pass walk
// the A entries only.
//
// Rows are binned by L = len A_i + len B_i (ewise_row_list, tsg_internal.h):
//   packed  L <= 32    16 lanes per row, 16 rows per workgroup; a lane holds up
//                      to two entries, the searches run in global memory
//   wave    L <= 512   a wave per row, four rows per workgroup; both rows staged
//                      in LDS (2 KiB per wave), 64 entries per step
//   tile    the rest   the row's merge path cut into units of kEwiseTile = 2,048
//                      merged entries, a workgroup per unit; the unit's two
//                      segments go to LDS, a thread takes EW_EPT of their entries.
//                      The unit list over all such rows is a scan of the rows'
//                      unit counts, a unit finds its row by owner_search
// The tie rule of the merge path is A before B on equal keys, in the count and
// the fill alike (ew_cut is the one place that cuts).  A cut that would part a
// pair a == b -- the A half the last entry before it, the B half the first after
// -- is moved past the B half: both halves belong to the earlier unit, the pair
// is counted there once, and a unit holds at most kEwiseTile + 1 entries.
//
// All indices come from validated operands (dev_sorted_patterns_validate runs
// first); LDS indices are bounded by the classes' caps, which the classify
// kernel applies to the device's own row lengths.  No atomic touches a result:
// the class lists' order is the only thing atomics decide, and no output
// depends on it.
#include <algorithm>
#include <type_traits>

#include "tsg_dev_common.h"
#include "tsg_semiring.h"

namespace tsg {

constexpr int EW_EPT = 9;  // tile class: entries per thread (256 x 9 covers kEwiseTile + 1)
constexpr int EW_LDS = WG * EW_EPT;
static_assert(EW_LDS >= kEwiseTile + 1, "a unit's entries, the moved pair half included, fit the workgroup's shares");
static_assert(kEwisePackedLen == 32, "the packed class: two entries per lane of a 16-lane group");
static_assert(kEwiseWaveLen % 64 == 0, "the wave class steps by whole waves");

struct EwOps {
    const int *rpA, *ciA, *rpB, *ciB;
    int *rp;   // C's row pointers: the rows' lengths before the scan
    int *ci;   // C's columns (fill)
    int mode;  // TSG_EWISE_* (the count kernels: the length that goes with `both`)
};
// the valued fill's: the structural instantiations keep EwOps and see no value pointer
struct EwOpsValued : EwOps {
    const double *va, *vb;
    double *vc;
    double alpha, beta;
};
template <bool VALUED> using EwOpsFor = std::conditional_t<VALUED, EwOpsValued, EwOps>;

// the tile class's units: ubase[i] the first unit of the list's row i (nrows + 1
// values); ucnt[u] the unit's output entries, after the scan those before it
struct EwTile {
    const int *list;
    const int *ubase;
    int nrows;
    long long *ucnt;
};

__device__ __forceinline__ int ew_len(int mode, int la, int lb, int both) {
    return mode == TSG_EWISE_UNION ? la + lb - both : mode == TSG_EWISE_INTERSECT ? both : la - both;
}

// An A entry: x its index among the group's A entries, pb its lower bound among
// the group's B entries, mb the matched A entries before it, out0 the group's
// first output place; ia / jb: its own and the lower bound's index in A's / B's arrays
template <int MODE, class OP, bool VALUED>
__device__ __forceinline__ void ew_emit_a(const EwOpsFor<VALUED> &o, int out0, int x, int pb, bool match, int mb,
                                          int key, int ia, int jb) {
    int p;
    if constexpr (MODE == TSG_EWISE_UNION) {
        p = out0 + x + pb - mb;
    } else if constexpr (MODE == TSG_EWISE_INTERSECT) {
        if (!match) return;
        p = out0 + mb;
    } else {
        if (match) return;
        p = out0 + x - mb;
    }
    o.ci[p] = key;
    if constexpr (VALUED) {
        double v;
        if (MODE != TSG_EWISE_DIFFERENCE && (MODE == TSG_EWISE_INTERSECT || match)) {
            double xa = 0.0, yb = 0.0;
            if constexpr (OP::kReadsA) xa = ew_scale(o.alpha, o.va[ia]);
            if constexpr (OP::kReadsB) yb = ew_scale(o.beta, o.vb[jb]);
            v = OP::apply(xa, yb);
        } else {
            v = ew_scale(o.alpha, o.va[ia]);
        }
        o.vc[p] = v;
    }
}
// a B entry of a union (matched: its A partner has written the pair): y its index
// among the group's B entries, pa its lower bound among the A entries, mb the
// matched B entries before it
template <bool VALUED>
__device__ __forceinline__ void ew_emit_b(const EwOpsFor<VALUED> &o, int out0, int y, int pa, bool match, int mb,
                                          int key, int jb) {
    if (match) return;
    const int p = out0 + y + pa - mb;
    o.ci[p] = key;
    if constexpr (VALUED) o.vc[p] = ew_scale(o.beta, o.vb[jb]);
}

// ---------------------------------------------------------------------------
// setup kernels
// ---------------------------------------------------------------------------
// EW_CPT rows per thread: their lists (one LDS atomic per wave and list, one
// global atomic per workgroup and list, as k_sym_classify); rows without an
// entry get their count (0) here
constexpr int EW_CPT = 8;
__global__ __launch_bounds__(WG) void k_ew_classify(const int *rpA, const int *rpB, int m, int *rp, int *lists,
                                                    int *nlist) {
    __shared__ int s_n[kEwLists], s_base[kEwLists];
    const int lane = lane_id();
    const u64 below = (1ull << lane) - 1ull;
    for (long base = (long)blockIdx.x * WG * EW_CPT; base < m; base += (long)gridDim.x * WG * EW_CPT) {
        if (threadIdx.x < kEwLists) s_n[threadIdx.x] = 0;
        __syncthreads();
        int l[EW_CPT], pos[EW_CPT];
#pragma unroll
        for (int k = 0; k < EW_CPT; ++k) {
            const long row = base + k * WG + threadIdx.x;
            l[k] = -1;
            pos[k] = 0;
            if (row < m) {
                l[k] = ewise_row_list((long long)(rpA[row + 1] - rpA[row]) + (rpB[row + 1] - rpB[row]));
                if (l[k] < 0) rp[row] = 0;
            }
#pragma unroll
            for (int t = 0; t < kEwLists; ++t) {
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
        if (threadIdx.x < kEwLists && s_n[threadIdx.x])
            s_base[threadIdx.x] = atomicAdd(&nlist[threadIdx.x], s_n[threadIdx.x]);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < EW_CPT; ++k)
            if (l[k] >= 0) lists[(long)l[k] * m + s_base[l[k]] + pos[k]] = (int)(base + k * WG + threadIdx.x);
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) rp[m] = 0;
}

// the tile rows' unit counts (nun[nrows] = 0: the scan makes them the rows' first units)
__global__ __launch_bounds__(WG) void k_ew_unit_counts(const int *list, int nrows, const int *rpA, const int *rpB,
                                                       int *nun) {
    for (long i = (long)blockIdx.x * WG + threadIdx.x; i <= nrows; i += (long)gridDim.x * WG) {
        int v = 0;
        if (i < nrows) {
            const int row = list[i];
            const long long len = (long long)(rpA[row + 1] - rpA[row]) + (rpB[row + 1] - rpB[row]);
            v = (int)((len + kEwiseTile - 1) / kEwiseTile);
        }
        nun[i] = v;
    }
}

// a tile row's length: its units' entries (uoff: the scanned unit counts)
__global__ __launch_bounds__(WG) void k_ew_tile_rows(EwTile t, int *rp) {
    for (long i = (long)blockIdx.x * WG + threadIdx.x; i < t.nrows; i += (long)gridDim.x * WG)
        rp[t.list[i]] = (int)(t.ucnt[t.ubase[i + 1]] - t.ucnt[t.ubase[i]]);
}

// ---------------------------------------------------------------------------
// packed class
// ---------------------------------------------------------------------------
template <bool FILL, int MODE, class OP, bool VALUED>
__global__ __launch_bounds__(WG) void k_ew_packed(const int *list, int nrows, EwOpsFor<VALUED> o) {
    constexpr int LN = 16;
    constexpr bool BSIDE = FILL && MODE == TSG_EWISE_UNION;  // (else the A entries alone are walked)
    const int g = threadIdx.x / LN, l = threadIdx.x % LN;
    const long li = (long)blockIdx.x * (WG / LN) + g;
    const bool have = li < nrows;
    const int row = have ? list[li] : 0;
    const int a0 = have ? o.rpA[row] : 0, la = have ? o.rpA[row + 1] - a0 : 0;
    const int b0 = have ? o.rpB[row] : 0, lb = have ? o.rpB[row + 1] - b0 : 0;
    const int sh = (lane_id() / LN) * LN;  // the group's first lane in its wave
    // the row's entries e = l and l + 16: its A entries, then its B entries (la + lb <= 32)
    int key[2], pos[2];
    bool match[2];
    u32 mm = 0;  // the entries' match flags, by e
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int e = l + h * LN;
        key[h] = 0, pos[h] = 0, match[h] = false;
        if (e < la) {
            key[h] = o.ciA[a0 + e];
            pos[h] = lower_bound_dev(o.ciB, b0, b0 + lb, key[h]) - b0;
            match[h] = pos[h] < lb && o.ciB[b0 + pos[h]] == key[h];
        } else if (BSIDE && e < la + lb) {
            key[h] = o.ciB[b0 + e - la];
            pos[h] = lower_bound_dev(o.ciA, a0, a0 + la, key[h]) - a0;
            match[h] = pos[h] < la && o.ciA[a0 + pos[h]] == key[h];
        }
        mm |= (u32)((__ballot(match[h]) >> sh) & 0xffffull) << (h * LN);
    }
    const u32 amask = (u32)((1ull << la) - 1ull);  // the A entries' bits
    if constexpr (!FILL) {
        if (have && l == 0) o.rp[row] = ew_len(o.mode, la, lb, __popc(mm & amask));
    } else {
        const int c0 = have ? o.rp[row] : 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int e = l + h * LN;
            const u32 below = (u32)((1ull << e) - 1ull);
            if (e < la)
                ew_emit_a<MODE, OP, VALUED>(o, c0, e, pos[h], match[h], __popc(mm & below), key[h], a0 + e,
                                            b0 + pos[h]);
            else if (BSIDE && e < la + lb)
                ew_emit_b<VALUED>(o, c0, e - la, pos[h], match[h], __popc(mm & below & ~amask), key[h], b0 + e - la);
        }
    }
}

// ---------------------------------------------------------------------------
// wave class
// ---------------------------------------------------------------------------
template <bool FILL, int MODE, class OP, bool VALUED>
__global__ __launch_bounds__(WG) void k_ew_wave(const int *list, int nrows, EwOpsFor<VALUED> o) {
    constexpr bool BSIDE = FILL && MODE == TSG_EWISE_UNION;
    __shared__ int s_key[WAVES][kEwiseWaveLen];
    const int lane = lane_id();
    const long li = (long)blockIdx.x * WAVES + wave_id();
    if (li >= nrows) return;  // (wave-uniform; the kernel has no workgroup barrier)
    const int row = list[li];
    const int a0 = o.rpA[row], la = o.rpA[row + 1] - a0;
    const int b0 = o.rpB[row], lb = o.rpB[row + 1] - b0;  // (la + lb <= kEwiseWaveLen: the row's class)
    int *sa = s_key[wave_id()], *sb = sa + la;
    for (int q = lane; q < la; q += 64) sa[q] = o.ciA[a0 + q];
    for (int q = lane; q < lb; q += 64) sb[q] = o.ciB[b0 + q];
    wave_lds_sync();
    const u64 below = (1ull << lane) - 1ull;
    const int ne = BSIDE ? la + lb : la;
    const int c0 = FILL ? o.rp[row] : 0;
    int ma = 0, mb = 0;  // the matched A / B entries of the earlier steps
    for (int e0 = 0; e0 < ne; e0 += 64) {  // (wave-uniform trips: the ballots see whole waves)
        const int e = e0 + lane;
        int key = 0, pos = 0;
        bool match = false;
        if (e < la) {
            key = sa[e];
            pos = lower_bound_dev(sb, 0, lb, key);
            match = pos < lb && sb[pos] == key;
        } else if (BSIDE && e < ne) {
            key = sb[e - la];
            pos = lower_bound_dev(sa, 0, la, key);
            match = pos < la && sa[pos] == key;
        }
        const u64 mm = __ballot(match), am = __ballot(e < la);
        if constexpr (FILL) {
            if (e < la)
                ew_emit_a<MODE, OP, VALUED>(o, c0, e, pos, match, ma + __popcll(mm & am & below), key, a0 + e,
                                            b0 + pos);
            else if (BSIDE && e < ne)
                ew_emit_b<VALUED>(o, c0, e - la, pos, match, mb + __popcll(mm & ~am & below), key, b0 + e - la);
        }
        ma += __popcll(mm & am);
        mb += __popcll(mm & ~am);
    }
    if constexpr (!FILL)
        if (lane == 0) o.rp[row] = ew_len(o.mode, la, lb, ma);
}

// ---------------------------------------------------------------------------
// tile class
// ---------------------------------------------------------------------------
// The merge path's cut of a[0, la) and b[0, lb) (strictly ascending each) at
// diagonal d, A before B on equal keys: (i, j) with i A entries and j B entries
// before the cut, i + j = d -- unless the cut would part a pair, a[i - 1] == b[j]:
// then b[j] goes before the cut too (i + j = d + 1).  Cuts stay monotone: the
// next diagonal's cut has passed b[j] anyway (it precedes a[i] in the merge).
__device__ __forceinline__ int2 ew_cut(const int *a, int la, const int *b, int lb, long long d) {
    if (d >= (long long)la + lb) return make_int2(la, lb);
    int lo = (int)max(0ll, d - lb), hi = (int)min(d, (long long)la);
    while (lo < hi) {  // the A entries among the first d: a[mid] is one iff a[mid] <= b[d - 1 - mid]
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= b[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    int j = (int)(d - lo);
    if (lo > 0 && j < lb && a[lo - 1] == b[j]) ++j;
    return make_int2(lo, j);
}

// a workgroup per unit (blockIdx.x + u0 of the unit list)
template <bool FILL, int MODE, class OP, bool VALUED>
__global__ __launch_bounds__(WG) void k_ew_tile(EwTile t, int u0, EwOpsFor<VALUED> o) {
    constexpr bool BSIDE = FILL && MODE == TSG_EWISE_UNION;
    __shared__ int s_key[EW_LDS];
    __shared__ int s_cut[4];
    __shared__ int s_red[WAVES];
    const int tid = threadIdx.x;
    const int u = u0 + blockIdx.x;
    const int k = owner_search(t.ubase, t.nrows, u);  // (every row of the list has a unit: ubase strictly ascends)
    const int row = t.list[k], ut = u - t.ubase[k];
    const int a0 = o.rpA[row], la = o.rpA[row + 1] - a0;
    const int b0 = o.rpB[row], lb = o.rpB[row + 1] - b0;
    if (tid < 2) {  // the unit's two cuts (the last unit's second: the rows' ends)
        const int2 c = ew_cut(o.ciA + a0, la, o.ciB + b0, lb, (long long)(ut + tid) * kEwiseTile);
        s_cut[2 * tid] = c.x;
        s_cut[2 * tid + 1] = c.y;
    }
    __syncthreads();
    const int i0 = s_cut[0], j0 = s_cut[1];
    const int na = min(s_cut[2] - i0, EW_LDS);       // (na + nb <= kEwiseTile + 1 by the cuts; the bounds only
    const int nb = min(s_cut[3] - j0, EW_LDS - na);  //  keep a malformed unit inside the LDS array)
    int *sa = s_key, *sb = s_key + na;
    for (int q = tid; q < na; q += WG) sa[q] = o.ciA[a0 + i0 + q];
    for (int q = tid; q < nb; q += WG) sb[q] = o.ciB[b0 + j0 + q];
    __syncthreads();
    // the thread's EW_EPT entries of the unit's A entries followed by its B entries
    const int ne = BSIDE ? na + nb : na;
    int pos[EW_EPT];
    u32 mbits = 0;
    int ca = 0, cb = 0;  // the thread's matched A / B entries
#pragma unroll
    for (int q = 0; q < EW_EPT; ++q) {
        const int e = tid * EW_EPT + q;
        pos[q] = 0;
        bool match = false;
        if (e < na) {
            const int key = sa[e];
            pos[q] = lower_bound_dev(sb, 0, nb, key);
            match = pos[q] < nb && sb[pos[q]] == key;
            ca += match ? 1 : 0;
        } else if (BSIDE && e < ne) {
            const int key = sb[e - na];
            pos[q] = lower_bound_dev(sa, 0, na, key);
            match = pos[q] < na && sa[pos[q]] == key;
            cb += match ? 1 : 0;
        }
        mbits |= (match ? 1u : 0u) << q;
    }
    if constexpr (!FILL) {
        const int both = block_sum(ca, s_red);
        if (tid == 0) t.ucnt[u] = ew_len(o.mode, na, nb, both);
    } else {
        // the matched entries before the thread's, per side, in one scan (each side's total fits 16 bits)
        int tot;
        const int off = block_excl_scan(ca | (cb << 16), &tot, s_red);
        int ma = off & 0xffff, mb = off >> 16;
        const int out0 = o.rp[row] + (int)(t.ucnt[u] - t.ucnt[t.ubase[k]]);
#pragma unroll
        for (int q = 0; q < EW_EPT; ++q) {
            const int e = tid * EW_EPT + q;
            const bool match = (mbits >> q) & 1u;
            if (e < na) {
                ew_emit_a<MODE, OP, VALUED>(o, out0, e, pos[q], match, ma, sa[e], a0 + i0 + e, b0 + j0 + pos[q]);
                ma += match ? 1 : 0;
            } else if (BSIDE && e < ne) {
                ew_emit_b<VALUED>(o, out0, e - na, pos[q], match, mb, sb[e - na], b0 + j0 + e - na);
                mb += match ? 1 : 0;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
bool ewise_mode_known(int mode) { return mode >= TSG_EWISE_UNION && mode <= TSG_EWISE_DIFFERENCE; }
bool binop_known(int op) { return op >= TSG_BINOP_PLUS && op <= TSG_BINOP_SECOND; }
bool ewise_reads_b_values(int mode, int op) {
    return mode == TSG_EWISE_UNION || (mode == TSG_EWISE_INTERSECT && op != TSG_BINOP_FIRST);
}

// the three classes' launch lists and the tile class's units
struct EwLaunch {
    const int *lists;
    int m;
    int cnt[kEwLists];
    EwTile tile;
    int nunits;
};

// one pass over the partition: the count (FILL false; MODE, OP, VALUED unused) or a fill
template <bool FILL, int MODE, class OP, bool VALUED>
static int ew_pass(const EwLaunch &L, const EwOpsFor<VALUED> &o, hipStream_t s) {
    // (the long rows first: their tails overlap the short rows' kernels)
    for (int u0 = 0; u0 < L.nunits; u0 += kMaxGridBlocks)
        k_ew_tile<FILL, MODE, OP, VALUED><<<std::min(L.nunits - u0, kMaxGridBlocks), WG, 0, s>>>(L.tile, u0, o);
    const auto rows_launch = [&](int l, int per, auto &&launch) {
        const long step = (long)kMaxGridBlocks * per;
        for (long r0 = 0; r0 < L.cnt[l]; r0 += step)
            launch(L.lists + (size_t)l * L.m + r0, (int)std::min(step, L.cnt[l] - r0));
    };
    rows_launch(kEwListWave, WAVES, [&](const int *l, int c) {
        k_ew_wave<FILL, MODE, OP, VALUED><<<(c + WAVES - 1) / WAVES, WG, 0, s>>>(l, c, o);
    });
    rows_launch(kEwListPacked, 16, [&](const int *l, int c) {
        k_ew_packed<FILL, MODE, OP, VALUED><<<(c + 15) / 16, WG, 0, s>>>(l, c, o);
    });
    TSG_HIP(hipGetLastError());
    return TSG_OK;
}

template <class OP> static int ew_fill_valued(int mode, const EwLaunch &L, const EwOpsValued &o, hipStream_t s) {
    return mode == TSG_EWISE_UNION ? ew_pass<true, TSG_EWISE_UNION, OP, true>(L, o, s)
                                   : ew_pass<true, TSG_EWISE_INTERSECT, OP, true>(L, o, s);
}

int dev_ewise(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, int mode, int op, double alpha, double beta,
              tsg_dev_csr &C, tsg_ewise_info &info, hipStream_t s, hipEvent_t *ev) {
    C = tsg_dev_csr{};
    info = tsg_ewise_info{};
    if (!ewise_mode_known(mode) || !binop_known(op)) return TSG_ERR_INVALID;
    if (A.m != B.m || A.n != B.n) return TSG_ERR_INVALID;
    const bool valued = A.value != nullptr;
    if (valued && B.nnz > 0 && !B.value && ewise_reads_b_values(mode, op)) return TSG_ERR_INVALID;
    const tsg_dev_csr *mats[2] = {&A, &B};
    TSG_TRY(dev_sorted_patterns_validate(cx, mats, 2, s));
    info.nnzA = A.nnz;
    info.nnzB = B.nnz;
    const int m = A.m, n = A.n;
    PoolScope ws(cx);  // (temporaries and half-built outputs: back to the pool on every way out)
    int *rp = nullptr;
    TSG_TRY(ws.get(&rp, (size_t)m + 1));
    for (int e = 4; e < 8; ++e) TSG_HIP(hipEventRecord(ev[e], s));  // (an early way out leaves valid brackets)
    if (m == 0 || (A.nnz == 0 && B.nnz == 0)) {
        TSG_HIP(hipMemsetAsync(rp, 0, ((size_t)m + 1) * sizeof(int), s));
        TSG_TRY(stream_wait(s));
        C = tsg_dev_csr{m, n, 0, ws.keep(rp), nullptr, nullptr};
        return TSG_OK;
    }
    // 1. the classes (host round trip 1: the lists' sizes)
    int *lists = nullptr, *nlist = nullptr;
    TSG_TRY(ws.get(&lists, (size_t)kEwLists * m));
    TSG_TRY(ws.get(&nlist, 4));
    TSG_HIP(hipMemsetAsync(nlist, 0, 4 * sizeof(int), s));
    k_ew_classify<<<grid_for(m, WG * EW_CPT, 16384), WG, 0, s>>>(A.rowpointer, B.rowpointer, m, rp, lists, nlist);
    TSG_HIP(hipGetLastError());
    TSG_HIP(hipMemcpyAsync(cx.slots->ew_nlist, nlist, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    TSG_TRY(stream_wait(s));
    EwLaunch L{};
    L.lists = lists;
    L.m = m;
    for (int l = 0; l < kEwLists; ++l) info.rows_class[l] = L.cnt[l] = cx.slots->ew_nlist[l];
    // 2. the tile rows' units (a round trip of its own, only where there are such rows)
    const int ntile = L.cnt[kEwListTile];
    if (ntile) {
        int *nun = nullptr;
        long long *ucnt = nullptr, units = 0;
        TSG_TRY(ws.get(&nun, (size_t)ntile + 1));
        k_ew_unit_counts<<<grid_for((long)ntile + 1, WG, 2048), WG, 0, s>>>(lists + (size_t)kEwListTile * m, ntile,
                                                                          A.rowpointer, B.rowpointer, nun);
        TSG_HIP(hipGetLastError());
        TSG_TRY(scan_exclusive_i32_total(cx, nun, (long)ntile + 1, s, &units));
        info.units = units;  // (nnzA + nnzB < 2^32 bounds them far below int32)
        TSG_TRY(ws.get(&ucnt, (size_t)units + 1));
        L.tile = EwTile{lists + (size_t)kEwListTile * m, nun, ntile, ucnt};
        L.nunits = (int)units;
    }
    // 3. count
    EwOps o{A.rowpointer, A.columnindex, B.rowpointer, B.columnindex, rp, nullptr, mode};
    TSG_HIP(hipEventRecord(ev[4], s));
    TSG_TRY((ew_pass<false, TSG_EWISE_UNION, EwFirst, false>(L, o, s)));
    if (L.nunits) {  // the units' counts -> the entries before each unit, the tile rows' lengths
        TSG_HIP(hipMemsetAsync(L.tile.ucnt + L.nunits, 0, sizeof(long long), s));
        TSG_TRY(dev_scan_i64(cx, L.tile.ucnt, (long)L.nunits + 1, s));
        k_ew_tile_rows<<<grid_for(ntile, WG, 2048), WG, 0, s>>>(L.tile, rp);
        TSG_HIP(hipGetLastError());
    }
    TSG_HIP(hipEventRecord(ev[5], s));
    TSG_HIP(hipEventRecord(ev[6], s));
    TSG_HIP(hipEventRecord(ev[7], s));
    // 4. the row pointers; nnz(C) in 64 bits before anything is sized by it (host round trip 2)
    long long total = 0;
    const int rc = scan_exclusive_i32_total(cx, rp, (long)m + 1, s, &total);
    info.nnzC = total;
    info.both = mode == TSG_EWISE_UNION ? info.nnzA + info.nnzB - total : mode == TSG_EWISE_INTERSECT ? total
                                                                                                  : info.nnzA - total;
    TSG_TRY(rc);
    if (total == 0) {
        C = tsg_dev_csr{m, n, 0, ws.keep(rp), nullptr, nullptr};
        return TSG_OK;
    }
    // 5. fill: every column and value once, at its final place
    int *ci = nullptr;
    double *vc = nullptr;
    TSG_TRY(ws.get(&ci, (size_t)total));
    if (valued) TSG_TRY(ws.get(&vc, (size_t)total));
    o.ci = ci;
    TSG_HIP(hipEventRecord(ev[6], s));
    if (!valued) {
        TSG_TRY(mode == TSG_EWISE_UNION       ? (ew_pass<true, TSG_EWISE_UNION, EwFirst, false>(L, o, s))
                : mode == TSG_EWISE_INTERSECT ? (ew_pass<true, TSG_EWISE_INTERSECT, EwFirst, false>(L, o, s))
                                              : (ew_pass<true, TSG_EWISE_DIFFERENCE, EwFirst, false>(L, o, s)));
    } else {
        EwOpsValued ov{};
        static_cast<EwOps &>(ov) = o;
        ov.va = A.value, ov.vb = B.value, ov.vc = vc, ov.alpha = alpha, ov.beta = beta;
        if (mode == TSG_EWISE_DIFFERENCE)
            TSG_TRY((ew_pass<true, TSG_EWISE_DIFFERENCE, EwFirst, true>(L, ov, s)));
        else
            TSG_TRY(binop_dispatch(op, [&](auto opt) { return ew_fill_valued<decltype(opt)>(mode, L, ov, s); }));
    }
    TSG_HIP(hipEventRecord(ev[7], s));
    TSG_TRY(stream_wait(s));
    C = tsg_dev_csr{m, n, (int)total, ws.keep(rp), ws.keep(ci), valued ? ws.keep(vc) : nullptr};
    return TSG_OK;
}

}  // namespace tsg
