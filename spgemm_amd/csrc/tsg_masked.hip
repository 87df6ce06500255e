// tsg_masked.hip -- masked SpGEMM C<M> = A*B on the mask's pattern only (gfx950,
// wave64).
//
// c_val[p] := sum_k A(i,k) * B(k,j) for every entry p = (i, j) of a structural
// mask M, 0.0 where no product reaches; products on other columns are dropped.
// Each row with mask entries runs on one of two legs, chosen at plan time:
//   row-wise  the numeric plan's kernels (tsg_numeric.hip) over the mask as the C
//             pattern: every element product of the row is walked and looked up
//             in the mask row; a miss is counted there and ignored here
//   dot       per mask entry (i, j) the intersection of A's row i with B^T's row
//             j: 16 lanes stride the shorter list and search each of its columns
//             in the longer one, multiply on a hit, and sum over the lanes
// The row-wise leg costs P_i (the row's element products) lookups, the dot leg
// D_i = sum over the row's mask entries of min(len A_i, len B^T_j) searches;
// AUTO takes the dot leg when kMskDotCost * D_i < P_i.  The dot leg needs A's
// rows strictly ascending and B free of a repeated (row, column) -- B^T's rows
// strictly ascending; otherwise every row is row-wise (that leg takes unsorted
// and repeating B rows as the numeric plan does).
//
// The plan holds B^T's pattern (built once: rows ascending, the transpose is
// stable) and each of its entries' position in B; a run gathers b_val into
// B^T's order first, so the dot loop reads values next to their columns.  The
// dot leg's work is cut into units of (row, a range of its mask entries) of at
// most kMskUnitWork searches and kMskUnitEntries entries; a workgroup runs one
// unit, A's row in LDS when it has at most kMskRowLds entries.
//
// The dot leg uses no atomics and does not need c_val zeroed: every mask entry
// is summed by one 16-lane group in an order the patterns fix (lane l takes the
// shorter list's entries l, l + 16, ... in turn, then the lanes' sums are added
// in a fixed tree), so its values are bit-reproducible from run to run.  The
// two legs write disjoint rows.  DESIGN.md section 3.8.
//
// The arithmetic is a semiring's (tsg_semiring.h): the
// dot kernel is templated on its traits -- "multiply" above is mul, "sum" its
// (+) from its identity, which is also what an entry no product reaches holds
// -- and dev_masked_run picks the instantiation of both legs.
#include <algorithm>
#include <vector>

#include "tsg_dev_common.h"
#include "tsg_semiring.h"

namespace tsg {

// ---------------------------------------------------------------------------
// plan-time kernels (validated patterns only)
// ---------------------------------------------------------------------------
// B^T's pattern with each entry's position in B: column histogram -> scan ->
// unordered scatter of (row << 32 | position) -> per-column sort (dev_transpose's
// steps; the keys' order is B's row order, so B^T's rows ascend and a repeated
// (row, column) of B shows as an equal neighbour)
__global__ __launch_bounds__(WG) void k_msk_colcount(const int *col, int nnz, int *cnt) {
    for (long p = (long)blockIdx.x * WG + threadIdx.x; p < nnz; p += (long)gridDim.x * WG) atomicAdd(&cnt[col[p]], 1);
}
__global__ __launch_bounds__(WG) void k_msk_scatter(const int *rp, const int *col, int m, const int *colptr,
                                                    int *fill, u64 *keys) {
    for (long r = (long)blockIdx.x * WAVES + wave_id(); r < m; r += (long)gridDim.x * WAVES) {
        const int p1 = rp[r + 1];
        for (int p = rp[r] + lane_id(); p < p1; p += 64) {
            const int c = col[p];
            keys[colptr[c] + atomicAdd(&fill[c], 1)] = ((u64)(u32)r << 32) | (u32)p;
        }
    }
}
__global__ __launch_bounds__(WG) void k_msk_tfinish(const u64 *keys, int nnz, int *rowidx, int *pos) {
    for (long q = (long)blockIdx.x * WG + threadIdx.x; q < nnz; q += (long)gridDim.x * WG) {
        const u64 k = keys[q];
        rowidx[q] = (int)(k >> 32);
        pos[q] = (int)(u32)k;
    }
}

// per row: its element products P and its dot work D = sum over its mask
// entries of min(len A_i, len B^T_j) (a wave per row; k_num_rowstats' sibling)
__global__ __launch_bounds__(WG) void k_msk_rowstats(const int *rpA, const int *ciA, const int *rpB, const int *rpM,
                                                     const int *ciM, const int *rpT, int m, long long *P,
                                                     long long *D) {
    for (long row = (long)blockIdx.x * WAVES + wave_id(); row < m; row += (long)gridDim.x * WAVES) {
        long long s = 0, d = 0;
        const int e0 = rpA[row], e1 = rpA[row + 1], q1 = rpM[row + 1];
        for (int e = e0 + lane_id(); e < e1; e += 64) {
            const int k = ciA[e];
            s += rpB[k + 1] - rpB[k];
        }
        for (int q = rpM[row] + lane_id(); q < q1; q += 64) {
            const int j = ciM[q];
            d += min(e1 - e0, rpT[j + 1] - rpT[j]);
        }
        s = wave_sum(s);
        d = wave_sum(d);
        if (lane_id() == 0) {
            P[row] = s;
            D[row] = d;
        }
    }
}

// The dot rows' units (a wave per row): the row's mask entries in order, a unit
// closed before the entry that would take its work past kMskUnitWork or its
// entries past kMskUnitEntries (so an entry heavier than kMskUnitWork is alone).
// The entries' work is loaded 64 at a time, the cuts walk it lane by lane.
// EMIT false: count[r] := the row's units; true: written from uoff[r] on.
template <bool EMIT>
__global__ __launch_bounds__(WG) void k_msk_cut(const int *rows, int nrows, const int *rpA, const int *rpM,
                                                const int *ciM, const int *rpT, int *count, const int *uoff,
                                                int4 *units) {
    for (long r = (long)blockIdx.x * WAVES + wave_id(); r < nrows; r += (long)gridDim.x * WAVES) {
        const int row = rows[r];
        const int la = rpA[row + 1] - rpA[row], q0 = rpM[row], q1 = rpM[row + 1];
        const int out = EMIT ? uoff[r] : 0;
        int first = q0, cnt = 0, nu = 0;
        long long cur = 0;
        for (int base = q0; base < q1; base += 64) {  // wave-uniform
            int w = 0;
            if (base + lane_id() < q1) {
                const int j = ciM[base + lane_id()];
                w = min(la, rpT[j + 1] - rpT[j]);
            }
            const int nv = min(64, q1 - base);
            for (int t = 0; t < nv; ++t) {
                const int wt = __builtin_amdgcn_readlane(w, t);
                if (cnt > 0 && (cur + wt > kMskUnitWork || cnt == kMskUnitEntries)) {
                    if (EMIT && lane_id() == 0) units[out + nu] = make_int4(row, first, cnt, 0);
                    ++nu;
                    first = base + t;
                    cnt = 0;
                    cur = 0;
                }
                ++cnt;
                cur += wt;
            }
        }
        if (cnt > 0) {
            if (EMIT && lane_id() == 0) units[out + nu] = make_int4(row, first, cnt, 0);
            ++nu;
        }
        if (!EMIT && lane_id() == 0) count[r] = nu;
    }
}

// ---------------------------------------------------------------------------
// run-time kernels
// ---------------------------------------------------------------------------
// bt_val := b_val in B^T's order
__global__ __launch_bounds__(WG) void k_msk_gather(const int *pos, int nnz, const double *b_val, double *bt_val) {
    for (long q = (long)blockIdx.x * WG + threadIdx.x; q < nnz; q += (long)gridDim.x * WG) bt_val[q] = b_val[pos[q]];
}

struct MskOps {
    const int *rpA, *ciA, *rpM, *ciM, *rpT, *ciT;
    const double *a_val, *t_val;
    double *c_val;
};

constexpr int MSK_G = 16;   // lanes per mask entry: one DPP row
constexpr int MSK_ILP = 4;  // searches per lane in flight

// inclusive (+)-sum over a 16-lane DPP row (for_products' row steps, on both
// halves of the double): the row's last lane ends with the sum of all 16, always
// combined in the same order.  The row is wholly active or not at all.  A lane
// without a source takes the DPP move's old value: the bits of the semiring's
// identity (all zero for +; a zero there would win a min over positive values
// or a max over negative ones in lane 0 at the first step and reach lane 15,
// the lane that stores, by the last).
template <class SR, int CTRL> __device__ __forceinline__ double row_shr_comb(double x) {
    const double id = SR::identity();
    const int lo = dpp_mov<CTRL, 0xf>(__double2loint(id), __double2loint(x)),
              hi = dpp_mov<CTRL, 0xf>(__double2hiint(id), __double2hiint(x));
    return SR::add(x, __hiloint2double(hi, lo));
}
template <class SR> __device__ __forceinline__ double row16_incl_sum(double x) {
    x = row_shr_comb<SR, 0x111>(x);  // row_shr:1
    x = row_shr_comb<SR, 0x112>(x);  // row_shr:2
    x = row_shr_comb<SR, 0x114>(x);  // row_shr:4
    x = row_shr_comb<SR, 0x118>(x);  // row_shr:8
    return x;
}

// Lane l's share of the (+)-sum over the columns common to a short list (ks, vs:
// ns entries) and a long one (kl, vl: nl >= ns entries, strictly ascending),
// from the semiring's identity.  The
// group strides the short list MSK_ILP * 16 entries at a time; each key is
// searched in the long list by a bounded branchless search whose trip count
// depends on nl alone (uniform over the group: the MSK_ILP searches interleave)
// and whose every read lies in [0, nl).  A lane past the short list's end
// searches INT_MAX, which no column equals.  A semiring that reads no values
// touches neither vs nor vl.  (Every (x) here commutes: which list is A's does
// not matter.)
template <class SR>
__device__ __forceinline__ double msk_intersect(const int *ks, const double *vs, int ns, const int *kl,
                                                const double *vl, int nl, int l) {
    double acc = SR::identity();
    for (int b = 0; b < ns; b += MSK_ILP * MSK_G) {  // (ns > 0 here, so nl > 0)
        int k[MSK_ILP], key[MSK_ILP], base[MSK_ILP];
#pragma unroll
        for (int u = 0; u < MSK_ILP; ++u) {
            k[u] = b + u * MSK_G + l;
            key[u] = k[u] < ns ? ks[k[u]] : INT_MAX;
            base[u] = 0;
        }
        int len = nl;
        while (len > 1) {  // the last index with kl[index] <= key, if the key is there
            const int half = len >> 1;
#pragma unroll
            for (int u = 0; u < MSK_ILP; ++u) base[u] = kl[base[u] + half] <= key[u] ? base[u] + half : base[u];
            len -= half;
        }
#pragma unroll
        for (int u = 0; u < MSK_ILP; ++u)
            if (kl[base[u]] == key[u]) acc = SR::add(acc, SR::mul(sr_load<SR>(vs, k[u]), sr_load<SR>(vl, base[u])));
    }
    return acc;
}

// one dot unit per workgroup: (row, first mask entry, entries, -).  The 16
// groups of 16 lanes take the unit's mask entries round-robin; the group's last
// lane stores the entry's value once (the identity where the lists share no
// column, an empty A row included).
template <class SR>
__global__ __launch_bounds__(WG) void k_msk_dot(const int4 *units, MskOps o) {
    __shared__ int s_col[kMskRowLds];
    __shared__ double s_val[kMskRowLds];
    const int4 u = units[blockIdx.x];
    const int a0 = o.rpA[u.x], la = o.rpA[u.x + 1] - a0;
    const bool lds = la <= kMskRowLds;  // (workgroup-uniform)
    if (lds) {
        for (int q = threadIdx.x; q < la; q += WG) {
            s_col[q] = o.ciA[a0 + q];
            if constexpr (SR::kValues) s_val[q] = o.a_val[a0 + q];
        }
        __syncthreads();
    }
    const int g = threadIdx.x / MSK_G, l = threadIdx.x % MSK_G;
    for (int x = g; x < u.z; x += WG / MSK_G) {  // (uniform over the group)
        const int p = u.y + x;
        const int j = o.ciM[p];
        const int t0 = o.rpT[j], lt = o.rpT[j + 1] - t0;
        const int *ct = o.ciT + t0;
        const double *vt = o.t_val + t0;
        double acc;
        if (lds)
            acc = la <= lt ? msk_intersect<SR>(s_col, s_val, la, ct, vt, lt, l)
                           : msk_intersect<SR>(ct, vt, lt, s_col, s_val, la, l);
        else
            acc = la <= lt ? msk_intersect<SR>(o.ciA + a0, o.a_val + a0, la, ct, vt, lt, l)
                           : msk_intersect<SR>(ct, vt, lt, o.ciA + a0, o.a_val + a0, la, l);
        acc = row16_incl_sum<SR>(acc);
        if (l == MSK_G - 1) o.c_val[p] = acc;
    }
}

// ---------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------
void dev_masked_plan_free(MaskedPlan &p) {
    dev_numeric_plan_free(p.rows);
    if (p.block) (void)hipFree(p.block);
    p.block = nullptr;
    p.nunits = 0;
}

static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

static int masked_plan_build(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, const tsg_dev_csr &M, int mode,
                             MaskedPlan &p, hipStream_t s) {
    if (mode != TSG_MASKED_AUTO && mode != TSG_MASKED_ROWS && mode != TSG_MASKED_DOT) return TSG_ERR_INVALID;
    // 1. the numeric plan's validation, before anything indexes with the patterns
    bool bsorted = false, asorted = false, tsorted = false;
    TSG_TRY(dev_numeric_validate(cx, A, B, M, &bsorted, s));
    TSG_TRY(dev_rows_sorted(cx, A, &asorted, s));
    const int m = A.m, nt = B.n;
    PoolScope ws(cx);  // (the temporaries: returned to the pool on every way out)
    // 2. B^T's pattern and its entries' positions in B
    tsg_dev_csr T{};
    T.m = nt;
    T.n = B.m;
    T.nnz = B.nnz;
    int *fill = nullptr, *tpos = nullptr;
    u64 *keys = nullptr;
    TSG_TRY(ws.get(&T.rowpointer, (size_t)nt + 1));
    TSG_TRY(ws.get(&T.columnindex, (size_t)B.nnz + 1));
    TSG_TRY(ws.get(&tpos, (size_t)B.nnz + 1));
    TSG_TRY(ws.get(&fill, (size_t)nt + 1));
    TSG_TRY(ws.get(&keys, (size_t)B.nnz + 1));
    TSG_HIP(hipMemsetAsync(T.rowpointer, 0, ((size_t)nt + 1) * sizeof(int), s));
    TSG_HIP(hipMemsetAsync(fill, 0, ((size_t)nt + 1) * sizeof(int), s));
    if (B.nnz) k_msk_colcount<<<grid_for(B.nnz, WG * 4, 8192), WG, 0, s>>>(B.columnindex, B.nnz, T.rowpointer);
    TSG_HIP(hipGetLastError());
    TSG_TRY(scan_exclusive_i32(cx, T.rowpointer, (long)nt + 1, s));
    if (B.nnz)
        k_msk_scatter<<<grid_for(B.m, WAVES, 8192), WG, 0, s>>>(B.rowpointer, B.columnindex, B.m, T.rowpointer, fill,
                                                                keys);
    TSG_HIP(hipGetLastError());
    TSG_TRY(segmented_sort_u64(cx, keys, T.rowpointer, nt, B.nnz, s));
    if (B.nnz) k_msk_tfinish<<<grid_for(B.nnz, WG * 4, 8192), WG, 0, s>>>(keys, B.nnz, T.columnindex, tpos);
    TSG_HIP(hipGetLastError());
    ws.put(fill);
    ws.put(keys);
    TSG_TRY(dev_rows_sorted(cx, T, &tsorted, s));
    const bool eligible = asorted && tsorted;
    if (mode == TSG_MASKED_DOT && !eligible) return TSG_ERR_INVALID;
    // 3. per row: products, dot work; the legs
    std::vector<long long> hP((size_t)m), hD((size_t)m);
    std::vector<int> rpM((size_t)m + 1);
    if (m) {
        long long *P = nullptr, *D = nullptr;
        TSG_TRY(ws.get(&P, (size_t)m));
        TSG_TRY(ws.get(&D, (size_t)m));
        k_msk_rowstats<<<grid_for(m, WAVES, 4096), WG, 0, s>>>(A.rowpointer, A.columnindex, B.rowpointer,
                                                              M.rowpointer, M.columnindex, T.rowpointer, m, P, D);
        TSG_HIP(hipGetLastError());
        TSG_HIP(hipMemcpyAsync(hP.data(), P, (size_t)m * sizeof(long long), hipMemcpyDeviceToHost, s));
        TSG_HIP(hipMemcpyAsync(hD.data(), D, (size_t)m * sizeof(long long), hipMemcpyDeviceToHost, s));
    }
    TSG_HIP(hipMemcpyAsync(rpM.data(), M.rowpointer, ((size_t)m + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
    TSG_TRY(stream_wait(s));
    tsg_masked_info info{};
    info.nnzM = M.nnz;
    info.a_rows_sorted = asorted;
    info.b_rows_sorted = bsorted;
    info.b_no_repeats = tsorted;
    info.dot_eligible = eligible;
    std::vector<unsigned char> skip((size_t)m + 1, 0);
    std::vector<int> dotrows;
    for (int i = 0; i < m; ++i) {
        info.products += hP[i];
        if (rpM[i + 1] == rpM[i]) {  // nothing to write: neither leg
            skip[i] = 1;
            continue;
        }
        const bool dot = mode == TSG_MASKED_DOT || (mode == TSG_MASKED_AUTO && eligible && kMskDotCost * hD[i] < hP[i]);
        if (dot) {
            skip[i] = 1;
            dotrows.push_back(i);
            ++info.rows_dot;
            info.dot_work += hD[i];
        } else {
            ++info.rows_rowwise;
            info.products_rowwise += hP[i];
        }
    }
    // 4. the dot leg: units counted and cut on the device, the plan's own block
    const int nd = (int)dotrows.size();
    if (nd) {
        int *drows = nullptr, *dcnt = nullptr;
        TSG_TRY(ws.get(&drows, (size_t)nd));
        TSG_TRY(ws.get(&dcnt, (size_t)nd));
        TSG_HIP(hipMemcpyAsync(drows, dotrows.data(), (size_t)nd * sizeof(int), hipMemcpyHostToDevice, s));
        k_msk_cut<false><<<grid_for(nd, WAVES, 4096), WG, 0, s>>>(drows, nd, A.rowpointer, M.rowpointer, M.columnindex,
                                                                 T.rowpointer, dcnt, nullptr, nullptr);
        TSG_HIP(hipGetLastError());
        std::vector<int> cnt((size_t)nd);
        TSG_HIP(hipMemcpyAsync(cnt.data(), dcnt, (size_t)nd * sizeof(int), hipMemcpyDeviceToHost, s));
        TSG_TRY(stream_wait(s));
        long long total = 0;
        for (int r = 0; r < nd; ++r) {  // (counts -> offsets; at most one unit per mask entry: fits an int)
            const int c = cnt[r];
            cnt[r] = (int)total;
            total += c;
        }
        if (total > (long long)INT_MAX) return TSG_ERR_OVERFLOW;
        const size_t b_rp = up256(((size_t)nt + 1) * sizeof(int)), b_ci = up256((size_t)B.nnz * sizeof(int)),
                     b_val = up256((size_t)B.nnz * sizeof(double)), b_units = up256((size_t)total * sizeof(int4));
        p.bytes = b_rp + 2 * b_ci + b_val + b_units;
        if (hipMalloc(&p.block, p.bytes) != hipSuccess) {
            (void)hipGetLastError();
            p.block = nullptr;
            return TSG_ERR_OOM;
        }
        char *q = (char *)p.block;
        p.bt_val = (double *)q, q += b_val;
        p.units = (int4 *)q, q += b_units;
        p.bt_rp = (int *)q, q += b_rp;
        p.bt_ci = (int *)q, q += b_ci;
        p.bt_pos = (int *)q;
        p.nunits = (int)total;
        TSG_HIP(hipMemcpyAsync(dcnt, cnt.data(), (size_t)nd * sizeof(int), hipMemcpyHostToDevice, s));
        k_msk_cut<true><<<grid_for(nd, WAVES, 4096), WG, 0, s>>>(drows, nd, A.rowpointer, M.rowpointer, M.columnindex,
                                                                T.rowpointer, nullptr, dcnt, p.units);
        TSG_HIP(hipGetLastError());
        TSG_HIP(hipMemcpyAsync(p.bt_rp, T.rowpointer, ((size_t)nt + 1) * sizeof(int), hipMemcpyDeviceToDevice, s));
        if (B.nnz) {
            TSG_HIP(hipMemcpyAsync(p.bt_ci, T.columnindex, (size_t)B.nnz * sizeof(int), hipMemcpyDeviceToDevice, s));
            TSG_HIP(hipMemcpyAsync(p.bt_pos, tpos, (size_t)B.nnz * sizeof(int), hipMemcpyDeviceToDevice, s));
        }
        TSG_TRY(stream_wait(s));
    }
    info.dot_units = p.nunits;
    // 5. the row-wise leg: a numeric plan over the mask, the other rows skipped
    TSG_TRY(dev_numeric_plan_create(cx, A, B, M, p.rows, s, skip.data(), &bsorted));
    p.A = A;
    p.B = B;
    p.M = M;
    p.A.value = p.B.value = p.M.value = nullptr;
    p.info = info;
    return TSG_OK;
}

// Synchronous (the one-off cost).  Temporaries come from the pool and go back
// to it; what the plan keeps is its own (the row-wise leg's block and one more).
int dev_masked_plan_create(Context &cx, const tsg_dev_csr &A, const tsg_dev_csr &B, const tsg_dev_csr &M, int mode,
                           MaskedPlan &p, hipStream_t s) {
    p = MaskedPlan{};
    const int rc = masked_plan_build(cx, A, B, M, mode, p, s);
    if (rc != TSG_OK) {
        if (hipStreamSynchronize(s) != hipSuccess) (void)hipGetLastError();  // (nothing of the block's in flight)
        dev_masked_plan_free(p);
        p = MaskedPlan{};
    }
    return rc;
}

// Queued on s and waited for: no allocation, every geometry from the plan.  The
// dot units first (the longest-running workgroups), then the row-wise leg in
// dev_numeric_run's order, which also waits for the stream.  The semiring picks
// both legs' instantiations (tsg_semiring.h); one that reads no values skips the
// gather.  An unknown semiring: TSG_ERR_INVALID, nothing queued.
int dev_masked_run(Context &cx, MaskedPlan &p, int semiring, const double *a_val, const double *b_val,
                   double *c_val, hipStream_t s, hipEvent_t *ev) {
    if (!semiring_known(semiring)) return TSG_ERR_INVALID;
    if (ev) TSG_HIP(hipEventRecord(ev[6], s));
    if (p.nunits) {
        const MskOps o{p.A.rowpointer, p.A.columnindex, p.M.rowpointer, p.M.columnindex, p.bt_rp, p.bt_ci,
                       a_val,          p.bt_val,        c_val};
        (void)semiring_dispatch(semiring, [&](auto sr) {
            using SR = decltype(sr);
            if (SR::kValues && p.B.nnz)
                k_msk_gather<<<grid_for(p.B.nnz, WG * 4, 8192), WG, 0, s>>>(p.bt_pos, p.B.nnz, b_val, p.bt_val);
            for (int u0 = 0; u0 < p.nunits; u0 += kMaxGridBlocks)  // (a grid holds fewer than 2^32 threads)
                k_msk_dot<SR><<<std::min(p.nunits - u0, kMaxGridBlocks), WG, 0, s>>>(p.units + u0, o);
            return TSG_OK;
        });
        TSG_HIP(hipGetLastError());
    }
    int missed = 0;  // (products whose column the mask lacks: dropped, by definition)
    return dev_numeric_run(cx, p.rows, semiring, a_val, b_val, c_val, s, ev, &missed);
}

}  // namespace tsg
