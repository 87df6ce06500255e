"""Transpose, csr2tile and the masked plan's B^T at the edges of the device's
segmented sort (segmented_sort_u64, tsg_device.hip) and of the tile writer
k_c2t_fill, every output bit-exact against a plain reference.

The sort's tiers by segment length (SORT_T1, SORT_T2, SORT_T3):
  tier 1, 2..16 keys       one thread, insertion sort
  tier 2, 17..512 keys     one wave, bitonic           (at most 8,192 resident waves)
  tier 3, 513..4,096 keys  one workgroup, bitonic      (at most 1,024 workgroups)
  tier 4, longer           4,096-key chunks sorted in LDS, each key placed by
                           rank; (segment, chunk) pairs on at most 1,024 workgroups
A segment is a column (transpose, the masked plan's B^T), a tile row (csr2tile)
or a tile column (the CSC tile order of the col-major form).  k_c2t_fill then
walks each sorted tile row in batches of 64 keys (one wave), carrying the tile
count and the tile's first position from batch to batch.

Every case computes its segment lengths on the host from its own inputs and
asserts the tiers it names, so a case that degenerates fails.  The transpose
reference is the reference's matrix_transposition in numpy (a counting scatter
in CSR order: a stable sort by column); the tiled layouts are compared with the
oracle's, which tests/test_oracle.py pins to the reference's host code (the
fixture x_rect_wide_64x4096 pins this file's wide operand there too)."""
import os

import numpy as np
import pytest

import _oracle as O
from _cases import tile_row_groups
from conftest import FIXTURES
from spgemm_amd import synth
from spgemm_amd import tilespgemm as T
from test_gpu_masked import _check, _csr, _dev, _reference, _run, _values
from test_gpu_parity import TILE_KEYS, assert_rowidx

pytestmark = pytest.mark.gpu

SORT_T1, SORT_T2, SORT_T3 = 16, 512, 4096  # tsg_device.hip
BATCH = 64                                 # k_c2t_fill: keys per wave batch
T2_WAVES, T3_GROUPS, T4_GROUPS = 8192, 1024, 1024  # the grids' caps (segmented_sort_u64)


@pytest.fixture(scope="module")
def ctx():
    from spgemm_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _tiers(lens):
    """per segment: 0 (nothing to sort), or its tier 1..4"""
    lens = np.asarray(lens, dtype=np.int64)
    return np.where(lens <= 1, 0, np.where(lens <= SORT_T1, 1, np.where(lens <= SORT_T2, 2,
                                                                         np.where(lens <= SORT_T3, 3, 4))))


def _chunks(lens):
    """tier 4's 4,096-key chunks per segment (0 for the other tiers)"""
    lens = np.asarray(lens, dtype=np.int64)
    return np.where(lens > SORT_T3, (lens + SORT_T3 - 1) // SORT_T3, 0)


def _coo_to_csr(m, n, rows, cols, rng):
    """CSR of the entries with the columns inside each row in shuffled order and
    distinct values (a permutation of 1..nnz)"""
    order = np.lexsort((rng.random(len(rows)), rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    vv = rng.permutation(len(rows)).astype(np.float64) + 1.0
    return m, n, rp, np.asarray(cols)[order].astype(np.int32), vv


def _rows_to_csr(m, n, rows, rng):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    return m, n, rp, ci, rng.permutation(len(ci)).astype(np.float64) + 1.0


def _transpose_ref(m, n, rp, ci, vv):
    """matrix_transposition: entries with equal columns keep their CSR order"""
    rows_of_entries = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
    order = np.argsort(ci, kind="stable")
    rpT = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n))]).astype(np.int32)
    return n, m, rpT, rows_of_entries[order], vv[order]


def _assert_csr(got, want, who, values=True):
    assert (got[0], got[1]) == (want[0], want[1]), who
    np.testing.assert_array_equal(got[2], want[2], err_msg=who + " rowpointer")
    np.testing.assert_array_equal(got[3], want[3], err_msg=who + " columnindex")
    if values:
        np.testing.assert_array_equal(got[4], want[4], err_msg=who + " value")


def _check_host_transpose(M, want):
    _assert_csr(T.transpose(T.Matrix.from_csr(*M)).csr(), want, "tsg_transpose")
    _assert_csr(O.transpose(O.OMat.from_csr(*M)).csr(), want, "oracle transpose")


# ------------------------------------------------------------ 1. transpose, tier edges
COL_COUNTS = [0, 1, 2, 16, 17, 64, 65, 512, 513, 1024, 1025, 4096, 4097, 8191, 8192, 8193, 12289,
              3, 15, 33, 100, 511, 1023, 2000]
REPEATED = {513: 10, 1025: 10, 4097: 10, 8193: 10, 12289: 10}  # column count -> entries that repeat a (row, column)


def _tall_columns(repeats):
    """12,400 x 24, column j with COL_COUNTS[j] entries (repeats included) in
    rows drawn without repeats; with `repeats`, 50 entries in all repeat an
    entry of their row and column -- the count stays, the value differs --, so
    that only the CSR position (the key's low word) orders the two"""
    rng = np.random.default_rng(12400)
    m, n = 12400, len(COL_COUNTS)
    rows, cols = [], []
    for j, c in enumerate(COL_COUNTS):
        k = REPEATED.get(c, 0) if repeats else 0
        r = rng.choice(m, c - k, replace=False)
        rows += [r, rng.choice(r, k, replace=False)]
        cols.append(np.full(c, j))
    return _coo_to_csr(m, n, np.concatenate(rows), np.concatenate(cols), rng)


def _assert_column_tiers(M, repeats):
    m, n, rp, ci, vv = M
    lens = np.bincount(ci, minlength=n)
    assert lens.tolist() == COL_COUNTS and 51000 < len(ci) < 53000
    assert set(_tiers(lens)) == {0, 1, 2, 3, 4}
    for edge in (SORT_T1, SORT_T2, SORT_T3, 2 * SORT_T3):  # either side of every edge
        assert edge in lens and edge + 1 in lens, edge
    assert 3 * SORT_T3 + 1 in lens and sorted(set(_chunks(lens))) == [0, 2, 3, 4]
    rows_of_entries = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
    keys = rows_of_entries * n + ci
    assert len(keys) - len(np.unique(keys)) == (50 if repeats else 0)
    assert len(np.unique(vv)) == len(vv)
    srt = np.concatenate([np.sort(ci[rp[i]:rp[i + 1]]) for i in range(m)])
    assert (srt != ci).any()  # the rows are not column-sorted


def test_transpose_column_tiers(ctx):
    """Columns of 0, 1, 2, 16, 17, 64, 65, 512, 513, 1,024, 1,025, 4,096, 4,097,
    8,191, 8,192, 8,193 and 12,289 entries (and a few between): nothing to sort,
    and tiers 1 to 4 on either side of 16, 512 and 4,096; tier-4 segments of 2,
    3 and 4 chunks on either side of 8,192 and past 12,288.  Unsorted rows, 50
    repeated (row, column) entries, distinct values.  The host tsg_transpose,
    the device tsg_dev_transpose and the latter on a pattern without values."""
    from spgemm_amd.device import DeviceCSR
    M = _tall_columns(repeats=True)
    _assert_column_tiers(M, repeats=True)
    want = _transpose_ref(*M)
    _check_host_transpose(M, want)
    m, n, rp, ci, vv = M
    dA = DeviceCSR.from_host(m, n, rp, ci, vv)
    _assert_csr(ctx.to_host(ctx.transpose(dA)), want, "tsg_dev_transpose")
    ctx.reset()
    got = ctx.to_host(ctx.transpose(DeviceCSR(m, n, dA.rowptr, dA.col, None)))
    _assert_csr(got, want, "tsg_dev_transpose (no values)", values=False)
    ctx.reset()


# ------------------------------------------------------------ 2. transpose, many long segments
def _columns_of(m, n, lo, hi, seed):
    """m x n, column j with lo..hi entries in rows drawn without repeats"""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(lo, hi + 1, n)
    perm = rng.permuted(np.tile(np.arange(m, dtype=np.int32), (n, 1)), axis=1)
    take = np.arange(m)[None, :] < cnt[:, None]
    return _coo_to_csr(m, n, perm[take], np.repeat(np.arange(n), cnt), rng), cnt


@pytest.mark.parametrize("case", ["tier4_dense", "tier2", "tier3"])
def test_transpose_many_segments(case):
    """More segments of a tier than its kernel starts workgroups or waves, so the
    kernels' grid-stride loops run: (a) a dense 4,097 x 1,030 matrix -- 1,030
    tier-4 segments of two chunks, 2,060 (segment, chunk) pairs on 1,024
    workgroups; (b) 10,000 columns of 17..60 entries on 8,192 waves; (c) 1,100
    columns of 513..600 entries on 1,024 workgroups."""
    if case == "tier4_dense":
        m, n = 4097, 1030
        M = (m, n, (np.arange(m + 1) * n).astype(np.int32), np.tile(np.arange(n, dtype=np.int32), m),
             np.arange(m * n, dtype=np.float64))
        lens = np.bincount(M[3], minlength=n)
        assert len(M[3]) == 4_219_910 and (_tiers(lens) == 4).all() and (_chunks(lens) == 2).all()
        assert _chunks(lens).sum() == 2060 > T4_GROUPS
        assert len(M[3]) // SORT_T3 + 1 > T4_GROUPS  # (the grid's size before its cap)
    elif case == "tier2":
        M, cnt = _columns_of(700, 10000, 17, 60, seed=2)
        lens = np.bincount(M[3], minlength=10000)
        assert (lens == cnt).all() and (_tiers(lens) == 2).all() and len(lens) > T2_WAVES
    else:
        M, cnt = _columns_of(700, 1100, 513, 600, seed=3)
        lens = np.bincount(M[3], minlength=1100)
        assert (lens == cnt).all() and (_tiers(lens) == 3).all() and len(lens) > T3_GROUPS
    _check_host_transpose(M, _transpose_ref(*M))


# ------------------------------------------------------------ csr2tile against the oracle
def _tile_row_lens(M, tr):
    rp = M[2].astype(np.int64)
    return np.diff(rp[np.minimum(np.arange(0, M[0] + tr, tr), M[0])])


def _tile_col_lens(M, tr, tc):
    """tiles per tile column"""
    m, n, rp, ci = M[:4]
    rows_of_entries = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
    ntc = (n + tc - 1) // tc
    tiles = np.unique(rows_of_entries // tr * ntc + ci // tc)
    return np.bincount(tiles % ntc, minlength=ntc)


def _sides(tm, tn, colmajor):
    """(rows, columns) of a tile of tsg_csr2tile_{row,col}_major(M, tm, tn): the
    col-major form tiles B, tn x tm"""
    return (tn, tm) if colmajor else (tm, tn)


def _assert_tiles(M, tm, tn, colmajor, who):
    """csr2tile of M itself, every field against the oracle's"""
    A, oA = T.Matrix.from_csr(*M), O.OMat.from_csr(*M)
    tr, tc = _sides(tm, tn, colmajor)
    if colmajor:
        T.csr2tile_col_major(A, tm, tn)
        O.csr2tile_col_major(oA, tm, tn)
    else:
        T.csr2tile_row_major(A, tm, tn)
        O.csr2tile_row_major(oA, tm, tn)
    t, ot = A.tiles(tr, tc // 16, csc=colmajor), oA.tiles(tr, tc // 16, csc=colmajor)
    for k in ("tilem", "tilen", "numtile"):
        assert t[k] == ot[k], (who, k)
    for k in TILE_KEYS:
        np.testing.assert_array_equal(t[k], ot[k], err_msg=f"{who} {k}")
    assert_rowidx(t, ot, who)
    if colmajor:
        np.testing.assert_array_equal(t["csc_tile_ptr"], ot["csc_tile_ptr"], err_msg=who + " csc_tile_ptr")
        np.testing.assert_array_equal(t["csc_tile_rowidx"], ot["csc_tile_rowidx"], err_msg=who + " csc_tile_rowidx")
        np.testing.assert_array_equal(np.diff(t["csc_tile_ptr"]), _tile_col_lens(M, tr, tc))
    else:  # (tile_nnz in tile-row order: the entries ahead of each tile row)
        np.testing.assert_array_equal(t["tile_nnz"][t["tile_ptr"]],
                                      np.concatenate([[0], np.cumsum(_tile_row_lens(M, tr))]))
    return t


# ------------------------------------------------------------ 3. csr2tile, tile-row tiers
WIDE_SUMS = (513, 4096, 4097, 17)
WIDE_ROWS = {16: [513, 4096, 4097, 17], 32: [4609, 4114], 48: [8706, 17], 64: [8723]}
WIDE2_SUMS = (40, 4097, 300, 8193, 16, 12289, 5)


def _wide_fixture():
    """W, the 64 x 4,096 fixture x_rect_wide_64x4096 (tests/golden/gen_extra_mtx.py)
    in its file order, with distinct values"""
    ij = np.loadtxt(os.path.join(FIXTURES, "x_rect_wide_64x4096.mtx"), comments="%", skiprows=1, usecols=(0, 1),
                    dtype=np.int64)
    (m, n), ij = ij[0], ij[1:] - 1
    order = np.argsort(ij[:, 0], kind="stable")
    rp = np.concatenate([[0], np.cumsum(np.bincount(ij[:, 0], minlength=m))]).astype(np.int32)
    vv = np.random.default_rng(64).permutation(len(ij)).astype(np.float64) + 1.0
    return int(m), int(n), rp, ij[order, 1].astype(np.int32), vv


def _wide_second():
    rng = np.random.default_rng(112)
    return _rows_to_csr(16 * len(WIDE2_SUMS), 4096, tile_row_groups(rng, 4096, WIDE2_SUMS), rng)


@pytest.mark.parametrize("colmajor", [False, True], ids=["row_major", "col_major"])
@pytest.mark.parametrize("tm,tn", [(16, 16), (32, 32), (64, 64), (48, 16), (16, 48), (64, 16), (32, 64)])
def test_csr2tile_tile_row_tiers(tm, tn, colmajor):
    """Tile rows at the tier edges.  W (64 x 4,096; groups of 16 rows with 513,
    4,096, 4,097 and 17 entries, in each two empty rows and one with half of the
    entries): at 16-row tiles tiers 2, 3, 4 (two chunks) and 2; at 32 rows 4,609
    and 4,114 entries, two chunks each; at 48 rows 8,706 (three chunks) and 17;
    at 64 rows 8,723, three chunks.  A second operand of the kind (112 x 4,096)
    with tier-4 tile rows of 4,097, 8,193 and 12,289 entries at 16-row tiles --
    2, 3 and 4 chunks -- between short tile rows, so the (segment, chunk) walk
    passes several long segments."""
    tr, _ = _sides(tm, tn, colmajor)
    W = _wide_fixture()
    assert (W[0], W[1]) == (64, 4096) and _tile_row_lens(W, 16).tolist() == list(WIDE_SUMS)
    per_row = np.diff(W[2]).reshape(4, 16)
    assert (per_row[:, [3, 11]] == 0).all() and (per_row[:, 7] == np.array(WIDE_SUMS) // 2).all()
    lens = _tile_row_lens(W, tr)
    assert lens.tolist() == WIDE_ROWS[tr]
    assert _chunks(lens).tolist() == {16: [0, 0, 2, 0], 32: [2, 2], 48: [3, 0], 64: [3]}[tr]
    if tr == 16:
        assert _tiers(lens).tolist() == [3, 3, 4, 2]
    _assert_tiles(W, tm, tn, colmajor, "W")
    W2 = _wide_second()
    lens2 = _tile_row_lens(W2, 16)
    assert lens2.tolist() == list(WIDE2_SUMS) and _chunks(lens2).tolist() == [0, 2, 0, 3, 0, 4, 0]
    assert _chunks(_tile_row_lens(W2, tr)).max() >= 3
    _assert_tiles(W2, tm, tn, colmajor, "W2")


# ------------------------------------------------------------ 4. CSC tile order, tile-column tiers
TALL_COLS = [16388, 513, 17, 16, 1]  # tiles per 16-column tile column at 16-row tiles


def _tall_thin():
    """262,208 x 80.  Columns 0..15: an entry in one row of every 16, and a
    second one in half of those groups of 16 rows; columns 16..31, 32..47, 48..63
    and 64..79: entries in 513, 17, 16 and 1 of the 16-row tiles"""
    rng = np.random.default_rng(80)
    ntr = TALL_COLS[0]
    m, n = 16 * ntr, 80
    k = np.arange(ntr)
    rows, cols = [16 * k + k % 16], [(5 * k) % 16]
    k2 = np.sort(rng.choice(ntr, ntr // 2, replace=False))
    rows.append(16 * k2 + (k2 + 1 + rng.integers(0, 15, len(k2))) % 16)
    cols.append(rng.integers(0, 16, len(k2)))
    for j, c in enumerate(TALL_COLS[1:], start=1):
        kt = np.repeat(rng.choice(ntr, c, replace=False), 2)  # two entries per tile (or one, twice the cell)
        cell = rng.integers(0, 256, len(kt))
        key = np.unique(kt * 256 + cell)
        rows.append(16 * (key // 256) + key % 256 // 16)
        cols.append(16 * j + key % 16)
    return _coo_to_csr(m, n, np.concatenate(rows), np.concatenate(cols), rng)


@pytest.mark.parametrize("t", [16, 64])
def test_csr2tile_tile_column_tiers(t):
    """The col-major form's second sort, a segment per tile column, on a tall
    operand: at 16 x 16 tile columns of 16,388 (tier 4, five chunks), 513 (tier
    3), 17 (tier 2), 16 (tier 1) and 1 tiles; at 64 x 64 tile columns of 4,097
    (tier 4, two chunks) and 1."""
    M = _tall_thin()
    assert (M[0], M[1]) == (262208, 80) and 24000 < len(M[3]) < 27000
    lens = _tile_col_lens(M, t, t)
    if t == 16:
        assert lens.tolist() == TALL_COLS and _tiers(lens).tolist() == [4, 3, 2, 1, 0]
        assert _chunks(lens)[0] == 5
    else:
        assert lens.tolist() == [4097, 1] and _chunks(lens).tolist() == [2, 0]
    tl = _assert_tiles(M, t, t, True, f"tall {t}x{t}")
    assert np.diff(tl["csc_tile_ptr"]).tolist() == lens.tolist()


# ------------------------------------------------------------ 5. the writer's 64-key batches
BATCH_TILE_COLS = (0, 2, 3, 5, 9)  # the tile columns of a tile row's five tiles
SPLIT_AT = {40: (1, 24), 50: (2, 14)}  # tile row f -> (tile, local index at which a tile-local row begins)


def _tile_cells(rng, t, c, split=None):
    """c distinct cells (local row, local column) of a t x t tile; with split=j the
    j first of them (in row order) lie above local row t/2 and the next begins it"""
    if split is None:
        cell = rng.choice(t * t, c, replace=False)
    else:
        half = t * t // 2
        lo = rng.choice(half, split, replace=False)
        hi = half + np.concatenate([[int(rng.integers(0, t))], t + rng.choice(half - t, c - split - 1, replace=False)])
        cell = np.concatenate([lo, hi])
    return cell // t, cell % t


def _batch_edge_operand(t):
    """67 tile rows of t-row tiles; tile row f: a tile of f entries (none for f =
    0), then tiles of 64, 65 and 1 entries and a full one"""
    rng = np.random.default_rng(67 + t)
    rows, cols = [], []
    for f in range(67):
        for q, c in enumerate((f, 64, 65, 1, t * t)):
            split = SPLIT_AT[f][1] if f in SPLIT_AT and SPLIT_AT[f][0] == q else None
            lr, lc = _tile_cells(rng, t, c, split)
            rows.append(t * f + lr)
            cols.append(t * BATCH_TILE_COLS[q] + lc)
    return _coo_to_csr(67 * t, 10 * t, np.concatenate(rows), np.concatenate(cols), rng)


def _segment_offsets(M, t):
    """in-segment offsets, in the sorted order of a tile row's keys, at which a
    tile begins and at which a tile-local row begins inside a tile"""
    m, n, rp, ci = M[:4]
    rows_of_entries = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
    seg, tc, lr = rows_of_entries // t, ci // t, rows_of_entries % t
    order = np.lexsort((lr, tc, seg))
    seg, tc, lr = seg[order], tc[order], lr[order]
    off = np.arange(len(seg)) - np.concatenate([[0], np.cumsum(np.bincount(seg))])[seg]
    new_tile = np.concatenate([[True], (seg[1:] != seg[:-1]) | (tc[1:] != tc[:-1])])
    new_row = ~new_tile & np.concatenate([[False], lr[1:] != lr[:-1]])
    return set(off[new_tile].tolist()), set(off[new_row].tolist()), np.bincount(seg)


@pytest.mark.parametrize("colmajor", [False, True], ids=["row_major", "col_major"])
@pytest.mark.parametrize("t", [16, 64])
def test_csr2tile_fill_batch_edges(t, colmajor):
    """Tile boundaries at every offset of a tile row around the writer's 64-key
    batches: tile row f (f = 0..66) opens with a tile of f entries, so its
    tiles of 64, 65 and 1 entries and its full tile (256 entries at 16 x 16,
    4,096 at 64 x 64) begin at offsets f, f + 64, f + 129 and f + 130 -- tiles
    that end with a batch, begin one, straddle one or two, and a one-entry tile
    first or last in a batch; in tile row 40 a tile-local row begins exactly at
    offset 64 and in tile row 50 at offset 128 inside a tile."""
    M = _batch_edge_operand(t)
    tile_starts, row_starts, seglen = _segment_offsets(M, t)
    assert seglen.tolist() == [f + 130 + t * t for f in range(67)]
    for edge in (BATCH, 2 * BATCH, 3 * BATCH):
        assert {edge - 1, edge, edge + 1} <= tile_starts, edge
    assert {BATCH, 2 * BATCH} <= row_starts
    assert (_tiers(seglen) == (2 if t == 16 else 4)).all()
    tl = _assert_tiles(M, t, t, colmajor, f"batch edges {t}x{t}")
    assert tl["numtile"] == 67 * 5 - 1


# ------------------------------------------------------------ 6. the masked plan's B^T
def test_masked_dot_leg_long_b_columns(ctx):
    """The masked plan transposes B with the same sort.  B is case 1's matrix
    with every entry of a column in a row of its own (the column counts, and so
    the tiers, are case 1's), rows unsorted; A is 8 x 12,400 with sorted rows
    of about 200 entries, the mask the full 8 x 24 pattern.  The dot leg
    intersects A's rows with B^T's, so it needs B^T's rows ascending: a
    mis-sorted B^T clears b_no_repeats and dot_eligible and mode="dot" is then
    refused.  Its values against the row-wise leg's and a dense numpy product
    within 1e-10 * sum |a||b|; two dot runs byte for byte the same."""
    Bm = _tall_columns(repeats=False)
    _assert_column_tiers(Bm, repeats=False)
    B = Bm[:4]
    rng = np.random.default_rng(8)
    A = _csr(8, 12400, [np.sort(rng.choice(12400, int(rng.integers(180, 221)), replace=False)) for _ in range(8)])
    mask = _csr(8, 24, [np.arange(24)] * 8)
    dA, dB, dM = _dev(A), _dev(B), _dev(mask)
    dot = ctx.masked_plan(dA, dB, dM, mode="dot")
    assert dot.info["b_no_repeats"] == 1 and dot.info["dot_eligible"] == 1
    assert dot.info["rows_dot"] == 8 and dot.info["rows_rowwise"] == 0
    rows = ctx.masked_plan(dA, dB, dM, mode="rows")
    assert rows.info["rows_rowwise"] == 8
    av, bv = _values(A, B, seed=81)
    got_dot, _ = _run(dot, av, bv)
    again, _ = _run(dot, av, bv)
    got_rows, _ = _run(rows, av, bv)
    assert got_dot.tobytes() == again.tobytes()
    Ad, Bd = np.zeros((8, 12400), np.longdouble), np.zeros((12400, 24), np.longdouble)
    Ad[np.repeat(np.arange(8), np.diff(A[2])), A[3]] = av
    Bd[np.repeat(np.arange(12400), np.diff(B[2])), B[3]] = bv
    want, mag = (Ad @ Bd).ravel(), (np.abs(Ad) @ np.abs(Bd)).ravel()
    assert (mag > 0).sum() >= 8 * 12
    for got in (got_dot, got_rows):
        assert np.all(np.abs(got - want) <= 1e-10 * mag)
        assert np.all(got[mag == 0] == 0.0)
    assert np.all(np.abs(got_dot - got_rows) <= 1e-10 * mag)
    _check(got_dot, mask, _reference(A, B, av, bv))
    dot.close()
    rows.close()


# ------------------------------------------------------------ 7. a natural operand
@pytest.mark.parametrize("colmajor", [False, True], ids=["row_major", "col_major"])
def test_csr2tile_hub_operand(colmajor):
    """The mawi stand-in at 3e-4 scale (68 K nodes, a hub of degree 3,000) at
    16 x 16: the hub's row makes a tier-3 tile row, the hub's column a tile
    column of more than 512 tiles (tier 3), beside thousands of tier-2
    segments."""
    M = synth.mawi(scale=3e-4)
    rows, cols = _tile_row_lens(M, 16), _tile_col_lens(M, 16, 16)
    hub = int(np.argmax(np.diff(M[2])))
    assert _tiers(rows)[hub // 16] == 3 and rows.argmax() == hub // 16
    assert _tiers(cols)[hub // 16] == 3 and cols.argmax() == hub // 16
    assert (_tiers(rows) == 2).sum() > 1000 and (_tiers(cols) == 2).sum() > 1000
    _assert_tiles(M, 16, 16, colmajor, "mawi")
