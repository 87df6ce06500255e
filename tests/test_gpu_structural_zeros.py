"""No zero dropping, on every route: pairs of A entries
+a and -a select B rows with identical columns and values, so the sum at those
columns is 0 -- exactly, in any order, every value being a small power of two.
C must keep the columns with value 0.0; in the tiled outputs their mask bits
must be set.  Routes: the banded, row-merge and staged tile paths of the CSR
call, tsg_tilespgemm at 16 x 16 (CSR streaming and tile payloads) and at
32 x 32, and the numeric-only run on the known pattern."""
import numpy as np
import pytest

import _oracle as O
from spgemm_amd import tilespgemm as T

pytestmark = pytest.mark.gpu
M, K, N = 100, 120, 300


def _pow2(rng, cnt, signed=True):
    v = 2.0 ** rng.integers(-3, 4, cnt)
    return v * rng.choice([-1.0, 1.0], cnt) if signed else v


def _operands():
    """B: rows 2g and 2g+1 (g < 20) identical, rows 40+g and 100+g identical, rows
    60..99 on their own.  A row i: +a and -a on one pair (adjacent entries for
    even i, a third entry between them for odd i), every third row a second
    pair, most rows an entry of their own whose B row shares some columns.
    Returns A, B as (m, n, rowptr, col, val), C's structural pattern as per-row
    column arrays and per row the columns whose sum cancels."""
    rng = np.random.default_rng(2)
    bcols, bvals = [None] * K, [None] * K
    for g in range(20):
        for lo, hi in ((2 * g, 2 * g + 1), (40 + g, 100 + g)):
            c = np.sort(rng.choice(np.arange(2 * lo, 2 * lo + 60), size=int(rng.integers(3, 13)), replace=False))
            v = _pow2(rng, len(c))
            bcols[lo], bvals[lo], bcols[hi], bvals[hi] = c, v, c.copy(), v.copy()
    for j in range(60, 100):
        bcols[j] = np.sort(rng.choice(np.arange(j, j + 120), size=int(rng.integers(2, 20)), replace=False))
        bvals[j] = _pow2(rng, len(bcols[j]))
    acols, avals, pattern, zeros = [], [], [], []
    for i in range(M):
        g = i % 20
        a = float(_pow2(rng, 1)[0])
        ent = {2 * g: a, 2 * g + 1: -a} if i % 2 == 0 else {40 + g: a, 100 + g: -a}
        if i % 3 == 0:  # a second pair in the same row
            a2 = float(_pow2(rng, 1)[0])
            ent.update({2 * ((g + 7) % 20): -a2, 2 * ((g + 7) % 20) + 1: a2})
        own = [60 + (i * 7) % 40] if i % 5 else []
        if i % 2:  # (odd rows: always an entry between the pair's two)
            own = [60 + (i * 7) % 40]
        for j in own:
            ent[j] = float(_pow2(rng, 1)[0])
        cols = np.array(sorted(ent), np.int64)
        acols.append(cols)
        avals.append(np.array([ent[j] for j in cols]))
        pattern.append(np.unique(np.concatenate([bcols[j] for j in cols])))
        live = np.unique(np.concatenate([bcols[j] for j in own])) if own else np.zeros(0, np.int64)
        zeros.append(np.setdiff1d(pattern[-1], live))
    arp = np.concatenate([[0], np.cumsum([len(c) for c in acols])]).astype(np.int32)
    brp = np.concatenate([[0], np.cumsum([len(c) for c in bcols])]).astype(np.int32)
    A = (M, K, arp, np.concatenate(acols).astype(np.int32), np.concatenate(avals))
    B = (K, N, brp, np.concatenate(bcols).astype(np.int32), np.concatenate(bvals))
    return A, B, pattern, zeros


@pytest.fixture(scope="module")
def case():
    A, B, pattern, zeros = _operands()
    ref = O.gustavson(O.OMat.from_csr(*A), O.OMat.from_csr(*B)).csr()
    crp = np.concatenate([[0], np.cumsum([len(p) for p in pattern])])
    ccol = np.concatenate(pattern)
    # the oracle keeps the structural pattern, and the cancelling columns are exact zeros there
    np.testing.assert_array_equal(ref[2], crp)
    np.testing.assert_array_equal(ref[3], ccol)
    iszero = np.concatenate([np.isin(p, z) for p, z in zip(pattern, zeros)])
    assert iszero.sum() > 400 and (~iszero).sum() > 400
    assert np.all(ref[4][iszero] == 0.0)
    for a in (crp, ccol, iszero, ref[4]):
        a.setflags(write=False)
    return A, B, crp, ccol, iszero, ref[4]


def _assert_csr(got, case):
    _, _, crp, ccol, iszero, val = case
    np.testing.assert_array_equal(got[2], crp)
    np.testing.assert_array_equal(got[3], ccol)  # the cancelled columns are kept
    assert np.all(got[4][iszero] == 0.0)         # ... with value exactly 0.0
    np.testing.assert_array_equal(got[4], val)   # (sums of a few small powers of two: exact in any order)


@pytest.mark.parametrize("path,want", [("band", T.PATH_BAND), ("rows", T.PATH_ROWS), ("tiles", T.PATH_TILES)])
def test_structural_zeros_kept_by_the_csr_routes(path, want, case, monkeypatch):
    monkeypatch.setenv("TSG_PATH", path)
    Cm, st = T.spgemm(T.Matrix.from_csr(*case[0]), T.Matrix.from_csr(*case[1]))
    assert st["path"] == want
    _assert_csr(Cm.csr(), case)
    assert st["nnzC"] == len(case[3])


@pytest.mark.parametrize("tm,mode", [(16, None), (16, "0"), (32, None)])
def test_structural_zeros_kept_by_the_tiled_routes(tm, mode, case, monkeypatch):
    if mode is None:
        monkeypatch.delenv("TSG_TILED_CSR", raising=False)
    else:
        monkeypatch.setenv("TSG_TILED_CSR", mode)
    A, B, crp, ccol, iszero, _ = case
    tA, tB = T.Matrix.from_csr(*A), T.Matrix.from_csr(*B)
    oA, oB = O.OMat.from_csr(*A), O.OMat.from_csr(*B)
    T.csr2tile_row_major(tA, tm, tm)
    T.csr2tile_col_major(tB, tm, tm)
    O.csr2tile_row_major(oA, tm, tm)
    O.csr2tile_col_major(oB, tm, tm)
    Cm, info = T.tilespgemm(tA, tB, tm, tm)
    ct, oct_ = Cm.tiles(tm, tm // 16), O.c_tiles(O.tilespgemm(oA, oB, tm, tm), tm)
    assert info["nnzC"] == len(ccol)
    for k in ("tile_ptr", "tile_columnidx", "tile_rowidx", "tile_nnz", "tile_csr_Ptr", "tile_csr_Col",
              "tile_csr_Value", "mask"):
        np.testing.assert_array_equal(ct[k], oct_[k], err_msg=k)
    # the mask from C's structural pattern alone: word c / 16 of row r, bit 15 - c % 16
    wpr = tm // 16
    rows = np.repeat(np.arange(M), np.diff(crp))
    tp, tc = ct["tile_ptr"], ct["tile_columnidx"]
    tile = np.array([tp[r // tm] + np.searchsorted(tc[tp[r // tm]:tp[r // tm + 1]], c // tm)
                     for r, c in zip(rows, ccol)])
    assert np.all(tc[tile] == ccol // tm)
    want = np.zeros(ct["numtile"] * tm * wpr, np.uint16)
    np.bitwise_or.at(want, tile * tm * wpr + (rows % tm) * wpr + (ccol % tm) // 16,
                     (1 << (15 - ccol % 16)).astype(np.uint16))
    np.testing.assert_array_equal(ct["mask"], want)
    assert np.all(want[(tile * tm * wpr + (rows % tm) * wpr + (ccol % tm) // 16)[iszero]]
                  & (1 << (15 - ccol[iszero] % 16)).astype(np.uint16))
    T.tile2csr(Cm, tm, tm)
    _assert_csr(Cm.csr(), case)


def test_structural_zeros_written_by_the_numeric_run(case):
    A, B, crp, ccol, _, _ = case
    Cm = T.Matrix.from_csr(M, N, crp, ccol, np.full(len(ccol), np.nan))
    st = T.spgemm_numeric(T.Matrix.from_csr(*A), T.Matrix.from_csr(*B), Cm)
    assert st["path"] == T.PATH_NUMERIC
    _assert_csr(Cm.csr(), case)
