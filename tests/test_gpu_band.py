"""The banded path (spgemm_amd/csrc/tsg_band.hip): every C row's reachable
columns inside one window of <= 2,048 columns with at least as many element
products as columns (FEM-like rows, e.g. cant).  One walk per row
accumulates a*b at acc[col - lo] in LDS and marks a hit byte per column; the
row's nonzeros go to a staging slot at the prefix of the window widths, a scan
of the row counts gives the CSR offsets and a compaction kernel moves them.  The library routes such products to it; TSG_PATH=band
forces it whenever the window check passes.  Pattern bit-exact, values within
1e-10 relative, against the oracle."""
import numpy as np
import pytest

import _oracle as O
from spgemm_amd import synth
from spgemm_amd import tilespgemm as T

pytestmark = pytest.mark.gpu


def _sorted_rows(m, n, rp, ci, vv):
    order = np.concatenate([rp[i] + np.argsort(ci[rp[i]:rp[i + 1]], kind="stable") for i in range(m)]
                           ).astype(np.int64) if len(ci) else np.zeros(0, np.int64)
    return m, n, rp, ci[order], vv[order]


def _banded(m, half, seed, fill=1.0):
    """rows i with columns |j - i| <= half (each kept with probability fill)"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(m):
        js = np.arange(max(0, i - half), min(m, i + half + 1))
        js = js[rng.random(len(js)) < fill] if fill < 1.0 else js
        rows.append(np.full(len(js), i))
        cols.append(js)
    r = np.concatenate(rows)
    c = np.concatenate(cols).astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))]).astype(np.int32)
    vv = (np.arange(len(c)) % 10).astype(np.float64)
    return m, m, rp, c, vv


def _check(m, n, rp, ci, vv, aat=False, real=False):
    A = T.Matrix.from_csr(m, n, rp, ci, vv)
    oA = O.OMat.from_csr(m, n, rp, ci, vv)
    if aat:
        B, oB = T.transpose(A), O.transpose(oA)
    else:
        B, oB = T.Matrix.alias(A), O.OMat.alias(oA)
    Cm, st = T.spgemm(A, B)
    got, ref = Cm.csr(), O.gustavson(oA, oB).csr()
    np.testing.assert_array_equal(got[2], ref[2])
    np.testing.assert_array_equal(got[3], ref[3])
    if real:
        oM = O.OMat.from_csr(m, n, rp, ci, np.abs(vv))
        oMb = O.transpose(oM) if aat else O.OMat.alias(oM)
        mag = O.gustavson(oM, oMb).csr()[4]
        assert np.all(np.abs(got[4] - ref[4]) <= 1e-10 * mag)
    else:
        np.testing.assert_allclose(got[4], ref[4], rtol=1e-10, atol=0)
    assert st["nnzC"] == len(ref[3])
    return st


@pytest.fixture
def band(monkeypatch):
    monkeypatch.setenv("TSG_PATH", "band")


@pytest.mark.parametrize("case", ["narrow", "wide_window", "gappy", "one_row", "empty_rows", "dense_block"])
def test_band_forced_vs_oracle(case, band):
    if case == "narrow":
        m, n, rp, ci, vv = _banded(3000, 8, 1)
    elif case == "wide_window":  # windows near the 2,048-column limit
        m, n, rp, ci, vv = _banded(4000, 500, 2, fill=0.3)
    elif case == "gappy":  # sparse band: window check may fail -> another path, same C
        m, n, rp, ci, vv = _banded(3000, 40, 3, fill=0.2)
    elif case == "one_row":
        m, n, rp, ci, vv = synth.random_csr(1, 1, density=1.0, seed=1)
    elif case == "empty_rows":
        m, n, rp, ci, vv = _banded(2000, 16, 4)
        keep = np.ones(m, bool)
        keep[::7] = False  # every 7th row empty
        lens = np.diff(rp) * keep
        mask = np.repeat(keep, np.diff(rp))
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        ci, vv = ci[mask], vv[mask]
    else:
        m, n, rp, ci, vv = _sorted_rows(*synth.random_csr(600, 600, density=0.2, seed=22))
    st = _check(m, n, rp, ci, vv)
    if case in ("narrow", "empty_rows", "dense_block"):
        assert st["path"] == T.PATH_BAND and st["numblkC"] == -1  # the banded path ran


def test_band_aat_and_real_values(band):
    m, n, rp, ci, _ = _banded(2500, 12, 5)
    vv = np.random.default_rng(6).uniform(-1, 1, len(ci))
    st = _check(m, n, rp, ci, vv, aat=True, real=True)
    assert st["path"] == T.PATH_BAND


def test_cant_routes_to_band_and_matches_oracle():
    """The cant stand-in (banded FEM-like, ~64 entries per row) takes the banded
    path by default; rows spread over all columns take the row-merge path."""
    m, n, rp, ci, vv = synth.GENERATORS["cant"]()
    st = _check(m, n, rp, ci, vv)
    assert st["path"] == T.PATH_BAND and st["numblkC"] == -1
    m, n, rp, ci, vv = synth.random_csr(3000, 3000, density=0.01, seed=4)  # spread rows
    st = _check(m, n, rp, ci, vv)
    assert st["path"] == T.PATH_ROWS


# ---------------------------------------------------------------------------
# The capacity edges of k_band_rows / k_band_compact / dev_spgemm_band: shaped
# A (m x k) and B (k x n) from per-row column lists, real values, each case
# proving on the host which edge it sits on before the GPU result is compared.

BD_SPAN = 2048  # tsg_band.hip


def _csr_of(rows, rng):
    """(rowptr, col, val) of per-row column lists, each row's order kept; real
    values of either sign, magnitudes in [0.5, 1.5)"""
    lens = np.array([len(r) for r in rows], np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate([np.asarray(r, np.int64).reshape(-1) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    vv = rng.uniform(0.5, 1.5, len(ci)) * rng.choice([-1.0, 1.0], len(ci))
    return rp, ci, vv


def _windows(arows, brows):
    """per C row what k_band_stats computes: lo, hi (lo > hi: no product), the
    window width and the element products"""
    first = np.array([r[0] if len(r) else 0 for r in brows], np.int64)
    last = np.array([r[-1] if len(r) else 0 for r in brows], np.int64)
    blen = np.array([len(r) for r in brows], np.int64)
    m = len(arows)
    lo, hi = np.full(m, np.iinfo(np.int32).max, np.int64), np.full(m, -1, np.int64)
    prod = np.zeros(m, np.int64)
    for i, a in enumerate(arows):
        a = np.asarray(a, np.int64).reshape(-1)
        a = a[blen[a] > 0] if len(a) else a
        if len(a):
            lo[i], hi[i], prod[i] = first[a].min(), last[a].max(), blen[a].sum()
    width = np.where(hi >= lo, hi - lo + 1, 0)
    return lo, hi, width, prod


def _band_product(arows, brows, n, seed, expect_path=T.PATH_BAND):
    """C = A*B of the per-row column lists against Gustavson (pattern and row
    pointers bit-exact, values within 1e-10 of |A|*|B|); B's rows must be
    ascending.  Returns (stats, the oracle's row pointers, the windows)."""
    rng = np.random.default_rng(seed)
    m, k = len(arows), len(brows)
    brows = [np.asarray(r, np.int64).reshape(-1) for r in brows]
    assert all(np.all(np.diff(r) > 0) for r in brows) and all(len(r) == 0 or (r[0] >= 0 and r[-1] < n) for r in brows)
    arp, aci, avv = _csr_of(arows, rng)
    brp, bci, bvv = _csr_of(brows, rng)
    assert len(aci) == 0 or (aci.min() >= 0 and aci.max() < k)
    win = _windows(arows, brows)
    if expect_path == T.PATH_BAND:
        assert win[2].max() <= BD_SPAN  # every window fits: the band check passes
    Cm, st = T.spgemm(T.Matrix.from_csr(m, k, arp, aci, avv), T.Matrix.from_csr(k, n, brp, bci, bvv))
    got = Cm.csr()
    ref = O.gustavson(O.OMat.from_csr(m, k, arp, aci, avv), O.OMat.from_csr(k, n, brp, bci, bvv)).csr()
    mag = O.gustavson(O.OMat.from_csr(m, k, arp, aci, np.abs(avv)), O.OMat.from_csr(k, n, brp, bci, np.abs(bvv))).csr()
    assert (got[0], got[1]) == (m, n)
    np.testing.assert_array_equal(got[2], ref[2])
    np.testing.assert_array_equal(got[3], ref[3])
    np.testing.assert_array_equal(mag[3], ref[3])
    assert np.all(np.abs(got[4] - ref[4]) <= 1e-10 * mag[4])
    assert st["nnzC"] == len(ref[3])
    assert st["path"] == expect_path, st["path"]  # (no other route can have produced this C)
    return st, ref[2], win


def _pick(rng, lo, hi, cnt):
    return np.sort(rng.choice(np.arange(lo, hi), size=cnt, replace=False))


B_ROW_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 192, 193, 300)


def test_band_b_row_lengths(band):
    """B rows of 1 .. 300 entries: lane l holds entries l and l + 64 (one set
    at <= 64, the second set's last lane at 128), 129 and more take the direct
    walk from entry 128 on in steps of 64 (192: one full step, 193: one lane of
    a second, 300: three).  Each length alone in an A row, then mixed in both
    orders and interleaved with short rows."""
    rng = np.random.default_rng(101)
    brows = [_pick(rng, 40 + 3 * i, 40 + 3 * i + max(2 * L, 8), L) for i, L in enumerate(B_ROW_LENGTHS)]
    brows += [_pick(rng, 10, 700, 5) for _ in range(4)]  # short rows to mix in
    nl = len(B_ROW_LENGTHS)
    arows = [[i] for i in range(nl)]
    arows += [list(range(nl)), list(range(nl))[::-1], [0, 9, 1, 8, 2, 7, 3, 6, 4, 5],
              [10, 5, 11, 7, 12, 9, 13, 6], [9, 9, 8], [5, 7, 5]]
    # a long row between equal-pattern rows of 127 and 128 entries, all in wave 0's share
    # (the direct walk flushes the pending sums first)
    brows += [brows[4].copy(), brows[5].copy()]
    seq = [4, 14, 8, 14, 4, 5, 15, 9, 15]
    arows.append(seq + [10, 11, 12, 13] * 7)
    assert (len(arows[-1]) + 3) // 4 >= len(seq) and np.array_equal(brows[14], brows[4])
    assert set(B_ROW_LENGTHS) <= {len(r) for r in brows}
    assert all(sorted(a) == list(range(nl)) for a in arows[nl:nl + 3])
    _band_product(arows, brows, 800, 1)


def _runs(arow, brows):
    """maximal runs of consecutive A entries whose B rows are non-empty and have
    identical column lists: [(first position, length)]"""
    out, p = [], 0
    while p < len(arow):
        q = p + 1
        while (q < len(arow) and len(brows[arow[p]]) > 0 and len(brows[arow[q]]) == len(brows[arow[p]])
               and np.array_equal(brows[arow[q]], brows[arow[p]])):
            q += 1
        out.append((p, q - p))
        p = q
    return out


def _pattern_b():
    """B for the equal-pattern cases: seven rows each of the patterns of 20, 100,
    128 and 64 columns (rows 0-6, 7-13, 14-20, 21-27), row 28 = the 20-column
    pattern with one other column, row 29 = the 100-column pattern with another
    column at entry 80 (lane 16's second register), row 30 empty, rows 31..330
    short rows with pairwise different patterns."""
    rng = np.random.default_rng(202)
    # (even columns only: the column after any of them is free for the rows that differ)
    pats = [2 * _pick(rng, 50, 200, 20), 2 * _pick(rng, 0, 350, 100), 2 * _pick(rng, 150, 450, 128),
            2 * _pick(rng, 25, 250, 64)]
    brows = [p.copy() for p in pats for _ in range(7)]
    odd20, odd100 = pats[0].copy(), pats[1].copy()
    odd20[7] += 1
    odd100[80] += 1
    brows += [odd20, odd100, np.zeros(0, np.int64)]
    brows += [np.array([i, i + 3 + i % 5, i + 40]) for i in range(300)]
    return brows


FILL0 = 31  # the first short row of _pattern_b


def _shares(arow):
    """the four waves' contiguous shares of an A row's entries (k_band_rows: per = (entries + 3) / 4)"""
    per = (len(arow) + 3) // 4
    return [arow[w * per:(w + 1) * per] for w in range(4)]


def _in_one_wave(seq, wave, fill):
    """an A row whose wave `wave` walks exactly `seq` (a wave combines B rows only
    inside its own share, so a run of L rows needs an A row of at least 4 L - 3
    entries): short rows from `fill` on everywhere else, the last share one
    entry short"""
    L = len(seq)
    row = [FILL0 + (fill + i) % 300 for i in range(wave * L)] + list(seq)
    row += [FILL0 + (fill + 150 + i) % 300 for i in range(4 * L - 1 - len(row))]
    assert _shares(row)[wave] == list(seq)
    return row


def _pattern_a(case):
    f = lambda *idx: [FILL0 + i for i in idx]  # noqa: E731
    seqs = None
    if case == "runs":  # runs of 1, 2, 3 and 7 rows of each pattern, alone and back to back
        seqs = []
        for b in (0, 7, 14, 21):
            seqs += [[b, b + 1], [b, b + 1, b + 2], list(range(b, b + 7)), f(5) + [b + 2, b + 3] + f(6) + [b]]
        seqs.append([0] + [7, 8] + [14, 15, 16] + list(range(21, 28)) + [1])
        seqs.append(f(0) + [3, 4] + f(1, 2) + [9, 10, 11] + f(3))
    elif case == "share_boundary":  # shares of 4, 3 and 2 entries: the run's parts in neighbouring waves
        return [f(0, 1) + [7, 8, 9, 10] + f(2, 3, 4, 5, 6, 7, 8, 9, 10, 11),     # 16 entries: run at 2..5, cut at 4
                f(0) + list(range(0, 7)) + f(1, 2, 3, 4),                         # 12 entries: run at 1..7, cuts at 3, 6
                list(range(14, 21)) + f(0)]                                        # 8 entries: a run of 7 over 3 cuts
    elif case == "batch_boundary":  # per >= 65: a wave's share spans two 64-entry batches
        return [f(*range(62)) + [14, 15, 16, 17, 18] + f(*range(62, 255)),       # 260 entries: run at 62..66
                f(*range(61)) + list(range(0, 7)) + f(*range(61, 293))]          # 300 entries: run at 61..67
    elif case == "other_column":  # same length, one column different: the run ends
        seqs = [[0, 1, 28, 2, 3], [7, 8, 29, 9], [28, 0], [29, 7], [28, 28, 0], [7, 29, 29, 8]]
    elif case == "empty_row":  # an empty B row inside a run
        seqs = [[0, 1, 30, 2], [30, 0], [0, 30], [30, 30, 7, 30, 30, 8], [14, 30, 14]]
    else:
        assert case == "same_row_twice"  # adjacent and apart
        seqs = [[3, 3], [3, 3, FILL0, 3], [7, 7, 7], [9, FILL0 + 1, FILL0 + 2, 9], [14, 21, 14, 21, 14]]
    return [_in_one_wave(q, w, 17 * i) for i, q in enumerate(seqs) for w in ((0, 2) if i % 2 else (3, 1))]


@pytest.mark.parametrize("case", ["runs", "share_boundary", "batch_boundary", "other_column", "empty_row",
                                  "same_row_twice"])
def test_band_equal_pattern_runs(case, band):
    """Consecutive A entries whose B rows have identical columns and different
    values (the dof triplets of FEM operands) are summed in registers by the
    wave whose share holds them and flushed at a change of pattern -- at the
    end of a 64-entry batch only if the next batch's first row differs (the
    pending state crosses batches) -- and at the end of the wave's share."""
    brows = _pattern_b()
    arows = _pattern_a(case)
    # the runs each wave sees (inside its share), and the runs of the whole row
    seen = [[_runs(sh, brows) for sh in _shares(a)] for a in arows]
    whole = [_runs(a, brows) for a in arows]
    per = [(len(a) + 3) // 4 for a in arows]
    lens = {n for row in seen for sh in row for _, n in sh}
    if case == "runs":
        assert {1, 2, 3, 7} <= lens
        for b in (0, 7, 14, 21):  # ... of every pattern (20, 100, 128 and 64 columns)
            assert {2, 3, 7} <= {n for a, row in zip(arows, seen) for sh, rs in zip(_shares(a), row)
                                 for p, n in rs if sh[p] in range(b, b + 7)}
    elif case == "share_boundary":  # a run holds the entries on both sides of a share's end
        assert all(any(p < c * pr < p + n for p, n in r for c in (1, 2, 3)) for r, pr in zip(whole, per))
        assert seen[0][:2] == [[(0, 1), (1, 1), (2, 2)], [(0, 2), (2, 1), (3, 1)]]
        assert [max(n for _, n in sh) for sh in seen[1][:3]] == [2, 3, 2] and per[1:] == [3, 2]
    elif case == "batch_boundary":  # ... of entries 63 and 64 of wave 0's share
        assert all(len(a) >= 260 and pr >= 65 for a, pr in zip(arows, per))
        assert all(any(p <= 63 and p + n > 64 and n > 1 for p, n in row[0]) for row in seen)
    elif case == "other_column":
        assert len(brows[28]) == len(brows[0]) and np.count_nonzero(brows[28] != brows[0]) == 1
        assert len(brows[29]) == len(brows[7]) and np.flatnonzero(brows[29] != brows[7]).tolist() == [80]
        assert seen[0][3] == [(0, 2), (2, 1), (3, 2)] and seen[2][0] == [(0, 2), (2, 1), (3, 1)]
    elif case == "empty_row":
        assert len(brows[30]) == 0 and seen[0][3] == [(0, 2), (2, 1), (3, 1)]
    else:
        assert seen[0][3] == [(0, 2)] and seen[2][0] == [(0, 2), (2, 1), (3, 1)]
        assert seen[6][0] == [(0, 1), (1, 1), (2, 1), (3, 1)]
    _band_product(arows, brows, 1000, 2)


A_ROW_ENTRIES = (1, 2, 3, 4, 5, 255, 256, 257, 260, 2048)


def test_band_a_row_entry_counts(band):
    """A rows of 1 .. 2,048 entries: fewer entries than waves (empty shares),
    shares of 64 (255, 256: one batch each), 65 (257, 260: a second batch of
    nj = 1) and 512 entries (2,048: eight batches per wave).  B's rows come in
    triplets of one pattern, so runs cross the batch and share ends."""
    k = 2130
    brows = [np.array([j // 3, j // 3 + 4, j // 3 + 11]) for j in range(k)]
    arows = [list(range(7 * i, 7 * i + c)) for i, c in enumerate(A_ROW_ENTRIES)]
    arows.insert(3, [])
    assert set(A_ROW_ENTRIES) <= {len(a) for a in arows}
    assert (260 + 3) // 4 == 65 and (2048 + 3) // 4 == 8 * 64
    _band_product(arows, brows, k // 3 + 12, 3)


WINDOW_WIDTHS = (1, 7, 8, 9, 31, 32, 33, 63, 65, 2047, 2048)


def test_band_window_widths(band):
    """Windows of 1 .. 2,048 columns starting at columns that are no multiple of
    8 or 32: only the first and the last column hit (the pack's bytes and the
    popcount scan's words at their ends), then every column hit and a random
    half of them; a row whose entries all select empty B rows (lo > hi, span 0)
    and a row without entries lie between them."""
    rng = np.random.default_rng(404)
    brows, arows, want = [np.zeros(0, np.int64), np.zeros(0, np.int64)], [], []
    for i, w in enumerate(WINDOW_WIDTHS):
        lo = 1003 + 38 * i if w < 2047 else 13 + 2 * i
        assert lo % 8 and lo % 32
        base = len(brows)
        brows += [np.array([lo]), np.array([lo + w - 1]), np.arange(lo, lo + w),
                  np.unique(np.concatenate([[lo, lo + w - 1], _pick(rng, lo, lo + w, (w + 1) // 2)]))]
        arows += [[base, base + 1], [0, 1], [base + 2], [], [base + 1, 0, base + 3, base]]
        want += [w, 0, w, 0, w]
    lo_, hi_, width, _ = _windows(arows, brows)
    assert width.tolist() == want and set(WINDOW_WIDTHS) <= set(width.tolist())
    assert np.all(lo_[width == 0] > hi_[width == 0])
    _, rp, _ = _band_product(arows, brows, 2100, 4)
    cnt = np.diff(rp)
    assert cnt[0::5].tolist() == [min(w, 2) for w in WINDOW_WIDTHS]  # first and last column only
    assert cnt[2::5].tolist() == list(WINDOW_WIDTHS)                   # every column
    assert not cnt[1::5].any() and not cnt[3::5].any()


def _routing_case(case):
    """A with 8 entries a row (rows i..i+7 of B), B row j = columns j .. j+L-1"""
    if case in ("window_2048", "window_2049"):
        # dense windows (40 products per entry against 47 columns a row) so that only the
        # width of the last row's window can send the product away from the band
        m, L = 200, 40
        brows = [np.arange(j, j + L) for j in range(m + 7)]
        far = (m - 1) + (2048 if case == "window_2049" else 2047)
        brows[m + 6] = np.concatenate([brows[m + 6], [far]])
        return [list(range(i, i + 8)) for i in range(m)], brows, far + 1
    # B row j = column j alone: 8 products and 8 window columns a row
    m = 64
    brows = [np.array([j]) for j in range(m + 7)]
    arows = [list(range(i, i + 8)) for i in range(m)]
    if case == "nnz_8m_minus_1":
        arows[0] = arows[0][1:]  # (its window loses the column with the product)
    elif case == "products_one_short":
        brows[m + 6] = np.array([m + 7])  # the last row's window one column wider, no product more
    return arows, brows, m + 8


@pytest.mark.parametrize("case,path", [("window_2048", T.PATH_BAND), ("window_2049", T.PATH_ROWS),
                                       ("nnz_8m", T.PATH_BAND), ("nnz_8m_minus_1", T.PATH_ROWS),
                                       ("products_equal", T.PATH_BAND), ("products_one_short", T.PATH_ROWS)])
def test_band_routing_at_the_limits(case, path, monkeypatch):
    """The default routing (no TSG_PATH) at its three limits: the window check
    runs from nnz(A) = 8 m on, passes while no window is wider than 2,048
    columns and while the products are no fewer than the window columns.  One
    step past each limit the product takes the row-merge path; the same C."""
    monkeypatch.delenv("TSG_PATH", raising=False)
    arows, brows, n = _routing_case(case)
    m, nnz = len(arows), sum(len(a) for a in arows)
    _, _, width, prod = _windows(arows, brows)
    if case.startswith("window"):
        assert nnz == 8 * m and width.max() == (2049 if case == "window_2049" else 2048)
        assert prod.sum() >= width.sum() + 2049  # dense either way
    elif case == "nnz_8m_minus_1":
        assert nnz == 8 * m - 1 and prod.sum() >= width.sum() and width.max() <= BD_SPAN
    else:
        assert nnz == 8 * m and width.max() <= BD_SPAN
        assert prod.sum() - width.sum() == (-1 if case == "products_one_short" else 0)
    _band_product(arows, brows, n, 5, expect_path=path)


C_ROW_COUNTS = (192, 193, 256, 257, 448, 449)


def test_band_compaction_row_lengths(band):
    """k_band_compact moves 256 entries a step while i + 192 < n and the rest 64
    at a time: C rows of 192 (tail only), 193 (one step, the lanes past the row
    masked), 256, 257 (a step and a tail of one), 448 and 449 (two steps)
    nonzeros, each the union of two overlapping B rows; staging offsets from the
    prefix of the window widths and the fixed 2,048 slots a row both."""
    rng = np.random.default_rng(606)
    brows, arows = [], []
    for c in C_ROW_COUNTS:
        cols = _pick(rng, 5, 5 + 2 * c, c)
        brows += [cols[: 2 * c // 3], cols[c // 3:]]
        arows.append([len(brows) - 2, len(brows) - 1])
    _, rp, (_, _, width, _) = _band_product(arows, brows, 1000, 6)
    assert np.diff(rp).tolist() == list(C_ROW_COUNTS)
    assert len(arows) * BD_SPAN <= 4 * width.sum()  # 2,048 staging slots a row
    # the same rows among 3,000 narrow ones: m * 2,048 > 4 x the window columns -> prefix offsets
    nb = len(brows)
    brows += [np.array([7 + j % 50]) for j in range(8)]
    arows = [[nb + i % 8] for i in range(1500)] + arows + [[nb + i % 8] for i in range(1500)]
    _, rp, (_, _, width, _) = _band_product(arows, brows, 1000, 7)
    assert len(arows) * BD_SPAN > 4 * width.sum()
    assert np.diff(rp)[1500:1500 + len(C_ROW_COUNTS)].tolist() == list(C_ROW_COUNTS)


def test_band_more_rows_than_the_fused_scans_take(band):
    """m + 1 > 2,048 tiles of 4,096 values: the scan of the window widths and the
    scan of the row counts both leave their two-launch form for the generic
    scans (dev_spgemm_band).  A has one entry a row (every 1,000th row none), B
    eight rows of 1-3 columns: C row i = a_i * B[i % 8], in closed form."""
    m = 2048 * 4096 + 5
    assert m + 1 > 2048 * 4096
    bcols = [[0], [1, 2], [0, 2, 5], [3], [4, 6], [1, 5, 7], [], [2, 3, 4]]
    blen = np.array([len(r) for r in bcols], np.int64)
    brp = np.concatenate([[0], np.cumsum(blen)]).astype(np.int32)
    bci = np.concatenate([np.array(r, np.int32) for r in bcols]).astype(np.int32)
    bvv = np.array([2.0 ** (j % 5 - 2) * (1 - 2 * (j % 2)) for j in range(len(bci))])
    rows = np.arange(m, dtype=np.int64)
    has = rows % 1000 != 999
    arp = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    aci = (rows[has] % 8).astype(np.int32)
    avv = 1.0 + 0.5 * (rows[has] % 7)
    Cm, st = T.spgemm(T.Matrix.from_csr(m, 8, arp, aci, avv), T.Matrix.from_csr(8, 8, brp, bci, bvv))
    assert st["path"] == T.PATH_BAND
    _, _, crp, cci, cvv = Cm.csr()
    clen = np.zeros(m, np.int64)
    clen[has] = blen[aci]
    np.testing.assert_array_equal(crp, np.concatenate([[0], np.cumsum(clen)]))
    # entry e of C: the (e - start of its A entry)th entry of B row aci
    ent = np.repeat(np.arange(len(aci)), blen[aci])
    off = np.arange(len(ent)) - np.repeat(np.cumsum(blen[aci]) - blen[aci], blen[aci])
    src = brp[aci[ent]] + off
    np.testing.assert_array_equal(cci, bci[src])
    np.testing.assert_array_equal(cvv, avv[ent] * bvv[src])  # (one product each, exact)
    assert st["nnzC"] == len(src)


def test_band_rectangular_a_times_b(band):
    """A (m x k) times a distinct B (k x n), m != k != n, real values: banded
    rows of 6-30 entries over B rows of 4-40 columns."""
    rng = np.random.default_rng(808)
    m, k, n = 700, 430, 1900
    brows = [_pick(rng, 4 * j, 4 * j + 90, int(rng.integers(4, 41))) for j in range(k)]
    arows = []
    for i in range(m):
        c = i * k // m
        lo, hi = max(0, c - 20), min(k, c + 21)
        arows.append(_pick(rng, lo, hi, min(hi - lo, int(rng.integers(6, 31)))).tolist())
    assert m != k and k != n and m != n and max(r[-1] for r in brows) < n
    _band_product(arows, brows, n, 8)
