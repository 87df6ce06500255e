"""Operand generators shared between test modules (each case is built in one
place; the modules that use it check different things on it)."""
import numpy as np

from spgemm_amd import synth


def csr_of_rows(m, n, rows):
    """CSR from a list of per-row column arrays (kept in the given order)"""
    lens = [len(c) for c in rows]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = (np.concatenate(rows) if sum(lens) else np.zeros(0)).astype(np.int32)
    vv = (np.arange(len(ci)) % 10).astype(np.float64)
    return m, n, rp, ci, vv


def tile_row_groups(rng, n, sums):
    """per-row column arrays of a 16 * len(sums) x n operand whose groups of 16
    rows hold sums[g] entries: rows 3 and 11 of a group empty, row 7 with half
    of the entries (at most n: a full row), the rest spread unevenly; a row's
    columns drawn without repeats and kept in drawn (unsorted) order.  The
    operand of tests/test_gpu_sort_tiers.py's tile-row cases and of the fixture
    x_rect_wide_64x4096 (tests/golden/gen_extra_mtx.py)."""
    rows = []
    for L in sums:
        w = rng.random(16)
        w[[3, 7, 11]] = 0
        heavy = min(L // 2, n)
        lens = np.floor(w / w.sum() * (L - heavy)).astype(int)
        lens[7] = heavy
        light = [r for r in range(16) if r not in (3, 7, 11)]
        for r in light[:L - lens.sum()]:  # (what flooring left over: fewer than 13)
            lens[r] += 1
        assert lens.sum() == L and lens.max() <= n
        rows += [rng.choice(n, size=int(l), replace=False) for l in lens]
    return rows


def hub_rows_case():
    """(A, B, arows) of test_rows_hub_rows_windowed_and_dominant_run: hub rows
    (past 65,536 products) without a dominant run -- many runs over 1,500,000
    columns with heavy collisions, two long colliding runs -- and with one (one
    long run with a few short ones, a row of one run), class-H rows of a few
    thousand products over the whole span, beside ordinary rows."""
    rng = np.random.default_rng(41)
    n = 1_500_000
    nb = 3000
    Brows = [np.sort(rng.choice(n, size=int(rng.integers(20, 120)), replace=False)) for _ in range(nb - 3)]
    Brows.append(np.sort(rng.choice(n, size=200_000, replace=False)))  # a hub's long row
    Brows.append(np.sort(rng.choice(np.arange(1000, 1000 + 150_000), size=90_000, replace=False)))  # narrow
    Brows.append(np.arange(0, n, 7)[:80_000])
    B = csr_of_rows(nb, n, Brows)
    arows = [np.sort(rng.choice(nb - 3, size=1500, replace=False)),   # ~100k products, many runs
             np.array([5, 17, nb - 3]),                                # long run + short ones
             np.array([nb - 2, nb - 1]),                               # two long runs, colliding
             np.array([nb - 2])]                                       # one run, one window
    # class-H rows of a few thousand products over the whole span: windows of
    # 2^18 columns, units of ~700 / ~1,050 / ~2,300 products (the sort fill's
    # and the bitmap fill's sizes on either side of 1,024)
    arows += [np.sort(rng.choice(nb - 3, size=k, replace=False)) for k in (60, 90, 200)]
    arows += [np.sort(rng.choice(nb - 3, size=5, replace=False)) for _ in range(50)]
    A = csr_of_rows(len(arows), nb, arows)
    return A, B, arows


def numeric_mixed_case():
    """(A, B) patterns (m, n, rowptr, col) of test_numeric_mixed_classes: row
    lengths spread over 0..600 so every class of the numeric plan appears"""
    rng = np.random.default_rng(11)
    n = 5000
    rows = []
    for i in range(3000):
        L = int(rng.choice([0, 1, 2, 3, 5, 8, 20, 60, 150, 600], p=[.1, .2, .15, .15, .1, .1, .08, .06, .04, .02]))
        rows.append(np.sort(rng.choice(n, size=L, replace=False)))
    A = csr_of_rows(3000, n, rows)[:4]
    Bm = synth.random_csr(n, 7000, density=0.003, seed=12)
    B = (Bm[0], Bm[1], Bm[2],
         np.concatenate([np.sort(Bm[3][Bm[2][i]:Bm[2][i + 1]]) for i in range(n)]).astype(np.int32))
    return A, B
