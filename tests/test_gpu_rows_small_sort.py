"""Classes S16 / S64 of the row-merge path (tsg_rows.hip: k_rows_small): a row's
products, one per lane, are ranked by sorting packed keys (column - the row's
minimum) << 6 | lane with a one-key-per-lane bitonic network over the row's 16
or 64 lanes; a row whose column span does not fit the key's 26 bits counts its
smaller keys instead.  The cases: rows of 2..16 runs at the products that fill
a lane group partly, exactly and by one less (and one past a half), with runs
that interleave fully or arrive largest columns first; one column in every run
(a sum of as many terms as runs); two equal columns in neighbouring sorted
positions; S16 rows of different lengths sharing a wave; the widest span that
packs, one column more, and a B of 2^26 + 10 columns with rows touching its
first and last column.  TSG_PATH=rows; pattern exact, values within 1e-10 of
|A||B| against the oracle, as in test_gpu_rows.py."""
import numpy as np
import pytest

from _cases import csr_of_rows as _csr
from test_gpu_rows import _check, _classes

pytestmark = pytest.mark.gpu

S16, S64 = 0, 1
P16, P64 = [2, 3, 15, 16], [17, 31, 32, 33, 63, 64]
SPAN_BITS = 26  # a packed key's column bits


@pytest.fixture(autouse=True)
def rows_path(monkeypatch):
    monkeypatch.setenv("TSG_PATH", "rows")


def _interleaved(P, t, base):
    """t runs, P products: run j holds base + j, base + j + t, ... (< base + P)"""
    return [np.arange(j, P, t) + base for j in range(t)]


def _descending(P, t, base):
    """t runs of contiguous columns, P in all: run 0 the largest, the last the smallest"""
    lens = [P // t + (j < P % t) for j in range(t)]
    runs, top = [], P
    for L in lens:
        runs.append(np.arange(top - L, top) + base)
        top -= L
    return runs


def _with_equal_pair(runs, i):
    """sorted position i + 1 takes position i's column (they sit in different runs)"""
    runs = [r.copy() for r in runs]
    own = next(r for r in runs if (r == i + 1).any())
    assert not (own == i).any()
    own[own == i + 1] = i
    assert (np.diff(own) > 0).all()
    return runs


def _build(rowruns, n):
    """A, B from per-row lists of runs: every run a B row of its own"""
    Brows, Arows = [], []
    for runs in rowruns:
        Arows.append(np.arange(len(Brows), len(Brows) + len(runs)))
        Brows += list(runs)
    return _csr(len(Arows), len(Brows), Arows), _csr(len(Brows), n, Brows)


def _want(rowruns):
    return [S16 if sum(len(r) for r in runs) <= 16 else S64 for runs in rowruns]


def _fill_rows(make):
    rows = []
    for P in P16 + P64:
        for t in sorted({2, min(3, P), min(7, P), min(16, P)}):
            rows.append(make(P, t, 100 + 3 * P))
    return rows


@pytest.mark.parametrize("make", [_interleaved, _descending], ids=["interleaved", "descending"])
def test_small_sort_group_fills(make):
    rows = _fill_rows(make)
    assert all(2 <= len(r) <= 16 for r in rows)
    A, B = _build(rows, 1000)
    assert list(_classes(A[0], A[1], A[2], A[3], B[2])) == _want(rows)
    _check(A, B, real=True, seed=151)


def test_small_sort_repeated_columns():
    rows = []
    # one column in every run: sums of as many terms as the row has runs
    for t in (2, 3, 15, 16):                                     # S16: t runs of that one column
        rows.append([np.array([77])] * t)
    for t, extra in ((16, 3), (16, 1), (9, 6), (2, 31)):         # S64: the column and `extra` others per run
        rows.append([np.sort(np.concatenate([[500], 10 + j * extra + np.arange(extra) + (490 if j % 2 else 0)]))
                     for j in range(t)])
    rows.append([np.array([4])] * 64)                            # 64 runs: a 64-fold sum
    # a pair of equal columns in neighbouring sorted positions: first, inside, last
    for P, t in ((16, 4), (15, 2), (64, 16), (33, 5), (63, 7)):
        for i in (0, P // 2, P - 2):
            rows.append(_with_equal_pair(_interleaved(P, t, 0), i))
    A, B = _build(rows, 1200)
    cls = _classes(A[0], A[1], A[2], A[3], B[2])
    assert list(cls[:4]) == [S16] * 4 and list(cls[4:9]) == [S64] * 5 and list(cls) == _want(rows)
    _check(A, B, real=True, seed=157)


def test_small_sort_s16_rows_of_different_lengths_share_a_wave():
    """the S16 kernel's wave holds eight rows (two per 16 lanes): their products
    2, 3, 15, 16 and 16, 5, 9, 2, then a partly filled wave"""
    rows = [_interleaved(P, 2, 10 * i) if i % 2 else _descending(P, min(P, 3), 10 * i)
            for i, P in enumerate([2, 3, 15, 16, 16, 5, 9, 2, 7, 16, 1 + 1])]
    A, B = _build(rows, 400)
    assert list(_classes(A[0], A[1], A[2], A[3], B[2])) == [S16] * len(rows)
    _check(A, B, real=True, seed=163)


def test_small_sort_span_edges_and_unpacked_rows():
    """per class the widest span that packs, 2^26 - 2 (its last product is the
    largest packed key, beside the ~0u padding), one column more (counted
    ranks), and rows touching column 0 and the last of 2^26 + 10 columns"""
    n = (1 << SPAN_BITS) + 10
    lim = (1 << SPAN_BITS) - 2

    def wide(P, t, span):
        lo = 0 if span == n - 1 else 7
        runs = _interleaved(P, t, lo)
        last = max(range(t), key=lambda j: runs[j][-1])
        runs[last][-1] = lo + span
        runs.append(runs.pop(last))  # the row's last product (its highest lane) holds the largest column
        return runs

    # S16: the four rows that share a lane-group slot of a wave pack together or
    # not at all -- the first four all pack, each of the next four sits beside a
    # row that does not
    rows = [wide(5, 2, lim), wide(16, 3, lim), _interleaved(12, 3, 50), _interleaved(9, 2, 50),
            wide(5, 2, lim + 1), wide(16, 3, n - 1), _interleaved(12, 3, 50), wide(16, 3, lim)]
    spans = [lim, lim, 11, 8, lim + 1, n - 1, 11, lim]
    for P, t in ((40, 3), (64, 16)):  # S64: a row per wave
        for span in (lim, lim + 1, n - 1):
            rows.append(wide(P, t, span))
            spans.append(span)
    rows.append(_interleaved(50, 4, 50))
    spans.append(49)
    A, B = _build(rows, n)
    assert list(_classes(A[0], A[1], A[2], A[3], B[2])) == [S16] * 8 + [S64] * 7
    assert spans == [max(r[-1] for r in runs) - min(r[0] for r in runs) for runs in rows]
    _check(A, B, real=True, seed=167)
