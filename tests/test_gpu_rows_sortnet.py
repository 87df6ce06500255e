"""The merge classes' sorting network (tsg_rows.hip: wave_sort256, xwave_merge)
at the fills where it changes shape.  A row of P products is padded with ~0u
keys to a power of two; each wave sorts 256 positions in registers -- skipping
the levels past 64 / 128 when its keys fit there -- and the waves' segments are
merged through LDS, where a wave holding padding alone only joins the barriers
and a wave whose partner segment is all padding keeps its keys without the
read.  So the cases are rows of exactly P products with P on both sides of
every multiple of 64 / 128 / 256 that changes which waves are live, in every
class M0..M4; runs that interleave fully (keys cross every wave boundary) or
arrive largest first (every key travels to its mirror); equal columns, one
pair across a multiple of 256 in sorted order; the largest packed key beside
the padding; and the windowed sort fill's units (k_rows_wsort) at the same
fills.  TSG_PATH=rows; pattern exact, values within 1e-10 of |A||B| against
the oracle, as in test_gpu_rows.py."""
import numpy as np
import pytest

from _cases import csr_of_rows as _csr
from test_gpu_rows import CAPS, _check, _classes

pytestmark = pytest.mark.gpu

M0 = 2  # (class indices as in test_gpu_rows.CAPS: S16, S64, M0..M4)
# products per row, by class M0..M4
FILLS = [[65, 127, 128, 129, 192, 193, 255, 256],
         [257, 320, 321, 384, 385, 512],
         [513, 640, 768, 769, 1024],
         [1025, 1281, 1536, 1537, 2048],
         [2049, 2305, 3072, 3073, 3841, 4096]]
POS_BITS = [8, 9, 10, 11, 12]  # a packed key's position bits, by class M0..M4
T_RUNS = 7                     # runs per row: within every class's entry cap


@pytest.fixture(autouse=True)
def rows_path(monkeypatch):
    monkeypatch.setenv("TSG_PATH", "rows")


def _interleaved_runs(P, t, base):
    """t runs of P products in all, run j holding the columns base + j + k*t
    below base + P: consecutive columns sit in different runs.  Then some
    columns repeated in two runs: sorted position i + 1 takes position i's
    column for i = 10, P - 2 and -- past 256 products -- 255."""
    runs = [np.arange(j, P, t) for j in range(t)]
    owner = np.arange(P) % t
    for i in [10, P - 2] + ([255] if P > 257 else []):
        r = runs[owner[i + 1]]
        r[r == i + 1] = i  # (the run's neighbours are i + 1 - t and i + 1 + t: still ascending)
    srt = np.sort(np.concatenate(runs))
    assert len(srt) == P and srt[10] == srt[11] and (P <= 257 or srt[255] == srt[256])
    assert all((np.diff(r) > 0).all() for r in runs)
    return [r + base for r in runs]


def _block_runs(P, t, base):
    """t runs of P products in all, contiguous column blocks, run 0 the largest
    columns and the last run the smallest; neighbouring runs share their
    boundary column."""
    lens = [P // t + (j < P % t) for j in range(t)]
    runs, top = [], P
    for j in range(t):
        runs.append(np.arange(top - lens[j], top) + base)
        top -= lens[j] - 1  # (the next run ends on this one's first column)
    assert sum(len(r) for r in runs) == P and (t == 1 or runs[0].min() > runs[-1].max())
    return runs


def _fills_case(make_runs):
    Brows, Arows, want = [], [], []
    for c, fills in enumerate(FILLS):
        for P in fills:
            runs = make_runs(P, T_RUNS, 1000)
            Arows.append(np.arange(len(Brows), len(Brows) + len(runs)))
            Brows += runs
            want.append(M0 + c)
    A = _csr(len(Arows), len(Brows), Arows)
    B = _csr(len(Brows), 1000 + 4096 + 8, Brows)
    blen = np.diff(B[2].astype(np.int64))
    assert [int(blen[r].sum()) for r in Arows] == sum(FILLS, [])
    assert list(_classes(A[0], A[1], A[2], A[3], B[2])) == want
    return A, B


def test_sortnet_wave_fill_boundaries_interleaved_runs():
    A, B = _fills_case(_interleaved_runs)
    _check(A, B, real=True, seed=71)


def test_sortnet_wave_fill_boundaries_descending_runs():
    A, B = _fills_case(_block_runs)
    _check(A, B, real=True, seed=73)


def test_sortnet_packing_edge():
    """Per class a row whose column span is the widest that packs,
    (1 << (32 - position bits)) - 2 -- its last product is the largest packed
    key, beside the ~0u padding -- and a row one column wider, which takes the
    unpacked merge-path branch."""
    lo = 3
    Brows, Arows, want = [], [], []
    for c, ib in enumerate(POS_BITS):
        P = CAPS[M0 + c][0] * 3 // 4 + 5  # (padding follows the keys; the last wave partly filled)
        for extra in (0, 1):
            runs = _interleaved_runs(P, T_RUNS, lo)
            last = max(range(T_RUNS), key=lambda j: runs[j][-1])
            runs[last][-1] = lo + (1 << (32 - ib)) - 2 + extra
            # the row's last product (largest expansion position) holds the largest column
            runs.append(runs.pop(last))
            Arows.append(np.arange(len(Brows), len(Brows) + len(runs)))
            Brows += runs
            want.append(M0 + c)
    n = lo + (1 << 24) + 4
    A = _csr(len(Arows), len(Brows), Arows)
    B = _csr(len(Brows), n, Brows)
    spans = [max(Brows[r][-1] for r in a) - min(Brows[r][0] for r in a) for a in Arows]
    assert spans == [(1 << (32 - ib)) - 2 + e for ib in POS_BITS for e in (0, 1)]
    assert list(_classes(A[0], A[1], A[2], A[3], B[2])) == want
    _check(A, B, real=True, seed=79)


# a windowed unit's products: fills on both sides of the waves' 256, and of the
# last wave's 64 / 128
UNIT_FILLS = [1, 64, 65, 128, 129, 256, 257, 320, 321, 384, 385, 512, 513, 640, 641, 768, 769, 1023, 1024]


@pytest.mark.parametrize("descending", [False, True])
def test_sortnet_windowed_sort_fill_pad_waves(monkeypatch, descending):
    """k_rows_wsort: a class-H row (past 4,096 products, wider than one bitmap)
    on the checked-scan path, its windows of 2^18 columns holding exactly
    UNIT_FILLS products each, from three runs per window -- interleaved, or in
    blocks with the largest columns first."""
    monkeypatch.setenv("TSG_ROWS_CHECKED_SCAN", "1")
    wb = 18
    Brows = []
    for w, nprod in enumerate(UNIT_FILLS):
        t = min(3, nprod)
        if descending:
            runs = _block_runs(nprod, t, w << wb)
        elif nprod > 12:
            runs = _interleaved_runs(nprod, t, w << wb)
        else:
            runs = [np.arange(j, nprod, t) + (w << wb) for j in range(t)]
        Brows += runs
    assert min(r[0] for r in Brows) == 0  # (the windows start at the row's first column)
    nb = len(Brows)
    Brows += [np.array([5, 900]), np.array([17])]
    n = len(UNIT_FILLS) << wb
    A = _csr(3, len(Brows), [np.arange(nb), np.array([nb, nb + 1]), np.array([nb + 1])])
    B = _csr(len(Brows), n, Brows)
    assert sum(UNIT_FILLS) > CAPS[-1][0] and n > (1 << 20)
    _check(A, B, real=True, seed=83)
