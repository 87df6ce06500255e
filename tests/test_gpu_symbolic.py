"""Symbolic SpGEMM (tsg_dev_spgemm_symbolic / Context.spgemm_symbolic,
tsg_spgemm_csr_symbolic): C's row pointers and columns without values, against
the oracle's Gustavson pattern on unit values (scipy on unit values for the
large cases: all sums positive, nothing drops) and against the pattern of the
full product.  Every comparison of row pointers and columns is exact.  Operands
go up without values unless a case says otherwise."""
import glob
import os

import numpy as np
import pytest

from conftest import FIXTURES
import _oracle as O
from _cases import csr_of_rows, hub_rows_case, numeric_mixed_case
from spgemm_amd import _lib, synth
from spgemm_amd import tilespgemm as T

pytestmark = pytest.mark.gpu

# the classes' product caps and the window (tsg_internal.h; tests/test_symbolic_cpu.py pins them to the source)
PACKED_CAP, SET_WAVE_CAP, SET_CAP, WINDOW_CAP = 32, 512, 4096, 65536
W = 131072
HUB_UNIT = 4096
ERR_INVALID, ERR_OOM, ERR_OVERFLOW = -1, -3, -4


@pytest.fixture(scope="module")
def ctx():
    from spgemm_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _csr(m, n, rows):
    return csr_of_rows(m, n, rows)[:4]


def _dev(M, val=None):
    """the pattern on the device, without values unless val is given"""
    import torch
    from spgemm_amd.device import DeviceCSR
    m, n, rp, ci = M[:4]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    return DeviceCSR(m, n, t(rp, np.int32), t(ci, np.int32), None if val is None else t(val, np.float64))


def _ref_oracle(A, B):
    oA = O.OMat.from_csr(*A[:4], np.ones(len(A[3])))
    oB = O.OMat.from_csr(*B[:4], np.ones(len(B[3])))
    r = O.gustavson(oA, oB).csr()
    return np.asarray(r[2], dtype=np.int32), np.asarray(r[3], dtype=np.int32)


def _ref_scipy(A, B):
    import scipy.sparse as sp
    mk = lambda M: sp.csr_matrix((np.ones(len(M[3])), M[3].astype(np.int64), M[2].astype(np.int64)), shape=M[:2])
    Cs = (mk(A) @ mk(B)).tocsr()
    Cs.sort_indices()
    assert np.all(Cs.data > 0)
    return Cs.indptr.astype(np.int32), Cs.indices.astype(np.int32)


def _shuffled_rows(B, seed):
    m, n, rp, ci = B[:4]
    rng = np.random.default_rng(seed)
    out = ci.copy()
    for i in range(m):
        out[rp[i]:rp[i + 1]] = rng.permutation(ci[rp[i]:rp[i + 1]])
    return m, n, rp, out


def _products(A, B):
    blen = np.diff(B[2].astype(np.int64))
    cum = np.concatenate([[0], np.cumsum(blen[A[3]])])
    return cum[A[2][1:]] - cum[A[2][:-1]]


def _expected_info(A, B, b_sorted):
    """rows per class and the work units from the documented caps"""
    P = _products(A, B)
    cls = [int(((P > lo) & (P <= hi)).sum()) for lo, hi in
           ((0, PACKED_CAP), (PACKED_CAP, SET_CAP), (SET_CAP, WINDOW_CAP), (WINDOW_CAP, 1 << 62))]
    units = int(np.sum((P[P > WINDOW_CAP] + HUB_UNIT - 1) // HUB_UNIT))
    brp, bci = B[2], B[3]
    for i in np.nonzero((P > SET_CAP) & (P <= WINDOW_CAP))[0]:
        lo, hi = 0, B[1] - 1
        if b_sorted:
            ks = A[3][A[2][i]:A[2][i + 1]]
            ks = ks[brp[ks + 1] > brp[ks]]
            lo, hi = int(bci[brp[ks]].min()), int(bci[brp[ks + 1] - 1].max())
        w0 = lo & ~31
        units += (hi - w0) // W + 1
    return cls, units, int(P.sum())


def _rows_sorted(M):
    rp, ci = M[2], M[3]
    if len(ci) < 2:
        return True
    asc = np.ones(len(ci), dtype=bool)
    asc[1:] = np.diff(ci.astype(np.int64)) > 0
    asc[rp[:-1][np.diff(rp) > 0]] = True
    return bool(asc.all())


def _sym(ctx, A, B, mode="pattern", aval=None, bval=None):
    """(rowptr, col or None, info, stats) of a symbolic call, copied to the host"""
    dA, dB = _dev(A, aval), _dev(B, bval)
    c, info, st = ctx.spgemm_symbolic(dA, dB, mode)
    assert c.value is None and c.m == A[0] and c.n == B[1]
    _, _, rp, ci, vv = ctx.to_host(c)
    has_cols = bool(c.columnindex)
    assert vv is None or c.nnz == 0
    assert rp[0] == 0 and rp[-1] == c.nnz == info["nnzC"] == st["nnzC"]
    assert st["path"] == T.PATH_SYMBOLIC == 6 and st["nnzCub"] == info["products"]
    assert st["numtileA"] == -1 and st["numblkC"] == -1 and st["t_step1_ms"] == 0
    ctx.reset()
    return rp, (ci if has_cols or c.nnz == 0 else None), info, st


def _check(ctx, A, B, ref=None, mode="pattern"):
    rrp, rci = ref if ref is not None else _ref_oracle(A, B)
    rp, ci, info, st = _sym(ctx, A, B, mode)
    np.testing.assert_array_equal(rp, rrp)
    if mode == "pattern":
        np.testing.assert_array_equal(ci, rci)
    else:
        assert ci is None or len(rci) == 0
    b_sorted = _rows_sorted(B)
    cls, units, products = _expected_info(A, B, b_sorted)
    assert info["rows_class"] == cls, (info, cls)
    assert info["products"] == products
    assert info["units"] == units
    assert info["b_rows_sorted"] == int(b_sorted)
    return info


def _full_pattern(ctx, A, B):
    c, st = ctx.spgemm(_dev(A, np.ones(len(A[3]))), _dev(B, np.ones(len(B[3]))))
    _, _, rp, ci, _ = ctx.to_host(c)
    ctx.reset()
    return rp, ci, st


# ---------------------------------------------------------------- 1. fixtures
def _fixture_cases():
    out = []
    for p in sorted(glob.glob(os.path.join(FIXTURES, "*.mtx"))):
        name = os.path.basename(p)[:-4]
        if "rect" not in name:
            out.append(pytest.param(p, False, id=name + "-AA"))
        out.append(pytest.param(p, True, id=name + "-AAT"))
    return out


@pytest.mark.parametrize("path,aat", _fixture_cases())
def test_symbolic_fixtures(ctx, path, aat):
    oA = O.OMat.load(path)
    m, n, rp, ci, _ = oA.csr()
    assert aat or m == n
    A = (m, n, rp, ci)
    B = O.transpose(oA).csr()[:4] if aat else A
    info = _check(ctx, A, B)
    frp, fci, _ = _full_pattern(ctx, A, B)
    got = _sym(ctx, A, B)
    np.testing.assert_array_equal(got[0], frp)
    np.testing.assert_array_equal(got[1], fci)
    if "unsorted" in path and not aat:
        assert info["b_rows_sorted"] == 0


def test_symbolic_fixture_set_is_complete():
    names = {os.path.basename(p)[:-4] for p in glob.glob(os.path.join(FIXTURES, "*.mtx"))}
    assert {"x_int_unsorted_dup_77", "x_rect_50x130", "x_empty_rows_64", "x_banded_500"} <= names


# ---------------------------------------------------------------- 2. classes and caps
@pytest.fixture(scope="module")
def mixed():
    A, B = numeric_mixed_case()
    return A, B, _ref_oracle(A, B)


def test_symbolic_mixed_classes(ctx, mixed):
    A, B, ref = mixed
    info = _check(ctx, A, B, ref)
    assert all(c > 0 for c in info["rows_class"][:3]), info
    assert info["b_rows_sorted"] == 1


@pytest.mark.parametrize("cap", [PACKED_CAP, SET_WAVE_CAP, SET_CAP, WINDOW_CAP])
def test_symbolic_product_cap_edges_few_columns(ctx, cap):
    """rows of exactly cap and cap + 1 products onto 8 columns: every referenced
    B row holds the same 8 columns (one more holds the first of them alone)"""
    k = cap // 8
    A = _csr(2, k + 1, [np.arange(k), np.arange(k + 1)])
    B = _csr(k + 1, 40, [np.arange(3, 11)] * k + [np.array([3])])
    info = _check(ctx, A, B, _ref_scipy(A, B))
    assert info["nnzC"] == 16 and info["products"] == 2 * cap + 1
    P = _products(A, B)
    assert list(P) == [cap, cap + 1]


@pytest.mark.parametrize("cap", [PACKED_CAP, SET_WAVE_CAP, SET_CAP, WINDOW_CAP])
def test_symbolic_product_cap_edges_distinct_columns(ctx, cap):
    """rows of exactly cap and cap + 1 distinct columns against an identity B:
    len_C = P, the fullest a class's set can get"""
    n = cap + 900
    rng = np.random.default_rng(cap)
    A = _csr(2, n, [rng.choice(n, size=cap, replace=False), rng.choice(n, size=cap + 1, replace=False)])
    B = _csr(n, n, [np.array([i]) for i in range(n)])
    info = _check(ctx, A, B, _ref_scipy(A, B))
    assert info["nnzC"] == 2 * cap + 1 == info["products"]


def test_symbolic_rows_without_products_and_single_products(ctx):
    """P = 0 (no A entries; A entries on empty B rows only), P = 1, and a packed
    row most of whose A entries meet empty B rows"""
    Brows = [np.zeros(0), np.array([4]), np.zeros(0), np.array([1, 4, 9]), np.zeros(0)]
    B = _csr(5, 12, Brows)
    A = _csr(6, 5, [np.zeros(0), np.array([0, 2, 4]), np.array([1]), np.array([0, 2, 4] * 30 + [3, 1]),
                    np.array([2]), np.array([3, 3, 3])])
    info = _check(ctx, A, B)
    assert info["rows_class"] == [3, 0, 0, 0] and info["nnzC"] == 1 + 3 + 3


@pytest.mark.parametrize("b_sorted", [True, False], ids=["sortedB", "unsortedB"])
def test_symbolic_every_product_on_one_column(ctx, b_sorted):
    """len C = 1 however large P: a row per class"""
    nb = 70000
    Brows = [np.array([7])] * nb
    Brows[0] = np.array([7, 7, 7]) if not b_sorted else Brows[0]  # (a repeat makes B's rows unsorted)
    B = _csr(nb, 20, Brows)
    ks = [20, 300, 3000, 50000, nb]
    A = _csr(len(ks), nb, [np.arange(1, k + 1) % nb for k in ks])
    info = _check(ctx, A, B, _ref_scipy(A, B))
    assert info["nnzC"] == len(ks) and all(c > 0 for c in info["rows_class"])


# ---------------------------------------------------------------- 3. bitmap edges
def _edge_case(target):
    """every row's B row repeated until the row holds target products or a few more"""
    n = 2 * W + 37
    assert n % 32 != 0
    edges = np.array([0, 31, 32, 63, 64, W - 1, W, 2 * W - 1, 2 * W, n - 1])
    Brows = [edges, np.array([2 * W, 2 * W + 5, n - 1]), np.array([5, 100, 2 * W + 1]),
             np.arange(0, n, 997), np.array([W - 1]), np.array([n - 1])]
    B = _csr(len(Brows), n, Brows)
    arows = [np.full(-(-target // len(Brows[k])), k) for k in range(len(Brows))]
    arows.append(np.concatenate([arows[2], np.full(3, 3)]))  # the empty middle window beside a spread row
    A = _csr(len(arows), len(Brows), arows)
    return A, B


@pytest.mark.parametrize("b_sorted", [True, False], ids=["sortedB", "unsortedB"])
@pytest.mark.parametrize("target", [5000, 70000], ids=["window", "hub"])
def test_symbolic_bitmap_edges(ctx, target, b_sorted):
    A, B = _edge_case(target)
    if not b_sorted:
        B = _shuffled_rows(B, 3)
    info = _check(ctx, A, B, _ref_scipy(A, B))
    want = [0, 0, 0, 0]
    want[2 if target == 5000 else 3] = A[0]
    assert info["rows_class"] == want


# ---------------------------------------------------------------- 4. hub class
@pytest.fixture(scope="module")
def hub():
    A, B, _ = hub_rows_case()
    A, B = A[:4], B[:4]
    return A, B, _ref_scipy(A, B)


def test_symbolic_hub_rows(ctx, hub):
    A, B, ref = hub
    info = _check(ctx, A, B, ref)
    assert info["rows_class"][3] == 4 and info["rows_class"][2] >= 2


@pytest.mark.parametrize("budget", [400000, 1], ids=["two-rows-a-batch", "one-row-a-batch"])
def test_symbolic_hub_rows_in_batches(ctx, hub, monkeypatch, budget):
    """more hub rows than one batch's bitmaps hold (the budget shrunk by the
    test-only knob): 4 hub rows of 187,504-byte bitmaps in 2 and in 4 batches"""
    A, B, ref = hub
    monkeypatch.setenv("TSG_SYM_HUB_BYTES", str(budget))
    monkeypatch.setenv("TSG_QUIET", "1")
    _check(ctx, A, B, ref)
    _check(ctx, A, B, ref, mode="count")


# ---------------------------------------------------------------- 5. unsorted B with repeats at size
def test_symbolic_unsorted_repeating_b(ctx):
    Am = synth.random_csr(300, 2000, nnz_per_row=40, seed=5, unsorted=True, dups=True)
    Bm = synth.random_csr(2000, 300000, nnz_per_row=60, seed=6, unsorted=True, dups=True)
    A, B = Am[:4], Bm[:4]
    info = _check(ctx, A, B, _ref_scipy(A, B))
    assert info["b_rows_sorted"] == 0
    assert info["rows_class"][1] > 0 and info["rows_class"][2] > 0, info


# ---------------------------------------------------------------- 6. agreement with every full route
def _route_case(route):
    if route == "band":
        m, n, rp, ci, _ = O.OMat.load(os.path.join(FIXTURES, "x_banded_500.mtx")).csr()
        return (m, n, rp, ci), (m, n, rp, ci)
    A, B = numeric_mixed_case()
    return (A, B) if route == "rows" else (A, _shuffled_rows(B, 10))


@pytest.mark.parametrize("route,want", [("band", T.PATH_BAND), ("rows", T.PATH_ROWS), ("tiles", T.PATH_TILES)])
def test_symbolic_agrees_with_every_full_route(ctx, monkeypatch, route, want):
    A, B = _route_case(route)
    if route != "band":
        monkeypatch.setenv("TSG_PATH", route)
    frp, fci, st = _full_pattern(ctx, A, B)
    assert st["path"] == want
    monkeypatch.delenv("TSG_PATH", raising=False)
    rp, ci, _, _ = _sym(ctx, A, B)
    np.testing.assert_array_equal(rp, frp)
    np.testing.assert_array_equal(ci, fci)


# ---------------------------------------------------------------- 7. empties
@pytest.mark.parametrize("kind", ["a_empty", "b_empty", "both_empty", "empty_rows_between", "n_is_1", "m_is_0"])
@pytest.mark.parametrize("mode", ["pattern", "count"])
def test_symbolic_empties(ctx, kind, mode):
    none = np.zeros(0)
    if kind == "a_empty":
        A, B = _csr(4, 3, [none] * 4), _csr(3, 5, [np.array([0, 4]), none, np.array([2])])
    elif kind == "b_empty":
        A, B = _csr(3, 4, [np.array([0, 3]), none, np.array([1])]), _csr(4, 6, [none] * 4)
    elif kind == "both_empty":
        A, B = _csr(2, 2, [none] * 2), _csr(2, 2, [none] * 2)
    elif kind == "empty_rows_between":
        A = _csr(5, 3, [np.array([0, 1, 2]), none, np.array([1]), none, np.array([2, 0])])
        B = _csr(3, 9, [np.array([8, 0]), none, np.array([3, 4, 8])])
    elif kind == "n_is_1":
        A, B = _csr(3, 2, [np.array([0, 1]), none, np.array([1])]), _csr(2, 1, [np.array([0]), none])
    else:
        A, B = _csr(0, 3, []), _csr(3, 4, [np.array([1])] * 3)
    ref = _ref_scipy(A, B) if A[0] else (np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32))
    rp, ci, info, _ = _sym(ctx, A, B, mode)
    np.testing.assert_array_equal(rp, ref[0])
    assert info["nnzC"] == len(ref[1])
    if mode == "pattern":
        np.testing.assert_array_equal(ci, ref[1])
    if kind in ("a_empty", "b_empty", "both_empty", "m_is_0"):
        assert not rp.any() and info["nnzC"] == 0 and info["products"] == 0
        c, _, _ = ctx.spgemm_symbolic(_dev(A), _dev(B), mode)
        assert c.nnz == 0 and c.columnindex is None and c.value is None  # (and to_host / to_torch take it)
        assert len(ctx.to_host(c)[3]) == 0 and ctx.to_torch(c).col.numel() == 0 and ctx.view_torch(c).nnz == 0
        ctx.reset()


# ---------------------------------------------------------------- 8. count mode
def test_symbolic_count_mode(ctx, mixed):
    A, B, ref = mixed
    rp, ci, info, _ = _sym(ctx, A, B, "pattern")
    c, info_c, st = ctx.spgemm_symbolic(_dev(A), _dev(B), "count")
    assert c.columnindex is None and c.value is None and c.nnz == len(ref[1])
    _, _, rp_c, ci_c, vv_c = ctx.to_host(c)
    assert len(ci_c) == 0 and vv_c is None
    dv = ctx.view_torch(c)
    assert dv.val is None and dv.col.numel() == 0
    np.testing.assert_array_equal(dv.rowptr.cpu().numpy(), ref[0])
    ctx.reset()
    np.testing.assert_array_equal(rp_c, rp)
    np.testing.assert_array_equal(rp_c, ref[0])
    assert info_c == info
    assert ctx.spgemm_symbolic(_dev(A), _dev(B), 1)[1] == info  # (the mode by its TSG_SYMBOLIC_* value)
    ctx.reset()


# ---------------------------------------------------------------- 9. int32 overflow of the total
def _outer(rows, cols):
    A = _csr(rows, 1, [np.array([0])] * rows)
    B = _csr(1, cols, [np.arange(cols)])
    return A, B


@pytest.mark.parametrize("mode", ["count", "pattern"])
def test_symbolic_total_overflows_int32(ctx, mode):
    A, B = _outer(46400, 46400)
    dA, dB = _dev(A), _dev(B)
    live = ctx.pool_stats()["live_blocks"]
    with pytest.raises(_lib.TsgError) as e:
        ctx.spgemm_symbolic(dA, dB, mode)
    assert e.value.rc == ERR_OVERFLOW
    assert e.value.info["nnzC"] == 46400 ** 2 == 2_152_960_000
    assert e.value.info["products"] == 46400 ** 2
    assert ctx.pool_stats()["live_blocks"] == live
    ctx.reset()


def test_symbolic_total_just_below_int32(ctx):
    """The largest outer product of a 46,340-column row that still fits int32:
    46,341 rows, nnz(C) = 2,147,441,940 <= 2^31 - 1 = 2,147,483,647, in count
    mode.  (The issue names 46,399 x 46,340 as this neighbour, but its
    2,150,129,660 lies above 2^31 - 1: that case is kept below as what it is, an
    overflow whose exact count is reported.)"""
    A, B = _outer(46341, 46340)
    c, info, _ = ctx.spgemm_symbolic(_dev(A), _dev(B), "count")
    assert info["nnzC"] == 46341 * 46340 == 2_147_441_940 <= 2 ** 31 - 1
    assert c.columnindex is None
    rp = ctx.to_host(c)[2]
    assert int(rp[-1]) == 46341 * 46340 == c.nnz
    np.testing.assert_array_equal(rp.astype(np.int64), np.arange(46342, dtype=np.int64) * 46340)
    ctx.reset()


def test_symbolic_total_46399_by_46340_is_past_int32(ctx):
    A, B = _outer(46399, 46340)
    assert 46399 * 46340 == 2_150_129_660 > 2 ** 31 - 1
    live = ctx.pool_stats()["live_blocks"]
    with pytest.raises(_lib.TsgError) as e:
        ctx.spgemm_symbolic(_dev(A), _dev(B), "count")
    assert e.value.rc == ERR_OVERFLOW and e.value.info["nnzC"] == 2_150_129_660
    assert ctx.pool_stats()["live_blocks"] == live


# ---------------------------------------------------------------- 10. validation
def _valid_pair():
    A = _csr(3, 4, [np.array([0, 3]), np.array([1]), np.array([2, 0])])
    B = _csr(4, 6, [np.array([5, 0]), np.array([1]), np.zeros(0), np.array([2, 3])])
    return A, B


def _broken(kind, which):
    A, B = _valid_pair()
    m, n, rp, ci = [A, B][which]
    rp, ci = rp.copy(), ci.copy()
    nnz = len(ci)
    if kind == "rp_decreasing":
        assert rp[1] < rp[2]
        rp[1], rp[2] = rp[2], rp[1]
    elif kind == "rp_end":
        rp[-1] -= 1
    elif kind == "rp_start":
        rp[0] = 1
    elif kind == "col_n":
        ci[1] = n
    elif kind == "col_neg":
        ci[0] = -1
    M = (m, n, rp, ci)
    return ((M, B) if which == 0 else (A, M)), nnz


@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
@pytest.mark.parametrize("kind", ["rp_decreasing", "rp_end", "rp_start", "col_n", "col_neg"])
def test_symbolic_validation(ctx, kind, which):
    (A, B), _ = _broken(kind, which)
    dA, dB = _dev(A), _dev(B)
    # (the struct keeps the true nnz: rp[m] != nnz is what rp_end tests)
    for d, M in ((dA, A), (dB, B)):
        assert d.nnz == len(M[3])
    live = ctx.pool_stats()["live_blocks"]
    for mode in ("pattern", "count"):
        with pytest.raises(_lib.TsgError) as e:
            ctx.spgemm_symbolic(dA, dB, mode)
        assert e.value.rc == ERR_INVALID
        assert ctx.pool_stats()["live_blocks"] == live
    Av, Bv = _valid_pair()
    _check(ctx, Av, Bv)


def test_symbolic_validation_shapes_and_mode(ctx):
    import ctypes as C
    A, B = _valid_pair()
    dA, dB = _dev(A), _dev(B)
    live = ctx.pool_stats()["live_blocks"]
    with pytest.raises(_lib.TsgError) as e:  # A.n != B.m
        ctx.spgemm_symbolic(dA, dA)
    assert e.value.rc == ERR_INVALID
    for mode in (2, -1, "neither"):
        with pytest.raises(_lib.TsgError) as e:
            ctx.spgemm_symbolic(dA, dB, mode)
        assert e.value.rc == ERR_INVALID
    # the output struct is zeroed on an error
    a, b, c = dA.struct(), dB.struct(), _lib.DevCSR(7, 7, 7, 1, 1, 1)
    rc = _lib.lib().tsg_dev_spgemm_symbolic(ctx.ptr, C.byref(a), C.byref(b), 9, None, C.byref(c), None, None)
    assert rc == ERR_INVALID
    assert (c.m, c.n, c.nnz, c.rowpointer, c.columnindex, c.value) == (0, 0, 0, None, None, None)
    assert ctx.pool_stats()["live_blocks"] == live
    _check(ctx, A, B)


# ---------------------------------------------------------------- 11. allocation failures
def _all_class_case():
    """a small operand with rows in all four classes (and one without products)"""
    rng = np.random.default_rng(77)
    n = 3 * W
    Brows = [np.sort(rng.choice(n, size=3 if i < 10 else 40, replace=False)) for i in range(2000)]
    B = _csr(2000, n, Brows)
    ks = [10, 100, 150, 1200, 1700]  # 400 / 4,000 / 6,000 / 48,000 / 68,000 products
    arows = [np.zeros(0), np.array([0]), np.array([1, 2, 3])]  # none / 3 / 9
    arows += [10 + np.sort(rng.choice(1990, size=k, replace=False)) for k in ks]
    A = _csr(len(arows), 2000, arows)
    return A, B


def test_symbolic_allocation_failures(ctx):
    A, B = _all_class_case()
    ref = _ref_scipy(A, B)
    info = _check(ctx, A, B, ref)
    assert all(c > 0 for c in info["rows_class"]), info
    dA, dB = _dev(A), _dev(B)
    before = ctx.pool_stats()
    ctx.spgemm_symbolic(dA, dB)
    ctx.reset()
    N = ctx.pool_stats()["allocs"] - before["allocs"]
    assert 8 <= N < 60
    live = ctx.pool_stats()["live_blocks"]
    for nth in range(N):
        assert ctx.fail_alloc(nth) is False
        with pytest.raises(_lib.TsgError) as e:
            ctx.spgemm_symbolic(dA, dB)
        assert e.value.rc == ERR_OOM, nth
        assert ctx.pool_stats()["live_blocks"] == live, nth
        assert ctx.fail_alloc(-1) is False, nth  # (it fired: nothing left pending)
    _check(ctx, A, B, ref)


# ---------------------------------------------------------------- 12. no product-sized memory
def test_symbolic_reserves_no_product_sized_memory():
    from spgemm_amd.device import Context
    cols = np.arange(0, 4000, 2)
    assert len(cols) == 2000
    A = _csr(64, 200, [np.arange(200)] * 64)
    B = _csr(200, 4000, [cols] * 200)
    c = Context(0)
    try:
        dA, dB = _dev(A), _dev(B)
        r0 = c.pool_stats()["reserved_bytes"]
        out, info, _ = c.spgemm_symbolic(dA, dB)
        grew = c.pool_stats()["reserved_bytes"] - r0
        assert info["products"] == 25_600_000 and info["nnzC"] == 128_000
        assert info["rows_class"] == [0, 0, 0, 64]
        _, _, rp, ci, _ = c.to_host(out)
        np.testing.assert_array_equal(rp, np.arange(65) * 2000)
        np.testing.assert_array_equal(ci, np.tile(cols, 64))
        assert grew <= 32 << 20, grew
    finally:
        c.close()


# ---------------------------------------------------------------- 13. plan from operands
def test_symbolic_plan_from_operands(ctx, mixed):
    import torch
    A, B, ref = mixed
    dA, dB = _dev(A), _dev(B)
    plan = ctx.spgemm_plan(dA, dB)
    ctx.reset()  # (the plan and its pattern survive)
    pat = plan.Cpattern
    assert pat.val is None
    np.testing.assert_array_equal(pat.rowptr.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(pat.col.cpu().numpy(), ref[1])
    rng = np.random.default_rng(99)
    av, bv = rng.uniform(-1, 1, len(A[3])), rng.uniform(-1, 1, len(B[3]))
    out = torch.full((len(ref[1]),), float("nan"), dtype=torch.float64, device="cuda")
    got, st = plan.run(torch.from_numpy(av).cuda(), torch.from_numpy(bv).cuda(), out=out)
    got = got.cpu().numpy()
    r = O.gustavson(O.OMat.from_csr(*A, av), O.OMat.from_csr(*B, bv)).csr()
    mag = O.gustavson(O.OMat.from_csr(*A, np.abs(av)), O.OMat.from_csr(*B, np.abs(bv))).csr()
    np.testing.assert_array_equal(r[2], ref[0])
    np.testing.assert_array_equal(r[3], ref[1])
    assert not np.isnan(got).any()
    assert np.all(np.abs(got - r[4]) <= 1e-10 * mag[4])
    assert st["path"] == T.PATH_NUMERIC
    plan.close()


# ---------------------------------------------------------------- 14. host layer
@pytest.mark.parametrize("name", ["x_int_unsorted_dup_77", "x_rect_50x130"])
def test_symbolic_host_layer(name):
    oA = O.OMat.load(os.path.join(FIXTURES, name + ".mtx"))
    m, n, rp, ci, vv = oA.csr()
    bm, bn, brp, bci, bvv = O.transpose(oA).csr()
    ref = _ref_oracle((m, n, rp, ci), (bm, bn, brp, bci))
    A, B = T.Matrix.from_csr(m, n, rp, ci, vv), T.Matrix.from_csr(bm, bn, brp, bci, bvv)
    Cm, st = T.spgemm_symbolic(A, B)
    cm, cn, crp, cci, cvv = Cm.csr()
    assert (cm, cn) == (m, bn) and len(cvv) == 0 and not Cm.s.value
    np.testing.assert_array_equal(crp, ref[0])
    np.testing.assert_array_equal(cci, ref[1])
    assert st["path"] == 6 and st["nnzC"] == len(ref[1])
    Cc, st = T.spgemm_symbolic(A, B, mode="count")
    _, _, crp, cci, cvv = Cc.csr()
    np.testing.assert_array_equal(crp, ref[0])
    assert len(cci) == 0 and len(cvv) == 0 and Cc.s.nnz == len(ref[1]) and st["path"] == 6
    with pytest.raises(_lib.TsgError) as e:
        T.spgemm_symbolic(A, B, mode=5)
    assert e.value.rc == ERR_INVALID


# ---------------------------------------------------------------- 15. operands untouched
def test_symbolic_leaves_operands_untouched_and_reads_no_values(ctx, mixed):
    A, B, ref = mixed
    nan_a, nan_b = np.full(len(A[3]), np.nan), np.full(len(B[3]), np.nan)
    dA, dB = _dev(A, nan_a), _dev(B, nan_b)
    before = [t.clone() for t in (dA.rowptr, dA.col, dB.rowptr, dB.col)]
    c, info, _ = ctx.spgemm_symbolic(dA, dB)
    _, _, rp, ci, vv = ctx.to_host(c)
    ctx.reset()
    assert vv is None
    np.testing.assert_array_equal(rp, ref[0])
    np.testing.assert_array_equal(ci, ref[1])
    import torch
    for t, b in zip((dA.rowptr, dA.col, dB.rowptr, dB.col), before):
        assert torch.equal(t, b)
    for t in (dA.val, dB.val):  # (still all NaN, bit for bit)
        assert bool(torch.isnan(t).all())
    assert info["nnzC"] == len(ref[1])
