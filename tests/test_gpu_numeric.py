"""Numeric-only SpGEMM on a known C pattern (tsg_dev_numeric_* / NumericPlan,
tsg_spgemm_csr_numeric) against the oracle's Gustavson product of the same
operands.  Every run draws fresh seeded uniform(-1, 1) values for A and B after
the pattern was made (stale values cannot pass), writes into a NaN-filled
c_val (an unwritten entry shows), and is held to the project's tolerance
|got - ref| <= 1e-10 * (|A| * |B|)."""
import glob
import os

import numpy as np
import pytest

from conftest import FIXTURES, GOLDEN
import _oracle as O
from _cases import numeric_mixed_case
from spgemm_amd import _lib, synth
from spgemm_amd import tilespgemm as T

pytestmark = pytest.mark.gpu

# the classes' caps (tsg_internal.h numeric_row_class): (len_C, products) of
# packed, wave, workgroup; the rest is split
CAPS = [(32, 512), (512, 8192), (4096, 65536)]
PACKED, WAVE, WORKGROUP, SPLIT = range(4)


@pytest.fixture(scope="module")
def ctx():
    from spgemm_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _csr(m, n, rows):
    """(m, n, rowptr, col) from a list of per-row column arrays, order kept"""
    lens = [len(c) for c in rows]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = (np.concatenate(rows) if sum(lens) else np.zeros(0)).astype(np.int32)
    return m, n, rp, ci


def _dev(M, val=None):
    from spgemm_amd.device import DeviceCSR
    m, n, rp, ci = M[:4]
    return DeviceCSR.from_host(m, n, rp, ci, np.ones(len(ci)) if val is None else val)


def _reference(A, B, av, bv):
    """oracle product of the valued operands: (rowptr, col, values, |A|*|B| values)"""
    oA, oB = O.OMat.from_csr(*A[:4], av), O.OMat.from_csr(*B[:4], bv)
    ref = O.gustavson(oA, oB).csr()
    mag = O.gustavson(O.OMat.from_csr(*A[:4], np.abs(av)), O.OMat.from_csr(*B[:4], np.abs(bv))).csr()
    np.testing.assert_array_equal(ref[3], mag[3])
    return ref[2], ref[3], ref[4], mag[4]


def _on_pattern(pat, ref):
    """the reference's values and magnitudes laid onto the pattern pat = (m, n,
    rowptr, col): (expected, magnitude, reached mask); the pattern must hold
    every reference entry"""
    m, n, prp, pci = pat[:4]
    rrp, rci, rv, rmag = ref
    pkey = np.repeat(np.arange(m, dtype=np.int64), np.diff(prp)) * n + pci
    rkey = np.repeat(np.arange(m, dtype=np.int64), np.diff(rrp)) * n + rci
    assert np.all(np.diff(pkey) > 0)
    pos = np.searchsorted(pkey, rkey)
    assert np.all(pos < len(pkey)) and np.all(pkey[pos] == rkey)
    exp, mag, reached = np.zeros(len(pkey)), np.zeros(len(pkey)), np.zeros(len(pkey), dtype=bool)
    exp[pos], mag[pos], reached[pos] = rv, rmag, True
    return exp, mag, reached


def _pattern_of(ctx, A, B):
    """C's pattern from a full spgemm of the operands (values 1.0), copied out
    of the context: (m, n, rowptr, col) on the host, DeviceCSR on the device"""
    dA, dB = _dev(A), _dev(B)
    c, _ = ctx.spgemm(dA, dB)
    dC = ctx.to_torch(c)
    ctx.reset()
    return (dC.m, dC.n, dC.rowptr.cpu().numpy(), dC.col.cpu().numpy()), dC


def _run_check(plan, A, B, pat, seed):
    import torch
    rng = np.random.default_rng(seed)
    av, bv = rng.uniform(-1, 1, len(A[3])), rng.uniform(-1, 1, len(B[3]))
    out = torch.full((len(pat[3]),), float("nan"), dtype=torch.float64, device="cuda")
    got, st = plan.run(torch.from_numpy(av).cuda(), torch.from_numpy(bv).cuda(), out=out)
    assert got.data_ptr() == out.data_ptr()
    got = got.cpu().numpy()
    exp, mag, reached = _on_pattern(pat, _reference(A, B, av, bv))
    assert not np.isnan(got).any()
    assert np.all(got[~reached] == 0.0)
    err = np.abs(got - exp)
    assert np.all(err <= 1e-10 * mag), float(np.max(err / np.maximum(mag, 1e-300)))
    assert st["path"] == T.PATH_NUMERIC == 4
    assert st["nnzCub"] == plan.info["products"] and st["nnzC"] == len(pat[3]) == plan.info["nnzC"]
    assert st["numtileA"] == -1 and st["numblkC"] == -1 and st["t_step1_ms"] == 0
    return reached


def _classes(A, B, pat):
    """per row: its class from the documented caps"""
    blen = np.diff(B[2].astype(np.int64))
    cum = np.concatenate([[0], np.cumsum(blen[A[3]])])
    P = cum[A[2][1:]] - cum[A[2][:-1]]
    lc = np.diff(pat[2])
    c = np.full(A[0], SPLIT)
    for i in range(len(CAPS) - 1, -1, -1):
        c[(lc <= CAPS[i][0]) & (P <= CAPS[i][1])] = i
    return c, P


def _plan_and_check(ctx, A, B, seeds=(1,), pat=None, dC=None):
    if pat is None:
        pat, dC = _pattern_of(ctx, A, B)
    dA, dB = _dev(A), _dev(B)
    plan = ctx.numeric_plan(dA, dB, dC)
    cls, P = _classes(A, B, pat)
    assert plan.info["rows_class"] == [int((cls == c).sum()) for c in range(4)]
    assert plan.info["products"] == int(P.sum())
    for s in seeds:
        _run_check(plan, A, B, pat, s)
    info = plan.info
    plan.close()
    return info


# ---------------------------------------------------------------- 1. fixtures
def _fixture_cases():
    out = []
    for p in sorted(glob.glob(os.path.join(FIXTURES, "*.mtx"))):
        name = os.path.basename(p)[:-4]
        square = "rect" not in name
        if square:
            out.append(pytest.param(p, False, id=name + "-AA"))
        out.append(pytest.param(p, True, id=name + "-AAT"))
    return out


@pytest.mark.parametrize("path,aat", _fixture_cases())
def test_numeric_fixtures(ctx, path, aat):
    oA = O.OMat.load(path)
    m, n, rp, ci, _ = oA.csr()
    assert aat or m == n
    A = (m, n, rp, ci)
    B = O.transpose(oA).csr()[:4] if aat else A
    info = _plan_and_check(ctx, A, B, seeds=(21, 22))  # (the second set of values on the same plan)
    if "unsorted" in path and not aat:
        assert info["b_rows_sorted"] == 0


def test_numeric_fixture_set_is_complete():
    names = {os.path.basename(p)[:-4] for p in glob.glob(os.path.join(FIXTURES, "*.mtx"))}
    assert {"x_int_unsorted_dup_77", "x_empty_rows_64", "x_dense_48"} <= names


# ---------------------------------------------------------------- 2. class binning
def test_numeric_mixed_classes(ctx):
    A, B = numeric_mixed_case()
    info = _plan_and_check(ctx, A, B, seeds=(5,))
    assert all(c > 0 for c in info["rows_class"]), info
    assert info["split_units"] > 0 and info["b_rows_sorted"] == 1


# ---------------------------------------------------------------- 3. cap edges
@pytest.mark.parametrize("cls", [PACKED, WAVE, WORKGROUP])
def test_numeric_len_cap_edges(ctx, cls):
    """rows of exactly cap and cap + 1 distinct columns against an identity B:
    len_C = P = L, so the pair straddles the class's len_C cap"""
    cap = CAPS[cls][0]
    n = 5000
    rng = np.random.default_rng(30 + cls)
    A = _csr(2, n, [np.sort(rng.choice(n, size=cap, replace=False)), np.sort(rng.choice(n, size=cap + 1, replace=False))])
    B = _csr(n, n, [np.array([i]) for i in range(n)])
    info = _plan_and_check(ctx, A, B, seeds=(3,))
    want = [0, 0, 0, 0]
    want[cls], want[cls + 1] = 1, 1
    assert info["rows_class"] == want
    assert info["nnzC"] == 2 * cap + 1 == info["products"]


@pytest.mark.parametrize("cls", [PACKED, WAVE, WORKGROUP])
def test_numeric_product_cap_edges(ctx, cls):
    """rows of exactly cap and cap + 1 products onto 8 columns: every referenced
    B row holds the same 8 columns (one more holds the first of them alone)"""
    cap = CAPS[cls][1]
    k = cap // 8
    A = _csr(2, k + 1, [np.arange(k), np.arange(k + 1)])
    B = _csr(k + 1, 40, [np.arange(3, 11)] * k + [np.array([3])])
    info = _plan_and_check(ctx, A, B, seeds=(4,))
    want = [0, 0, 0, 0]
    want[cls], want[cls + 1] = 1, 1
    assert info["rows_class"] == want
    assert info["nnzC"] == 16 and info["products"] == 2 * cap + 1


# ---------------------------------------------------------------- 4. split class
def _shuffled_rows(B, seed):
    """the same matrix with every row's entries in a random order"""
    m, n, rp, ci = B
    rng = np.random.default_rng(seed)
    out = ci.copy()
    for i in range(m):
        out[rp[i]:rp[i + 1]] = rng.permutation(ci[rp[i]:rp[i + 1]])
    return m, n, rp, out


def _split_case(kind):
    if kind == "products":  # 67,200 products (cap 65,536) onto 96 columns
        A = _csr(3, 700, [np.arange(700), np.array([5, 9]), np.zeros(0)])
        B = _csr(700, 300, [np.arange(100, 196)] * 700)
    elif kind == "len_c":  # len_C 8,200 (cap 4,096), 8,200 products
        A = _csr(2, 4100, [np.arange(4100), np.array([7])])
        B = _csr(4100, 10000, [np.array([i, i + 5000]) for i in range(4100)])
    else:  # "long_b_row": B rows longer than a split unit (4,096 products): cut into pieces
        rng = np.random.default_rng(8)
        A = _csr(2, 5, [np.arange(5), np.array([2])])
        B = _csr(5, 30000, [np.sort(rng.choice(30000, size=20000, replace=False)) for _ in range(5)])
    return A, B


@pytest.mark.parametrize("b_sorted", [True, False], ids=["sortedB", "unsortedB"])
@pytest.mark.parametrize("kind", ["products", "len_c", "long_b_row"])
def test_numeric_split_rows(ctx, kind, b_sorted):
    A, B = _split_case(kind)
    if not b_sorted:
        B = _shuffled_rows(B, 17)
    info = _plan_and_check(ctx, A, B, seeds=(6,))
    assert info["rows_class"][SPLIT] >= 1 and info["split_units"] >= 2
    assert info["b_rows_sorted"] == int(b_sorted)
    if kind == "products":
        assert info["products"] > 65536 and info["nnzC"] < 3 * 100
    if kind == "long_b_row":
        assert info["split_units"] >= 5 * 2


# ---------------------------------------------------------------- 4b. windowed wave rows
def _window_case():
    """wave-class rows (len_C <= 512, 1,024 <= P <= 8,192) whose columns span at
    most 2,048: the dense-window kernel.  Row 0: B rows longer than 128 entries
    (added straight to the window); row 1: runs of B rows with identical
    columns (summed in registers first), a different one between them; row 2:
    two lanes' worth (65..128 entries per B row)"""
    rng = np.random.default_rng(23)
    long_a = np.sort(rng.choice(np.arange(1000, 1400), size=200, replace=False))
    long_b = np.sort(rng.choice(np.arange(1100, 1500), size=200, replace=False))
    trip = np.sort(rng.choice(np.arange(3000, 3400), size=60, replace=False))
    other = np.sort(rng.choice(np.arange(3000, 3400), size=60, replace=False))
    two = np.sort(rng.choice(np.arange(5000, 5300), size=100, replace=False))
    two_b = np.sort(rng.choice(np.arange(5000, 5300), size=100, replace=False))
    Brows = [long_a] * 3 + [long_b] * 3 + [trip] * 9 + [other] + [trip] * 9 + [two] * 6 + [two_b] * 6
    B = _csr(len(Brows), 6000, Brows)
    A = _csr(4, len(Brows), [np.arange(0, 6), np.arange(6, 25), np.arange(25, 37), np.zeros(0)])
    return A, B


@pytest.mark.parametrize("b_sorted", [True, False], ids=["sortedB", "unsortedB"])
def test_numeric_window_rows(ctx, b_sorted):
    A, B = _window_case()
    if not b_sorted:
        B = _shuffled_rows(B, 19)
    info = _plan_and_check(ctx, A, B, seeds=(12, 13))
    assert info["rows_class"] == [1, 3, 0, 0] and info["products"] == 1200 + 19 * 60 + 1200


def test_numeric_window_row_reports_missing_column(ctx):
    import torch
    A, B = _window_case()
    pat, _ = _pattern_of(ctx, A, B)
    m, n, rp, ci = pat
    rng = np.random.default_rng(2)
    av = torch.from_numpy(rng.uniform(-1, 1, len(A[3]))).cuda()
    bv = torch.from_numpy(rng.uniform(-1, 1, len(B[3]))).cuda()
    for row, where in ((0, 5), (1, 0), (2, -1)):  # inside the window, its first column, its last
        drop = (rp[row] + where) if where >= 0 else (rp[row + 1] - 1)
        rp2 = rp.copy()
        rp2[row + 1:] -= 1
        plan = ctx.numeric_plan(_dev(A), _dev(B), _dev((m, n, rp2, np.delete(ci, drop))))
        assert plan.info["rows_class"] == [1, 3, 0, 0]
        _raises_invalid(lambda: plan.run(av, bv))
        plan.close()
    _plan_and_check(ctx, A, B, seeds=(14,))


# ---------------------------------------------------------------- 5. superset pattern
def test_numeric_superset_pattern(ctx):
    m = 300
    Am = synth.random_csr(m, m, density=0.02, seed=41)
    Bm = synth.random_csr(m, 400, density=0.02, seed=42)
    A, B = Am[:4], Bm[:4]
    # the pattern of (|A| + I) * B
    rows = [np.union1d(A[3][A[2][i]:A[2][i + 1]], [i]) for i in range(m)]
    A1 = _csr(m, m, rows)
    pat, dC = _pattern_of(ctx, A1, B)
    plan = ctx.numeric_plan(_dev(A), _dev(B), dC)
    reached = _run_check(plan, A, B, pat, 9)
    assert (~reached).sum() > 100 and reached.sum() > 100
    plan.close()


# ---------------------------------------------------------------- 6. rejected input
def _small_valid():
    Am = synth.random_csr(200, 150, density=0.05, seed=51)
    Bm = synth.random_csr(150, 180, density=0.05, seed=52)
    A, B = Am[:4], Bm[:4]
    ones = O.gustavson(O.OMat.from_csr(*A, np.ones(len(A[3]))), O.OMat.from_csr(*B, np.ones(len(B[3])))).csr()
    return A, B, (ones[0], ones[1], ones[2], ones[3])


def _raises_invalid(fn):
    with pytest.raises(_lib.TsgError) as ei:
        fn()
    assert ei.value.rc == -1  # TSG_ERR_INVALID


BAD_CASES = ["a_column_equal_n", "b_rowpointer_not_monotone", "c_column_equal_n", "c_descending_pair",
             "c_negative_column", "c_repeated_column", "c_rowpointer_end_huge", "c_rowpointer_end_not_nnz",
             "c_rowpointer_not_monotone", "c_rowpointer_start_not_zero", "shape_c_cols", "shape_c_rows",
             "shape_inner"]
_bad = {}


def _bad_patterns():
    if _bad:
        return _bad
    A, B, Cp = _small_valid()
    m, n, rp, ci = Cp
    row = int(np.argmax(np.diff(rp) >= 3))
    assert rp[row + 1] - rp[row] >= 3
    out = {}
    c = ci.copy()
    c[rp[row]], c[rp[row] + 1] = ci[rp[row] + 1], ci[rp[row]]
    out["c_descending_pair"] = (A, B, (m, n, rp, c))
    c = ci.copy()
    c[rp[row] + 1] = c[rp[row]]
    out["c_repeated_column"] = (A, B, (m, n, rp, c))
    c = ci.copy()
    c[rp[row + 1] - 1] = n
    out["c_column_equal_n"] = (A, B, (m, n, rp, c))
    c = ci.copy()
    c[rp[row]] = -1
    out["c_negative_column"] = (A, B, (m, n, rp, c))
    r = rp.copy()
    r[row + 1] = r[row] - 1 if r[row] > 0 else r[row + 2] + 1
    assert r[row + 1] < r[row] or r[row + 2] < r[row + 1]
    out["c_rowpointer_not_monotone"] = (A, B, (m, n, r, ci))
    r = rp.copy()
    r[m] = len(ci) - 1
    out["c_rowpointer_end_not_nnz"] = (A, B, (m, n, r, ci))
    r = rp.copy()
    r[0] = 1
    out["c_rowpointer_start_not_zero"] = (A, B, (m, n, r, ci))
    r = rp.copy()
    r[m] = 2 ** 30  # (far past the arrays: nothing may index with it)
    out["c_rowpointer_end_huge"] = (A, B, (m, n, r, ci))
    a = A[3].copy()
    a[0] = A[1]
    out["a_column_equal_n"] = ((A[0], A[1], A[2], a), B, Cp)
    r = B[2].copy()
    r[5], r[6] = r[6] + 1, r[5]
    out["b_rowpointer_not_monotone"] = (A, (B[0], B[1], r, B[3]), Cp)
    out["shape_c_rows"] = (A, B, (m + 1, n, np.append(rp, rp[-1]).astype(np.int32), ci))
    out["shape_c_cols"] = (A, B, (m, n + 1, rp, ci))
    out["shape_inner"] = ((A[0], A[1] + 1, A[2], A[3]), B, Cp)
    assert sorted(out) == BAD_CASES
    _bad.update(out)
    return _bad


@pytest.mark.parametrize("case", BAD_CASES)
def test_numeric_rejects_malformed_pattern(ctx, case):
    A, B, Cp = _bad_patterns()[case]
    dA, dB, dC = _dev(A), _dev(B), _dev(Cp)
    _raises_invalid(lambda: ctx.numeric_plan(dA, dB, dC))
    # the context is still usable
    A, B, Cp = _small_valid()
    _plan_and_check(ctx, A, B, seeds=(7,), pat=Cp, dC=_dev(Cp))


def test_numeric_run_reports_missing_column(ctx):
    import torch
    A, B, Cp = _small_valid()
    m, n, rp, ci = Cp
    row = int(np.argmax(np.diff(rp) >= 3))
    drop = rp[row] + 1  # a column A*B reaches (the pattern is exactly A*B's)
    rp2 = rp.copy()
    rp2[row + 1:] -= 1
    short = (m, n, rp2, np.delete(ci, drop))
    dA, dB, dC = _dev(A), _dev(B), _dev(short)
    plan = ctx.numeric_plan(dA, dB, dC)  # well-formed: only a run can tell
    rng = np.random.default_rng(1)
    av = torch.from_numpy(rng.uniform(-1, 1, len(A[3]))).cuda()
    bv = torch.from_numpy(rng.uniform(-1, 1, len(B[3]))).cuda()
    _raises_invalid(lambda: plan.run(av, bv))
    plan.close()
    _plan_and_check(ctx, A, B, seeds=(8,), pat=Cp, dC=_dev(Cp))


# ---------------------------------------------------------------- 7. lifetime
def test_numeric_plan_lifetime(ctx):
    A, B, Cp = _small_valid()
    dA, dB, dC = _dev(A), _dev(B), _dev(Cp)
    plan = ctx.numeric_plan(dA, dB, dC)
    # a full product of another matrix, then a reset: the plan's memory is its own
    m, n, rp, ci, vv = synth.random_csr(3000, 3000, density=0.003, seed=11)
    dM = _dev((m, n, rp, ci), vv)
    c, _ = ctx.spgemm(dM, dM)
    assert c.nnz > 0
    ctx.reset()
    _run_check(plan, A, B, Cp, 61)
    # two plans on one context, interleaved
    A2, B2 = (m, n, rp, ci), (m, n, rp, ci)
    pat2, dC2 = _pattern_of(ctx, A2, B2)
    plan2 = ctx.numeric_plan(dM, dM, dC2)
    for s in (62, 63):
        _run_check(plan2, A2, B2, pat2, s)
        ctx.reset()
        _run_check(plan, A, B, Cp, s + 10)
    plan.close()
    plan.close()  # (closing twice is harmless)
    _run_check(plan2, A2, B2, pat2, 64)
    plan3 = ctx.numeric_plan(dA, dB, dC)
    _run_check(plan3, A, B, Cp, 65)
    plan3.close()
    plan2.close()
    with pytest.raises(RuntimeError):
        plan2.run(None, None)


def test_numeric_context_close_takes_its_plans():
    from spgemm_amd.device import Context
    A, B, Cp = _small_valid()
    c2 = Context(0)
    plan = c2.numeric_plan(_dev(A), _dev(B), _dev(Cp))
    _run_check(plan, A, B, Cp, 66)
    c2.close()  # frees the plan with the context
    assert not plan.ptr
    plan.close()


# ---------------------------------------------------------------- 8. host layer
@pytest.mark.parametrize("name", ["x_powerlaw_400", "x_int_unsorted_dup_77"])
def test_numeric_host_layer(name):
    g = np.load(os.path.join(GOLDEN, "ref", name + "_aat0_16x16.npz"))
    A = (int(g["A__m"]), int(g["A__n"]), g["A__rowpointer"], g["A__columnindex"])
    B = (int(g["B__m"]), int(g["B__n"]), g["B__rowpointer"], g["B__columnindex"])
    pat = (A[0], B[1], g["C__rowpointer"], g["C__columnindex"])
    rng = np.random.default_rng(71)
    av, bv = rng.uniform(-1, 1, len(A[3])), rng.uniform(-1, 1, len(B[3]))
    Cm = T.Matrix.from_csr(*pat, np.full(len(pat[3]), np.nan))
    st = T.spgemm_numeric(T.Matrix.from_csr(*A, av), T.Matrix.from_csr(*B, bv), Cm)
    got = Cm.csr()
    np.testing.assert_array_equal(got[2], pat[2])
    np.testing.assert_array_equal(got[3], pat[3])
    exp, mag, reached = _on_pattern(pat, _reference(A, B, av, bv))
    assert reached.all() and not np.isnan(got[4]).any()
    assert np.all(np.abs(got[4] - exp) <= 1e-10 * mag)
    assert st["path"] == 4 and st["nnzCub"] == int(g["nnzCub"]) and st["nnzC"] == len(pat[3])
