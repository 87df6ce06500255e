"""Masked SpGEMM C<M> = A*B on the mask's pattern only (tsg_dev_masked_* /
MaskedPlan, tsg_spgemm_csr_masked) against the oracle's Gustavson product of
the same valued operands read at the mask's entries (0.0 where absent).  Every
run draws seeded uniform(-1, 1) values after its plan was made, writes into a
NaN-filled slice between two NaN guards of 64 doubles, and is held to the
project's tolerance |got - ref| <= 1e-10 * (|A| * |B|) at that entry, exactly
0.0 where no product reaches."""
import glob
import os

import numpy as np
import pytest

from conftest import FIXTURES, GOLDEN
import _oracle as O
from spgemm_amd import _lib, synth
from spgemm_amd import tilespgemm as T

pytestmark = pytest.mark.gpu

# tsg_internal.h: a dot unit's work and entries at most, the A rows copied to
# LDS, and the routing rule's cost of a dot step against a row-wise product
UNIT_WORK, UNIT_ENTRIES, ROW_LDS, DOT_COST = 4096, 256, 2048, 1
MODES = ("rows", "dot", "auto")
GUARD = 64


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


def _dev(M):
    from spgemm_amd.device import DeviceCSR
    m, n, rp, ci = M[:4]
    return DeviceCSR.from_host(m, n, rp, ci, np.ones(len(ci)))


def _keys(M):
    m, n, rp, ci = M[:4]
    return np.repeat(np.arange(m, dtype=np.int64), np.diff(rp)) * n + ci


def _from_keys(m, n, keys):
    """the CSR pattern (ascending columns) of a set of row * n + column keys"""
    keys = np.unique(np.asarray(keys, dtype=np.int64))
    rp = np.zeros(m + 1, dtype=np.int64)
    np.add.at(rp, keys // n + 1, 1)
    return m, n, np.cumsum(rp).astype(np.int32), (keys % n).astype(np.int32)


def _values(A, B, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, len(A[3])), rng.uniform(-1, 1, len(B[3]))


def _reference(A, B, av, bv):
    """oracle product of the valued operands: (sorted keys, values, |A|*|B| values)"""
    ref = O.gustavson(O.OMat.from_csr(*A[:4], av), O.OMat.from_csr(*B[:4], bv)).csr()
    mag = O.gustavson(O.OMat.from_csr(*A[:4], np.abs(av)), O.OMat.from_csr(*B[:4], np.abs(bv))).csr()
    np.testing.assert_array_equal(ref[3], mag[3])
    k = _keys(ref)
    order = np.argsort(k, kind="stable")
    return k[order], ref[4][order], mag[4][order]


def _at_mask(mask, ref):
    """the reference read at the mask's entries: (expected, magnitude, reached)"""
    rk, rv, rmag = ref
    mk = _keys(mask)
    exp, mag, reached = np.zeros(len(mk)), np.zeros(len(mk)), np.zeros(len(mk), dtype=bool)
    if len(rk) and len(mk):
        pos = np.minimum(np.searchsorted(rk, mk), len(rk) - 1)
        reached = rk[pos] == mk
        exp[reached], mag[reached] = rv[pos[reached]], rmag[pos[reached]]
    return exp, mag, reached


def _run(plan, av, bv):
    """one run into a NaN-filled slice between NaN guards: (values, stats)"""
    import torch
    n = plan.nnzM
    big = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    out = big[GUARD:GUARD + n]
    got, st = plan.run(torch.from_numpy(av).cuda(), torch.from_numpy(bv).cuda(), out=out)
    assert got.data_ptr() == out.data_ptr()
    host = big.cpu().numpy()
    assert np.isnan(host[:GUARD]).all() and np.isnan(host[GUARD + n:]).all(), "a guard was written"
    assert st["path"] == T.PATH_MASKED == 5
    assert st["nnzCub"] == plan.info["products"] and st["nnzC"] == n == plan.info["nnzM"]
    assert st["numtileA"] == -1 and st["numblkC"] == -1 and st["t_step1_ms"] == 0
    return host[GUARD:GUARD + n].copy(), st


def _check(got, mask, ref):
    exp, mag, reached = _at_mask(mask, ref)
    assert not np.isnan(got).any(), int(np.isnan(got).sum())
    assert np.all(got[~reached] == 0.0)
    err = np.abs(got - exp)
    assert np.all(err <= 1e-10 * mag), float(np.max(err / np.maximum(mag, 1e-300)))
    return reached


def _raises_invalid(fn):
    with pytest.raises(_lib.TsgError) as ei:
        fn()
    assert ei.value.rc == -1  # TSG_ERR_INVALID


# ------------------------------------------------- the documented rules in numpy
def _lens_t(B):
    return np.bincount(B[3], minlength=B[1]).astype(np.int64)


def _row_sums(rp, x):
    cum = np.concatenate([[0], np.cumsum(x)])
    return cum[rp[1:]] - cum[rp[:-1]]


def _row_stats(A, B, mask):
    """per row: element products P, dot work D, mask entries; per mask entry: its work"""
    blen = np.diff(B[2].astype(np.int64))
    P = _row_sums(A[2], blen[A[3]])
    la = np.diff(A[2].astype(np.int64))
    lm = np.diff(mask[2].astype(np.int64))
    w = np.minimum(np.repeat(la, lm), _lens_t(B)[mask[3]])
    return P, _row_sums(mask[2], w), lm, w


def _eligible(A, B):
    def strictly(M):
        m, n, rp, ci = M[:4]
        if len(ci) < 2:
            return True
        d = np.diff(ci.astype(np.int64)) > 0
        d[rp[1:-1][(rp[1:-1] > 0) & (rp[1:-1] < len(ci))] - 1] = True  # (pairs across a row boundary)
        return bool(d.all())
    bk = _keys(B)
    return strictly(A), len(np.unique(bk)) == len(bk)


def _routing(A, B, mask, mode):
    """what the plan's info must say, from the documented rule and constants"""
    P, D, lm, w = _row_stats(A, B, mask)
    a_sorted, no_rep = _eligible(A, B)
    elig = a_sorted and no_rep
    has = lm > 0
    if mode == "dot":  # (needs elig: the caller expects TSG_ERR_INVALID otherwise)
        dot = has
    elif mode == "auto" and elig:
        dot = has & (DOT_COST * D < P)
    else:
        dot = np.zeros(len(P), dtype=bool)
    units = 0
    rp = mask[2]
    for i in np.flatnonzero(dot):
        cur = cnt = 0
        for x in w[rp[i]:rp[i + 1]]:
            if cnt > 0 and (cur + x > UNIT_WORK or cnt == UNIT_ENTRIES):
                units += 1
                cur = cnt = 0
            cnt += 1
            cur += int(x)
        units += cnt > 0
    return dict(products=int(P.sum()), nnzM=len(mask[3]), rows_rowwise=int((has & ~dot).sum()),
                rows_dot=int(dot.sum()), products_rowwise=int(P[has & ~dot].sum()), dot_work=int(D[dot].sum()),
                dot_units=int(units), a_rows_sorted=int(a_sorted), b_no_repeats=int(no_rep), dot_eligible=int(elig))


def _info_matches(info, want):
    for k, v in want.items():
        assert info[k] == v, (k, info[k], v)


def _plan(ctx, dA, dB, A, B, mask, mode):
    """the plan, or None for dot mode on operands the dot leg cannot take (then
    creation must raise TSG_ERR_INVALID)"""
    dM = _dev(mask)
    if mode == "dot" and not all(_eligible(A, B)):
        _raises_invalid(lambda: ctx.masked_plan(dA, dB, dM, mode=mode))
        return None
    plan = ctx.masked_plan(dA, dB, dM, mode=mode)
    _info_matches(plan.info, _routing(A, B, mask, mode))
    return plan


# ---------------------------------------------------------------- 1. fixtures
def _fixture_cases():
    out = []
    for p in sorted(glob.glob(os.path.join(FIXTURES, "*.mtx"))):
        name = os.path.basename(p)[:-4]
        if "rect" not in name:
            out.append(pytest.param(p, False, id=name + "-AA"))
        out.append(pytest.param(p, True, id=name + "-AAT"))
    return out


def _masks(A, B, full, square, seed):
    m, n = A[0], B[1]
    rng = np.random.default_rng(seed)
    fk = _keys(full)
    out = {}
    if square:
        out["own"] = _from_keys(m, n, _keys(A))
    out["full"] = _from_keys(m, n, fk)
    half = fk[rng.random(len(fk)) < 0.5]
    extra = np.setdiff1d(rng.integers(0, max(m * n, 1), size=max(8, len(fk) // 4)), fk) if m * n else fk[:0]
    out["half_plus_outside"] = _from_keys(m, n, np.concatenate([half, extra]))
    d = np.arange(min(m, n), dtype=np.int64)
    out["diagonal"] = _from_keys(m, n, d * n + d)
    out["every_second_row_empty"] = _from_keys(m, n, fk[(fk // n) % 2 == 0])
    out["empty"] = _from_keys(m, n, fk[:0])
    return out


@pytest.mark.parametrize("path,aat", _fixture_cases())
def test_masked_fixtures(ctx, path, aat):
    import torch
    oA = O.OMat.load(path)
    m, n, rp, ci, _ = oA.csr()
    A = (m, n, rp, ci)
    B = O.transpose(oA).csr()[:4] if aat else A
    dA, dB = _dev(A), _dev(B)
    ones = O.gustavson(O.OMat.from_csr(*A, np.ones(len(A[3]))), O.OMat.from_csr(*B, np.ones(len(B[3])))).csr()
    masks = _masks(A, B, ones[:4], m == n and not aat, 100)
    plans = {(k, mode): _plan(ctx, dA, dB, A, B, mask, mode) for k, mask in masks.items() for mode in MODES}
    av, bv = _values(A, B, 101)  # (after the plans were made)
    ref = _reference(A, B, av, bv)
    for (k, mode), plan in plans.items():
        if plan is None:
            continue
        got, _ = _run(plan, av, bv)
        reached = _check(got, masks[k], ref)
        if k == "full":
            assert reached.all() and len(got) == len(ref[0])
            if mode == "rows":  # the numeric plan on the same pattern and values
                nplan = ctx.numeric_plan(dA, dB, _dev(masks[k]))
                nv, _ = nplan.run(torch.from_numpy(av).cuda(), torch.from_numpy(bv).cuda())
                nplan.close()
                assert np.all(np.abs(nv.cpu().numpy() - got) <= 1e-10 * _at_mask(masks[k], ref)[1])
        if k == "empty":
            assert len(got) == 0
        plan.close()


# ---------------------------------------------------------------- 2, 3, 5. the R-MAT operand
_rmat = {}


def _rmat_case():
    if not _rmat:
        m, n, rp, ci, _ = synth.rmat(scale_n=20_000)
        A = (m, n, rp.astype(np.int32), ci.astype(np.int32))
        _rmat["A"] = A
        k = _keys(A)
        _rmat["L"] = _from_keys(m, n, k[k % n < k // n])  # strict lower triangle (the generator removed duplicates)
    return _rmat


def _rmat_ref():
    """values and reference of the R-MAT A*A (computed once; the plans exist by then)"""
    c = _rmat_case()
    if "ref" not in c:
        c["av"], c["bv"] = _values(c["A"], c["A"], 201)
        c["ref"] = _reference(c["A"], c["A"], c["av"], c["bv"])
    return c["av"], c["bv"], c["ref"]


def test_masked_legs_agree_and_dot_is_reproducible(ctx):
    A = _rmat_case()["A"]
    dA = _dev(A)
    rows, dot = _plan(ctx, dA, dA, A, A, A, "rows"), _plan(ctx, dA, dA, A, A, A, "dot")
    av, bv, ref = _rmat_ref()
    g_rows, _ = _run(rows, av, bv)
    g_dot, _ = _run(dot, av, bv)
    g_dot2, _ = _run(dot, av, bv)
    _check(g_rows, A, ref)
    _check(g_dot, A, ref)
    mag = _at_mask(A, ref)[1]
    assert np.all(np.abs(g_rows - g_dot) <= 1e-10 * mag)
    assert g_dot.tobytes() == g_dot2.tobytes()  # bitwise
    rows.close()
    dot.close()


@pytest.mark.parametrize("mode", MODES)
def test_masked_triangle_count(ctx, mode):
    import scipy.sparse as sp
    L = _rmat_case()["L"]
    m, n, rp, ci = L
    ones = np.ones(len(ci))
    S = sp.csr_matrix((ones, ci, rp), shape=(m, n))
    want = (S @ S).multiply(S).sum()
    dL = _dev(L)
    plan = _plan(ctx, dL, dL, L, L, L, mode)
    got, _ = _run(plan, ones, ones)
    plan.close()
    assert want > 0 and got.sum() == want  # (small integers: exact in fp64)


def test_masked_routing(ctx):
    A = _rmat_case()["A"]
    dA = _dev(A)
    plan = _plan(ctx, dA, dA, A, A, A, "auto")  # (checks the info against the rule)
    assert plan.info["rows_dot"] > 0 and plan.info["rows_rowwise"] > 0, plan.info
    av, bv, ref = _rmat_ref()
    got, _ = _run(plan, av, bv)
    _check(got, A, ref)
    plan.close()


# ---------------------------------------------------------------- 4. dot-kernel edges
def _edge_case():
    """B: 6,000 x 600 with columns (B^T rows) of 1, 16, 17 and 5,000 entries and
    a hundred of 80; A: rows of 0, 1, 16, 17, kMskRowLds, kMskRowLds + 1 and
    5,000 entries, and rows of 64 entries for the unit cuts"""
    rng = np.random.default_rng(77)
    K, N = 6000, 600
    clen = np.concatenate([[1, 16, 17, 5000], rng.integers(1, 40, 96), np.full(100, 80), rng.integers(1, 40, 400)])
    assert len(clen) == N
    bk = np.concatenate([np.sort(rng.choice(K, size=c, replace=False)).astype(np.int64) * N + j
                         for j, c in enumerate(clen)])
    B = _from_keys(K, N, bk)
    assert np.array_equal(_lens_t(B), clen)
    alen = [0, 1, 16, 17, ROW_LDS, ROW_LDS + 1, 5000, 8, 8, 64, 64, 64, 0]
    A = _csr(len(alen), K, [np.sort(rng.choice(K, size=c, replace=False)) for c in alen])
    some = lambda k: np.union1d([0, 1, 2, 3], rng.choice(N, size=k, replace=False))
    w80 = np.arange(100, 200)  # the columns of 80 entries: work min(64, 80) = 64 against the 64-entry rows
    mrows = [some(30) for _ in range(7)]                       # rows 0..6: the A-row lengths; row 6 x column 3: the
    #                                                            single entry past kMskUnitWork on both sides
    mrows += [np.sort(rng.choice(N, size=UNIT_ENTRIES, replace=False)),       # row 7: exactly kMskUnitEntries
              np.sort(rng.choice(N, size=UNIT_ENTRIES + 1, replace=False)),   # row 8: one more
              w80[:64],                                        # row 9: 64 * 64 = kMskUnitWork exactly
              np.concatenate([[0], w80[:64]]),                 # row 10: 1 + 64 * 64: one more
              w80[:65],                                        # row 11: 65 * 64
              np.array([5, 9])]                                # row 12: mask entries, empty A row
    mask = _csr(len(alen), N, mrows)
    return A, B, mask


def test_masked_dot_kernel_edges(ctx):
    A, B, mask = _edge_case()
    P, D, lm, w = _row_stats(A, B, mask)
    rp = mask[2]
    assert w[rp[6]:rp[7]].max() == 5000 > UNIT_WORK
    assert D[9] == UNIT_WORK and D[10] == UNIT_WORK + 1 and lm[7] == UNIT_ENTRIES and lm[8] == UNIT_ENTRIES + 1
    want = _routing(A, B, mask, "dot")
    assert want["rows_dot"] == 13 and want["dot_units"] > 13 + 4  # (rows 6, 8, 10, 11 and the heavy entry cut)
    dA, dB = _dev(A), _dev(B)
    plan = _plan(ctx, dA, dB, A, B, mask, "dot")  # (dot_units against the rule in numpy)
    av, bv = _values(A, B, 301)
    ref = _reference(A, B, av, bv)
    got, _ = _run(plan, av, bv)
    reached = _check(got, mask, ref)
    assert reached.sum() > 50 and not reached[rp[0]:rp[1]].any() and not reached[rp[12]:rp[13]].any()
    plan.close()
    for mode in ("rows", "auto"):
        plan = _plan(ctx, dA, dB, A, B, mask, mode)
        _check(_run(plan, av, bv)[0], mask, ref)
        plan.close()


# ---------------------------------------------------------------- 6. ineligible operands
def _small():
    A = synth.random_csr(200, 150, density=0.05, seed=51)[:4]
    B = synth.random_csr(150, 180, density=0.05, seed=52)[:4]
    A = (A[0], A[1], A[2].astype(np.int32), A[3].astype(np.int32))
    B = (B[0], B[1], B[2].astype(np.int32), B[3].astype(np.int32))
    ones = O.gustavson(O.OMat.from_csr(*A, np.ones(len(A[3]))), O.OMat.from_csr(*B, np.ones(len(B[3])))).csr()
    rng = np.random.default_rng(53)
    fk = _keys(ones)
    mask = _from_keys(A[0], B[1], np.concatenate([fk[rng.random(len(fk)) < 0.6],
                                                  rng.integers(0, A[0] * B[1], size=500)]))
    return A, B, mask


@pytest.mark.parametrize("kind", ["a_unsorted_row", "b_repeated_column"])
def test_masked_ineligible_operands(ctx, kind):
    A, B, mask = _small()
    if kind == "a_unsorted_row":
        row = int(np.argmax(np.diff(A[2]) >= 3))
        ci = A[3].copy()
        ci[A[2][row]], ci[A[2][row] + 1] = A[3][A[2][row] + 1], A[3][A[2][row]]
        A = (A[0], A[1], A[2], ci)
    else:
        row = int(np.argmax(np.diff(B[2]) >= 3))
        at = B[2][row] + 1
        rp = B[2].copy()
        rp[row + 1:] += 1
        B = (B[0], B[1], rp, np.insert(B[3], at, B[3][at]))  # (a column twice in one row)
    assert all(_eligible(A, B)) is False
    dA, dB = _dev(A), _dev(B)
    auto = _plan(ctx, dA, dB, A, B, mask, "auto")
    assert auto.info["dot_eligible"] == 0 and auto.info["rows_dot"] == 0 and auto.info["dot_units"] == 0
    assert (auto.info["a_rows_sorted"], auto.info["b_no_repeats"]) == ((0, 1) if kind == "a_unsorted_row" else (1, 0))
    av, bv = _values(A, B, 61)
    _check(_run(auto, av, bv)[0], mask, _reference(A, B, av, bv))  # (the oracle sums the repeats)
    auto.close()
    assert _plan(ctx, dA, dB, A, B, mask, "dot") is None  # (raised TSG_ERR_INVALID)


# ---------------------------------------------------------------- 7. validation, error contract
def _bad_masks():
    A, B, mask = _small()
    m, n, rp, ci = mask
    row = int(np.argmax(np.diff(rp) >= 3))
    out = {}
    c = ci.copy()
    c[rp[row]], c[rp[row] + 1] = ci[rp[row] + 1], ci[rp[row]]
    out["unsorted_mask_row"] = (m, n, rp, c)
    c = ci.copy()
    c[rp[row + 1] - 1] = n
    out["mask_column_equal_n"] = (m, n, rp, c)
    r = rp.copy()
    r[m] = len(ci) - 1
    out["rowpointer_end_not_nnz"] = (m, n, r, ci)
    out["wrong_shape_rows"] = (m + 1, n, np.append(rp, rp[-1]).astype(np.int32), ci)
    out["wrong_shape_cols"] = (m, n + 1, rp, ci)
    return A, B, mask, out


@pytest.mark.parametrize("case", ["unsorted_mask_row", "mask_column_equal_n", "rowpointer_end_not_nnz",
                                  "wrong_shape_rows", "wrong_shape_cols", "mode_7"])
def test_masked_rejects_malformed_input(ctx, case):
    A, B, mask, bad = _bad_masks()
    dA, dB = _dev(A), _dev(B)
    ctx.reset()
    before = ctx.pool_stats()["live_blocks"]
    for mode in (MODES if case != "mode_7" else (7,)):
        dM = _dev(bad.get(case, mask))
        _raises_invalid(lambda: ctx.masked_plan(dA, dB, dM, mode=mode))
        assert ctx.pool_stats()["live_blocks"] == before
    # the context is still usable
    plan = _plan(ctx, dA, dB, A, B, mask, "auto")
    av, bv = _values(A, B, 62)
    _check(_run(plan, av, bv)[0], mask, _reference(A, B, av, bv))
    plan.close()


@pytest.mark.parametrize("mode", ["auto", "dot"])
def test_masked_failed_allocation_leaks_nothing(mode):
    from spgemm_amd.device import Context
    A, B, mask = _small()
    c2 = Context(0)
    try:
        dA, dB, dM = _dev(A), _dev(B), _dev(mask)
        failed = 0
        for k in range(1000):
            assert not c2.fail_alloc(k)
            try:
                plan = c2.masked_plan(dA, dB, dM, mode=mode)
            except _lib.TsgError as e:
                assert e.rc == -3, (k, e.rc)  # TSG_ERR_OOM
                assert not c2.fail_alloc(-1)  # (it fired)
                assert c2.pool_stats()["live_blocks"] == 0, k
                failed += 1
                continue
            assert c2.fail_alloc(-1)  # still pending: creation makes k allocations
            break
        else:
            pytest.fail("creation never succeeded")
        assert failed == k > 0
        assert c2.pool_stats()["live_blocks"] == 0  # (a plan's memory is not the pool's)
        av, bv = _values(A, B, 63)
        _check(_run(plan, av, bv)[0], mask, _reference(A, B, av, bv))
        plan.close()
    finally:
        c2.close()


# ---------------------------------------------------------------- 8. lifetime
def test_masked_plan_lifetime(ctx):
    A, B, mask = _small()
    dA, dB = _dev(A), _dev(B)
    plan = _plan(ctx, dA, dB, A, B, mask, "dot")
    auto = _plan(ctx, dA, dB, A, B, mask, "auto")
    # a full product of another matrix, then a reset: the plans' memory is their own
    m, n, rp, ci, vv = synth.random_csr(3000, 3000, density=0.003, seed=11)
    from spgemm_amd.device import DeviceCSR
    dM = DeviceCSR.from_host(m, n, rp, ci, vv)
    c, _ = ctx.spgemm(dM, dM)
    assert c.nnz > 0
    ctx.reset()
    av, bv = _values(A, B, 64)
    ref = _reference(A, B, av, bv)
    _check(_run(plan, av, bv)[0], mask, ref)
    _check(_run(auto, av, bv)[0], mask, ref)
    plan.close()
    plan.close()  # (closing twice is harmless)
    _check(_run(auto, av, bv)[0], mask, ref)
    auto.close()
    with pytest.raises(RuntimeError):
        plan.run(None, None)


def test_masked_context_close_takes_its_plans():
    from spgemm_amd.device import Context
    A, B, mask = _small()
    c2 = Context(0)
    plan = c2.masked_plan(_dev(A), _dev(B), _dev(mask), mode="dot")
    av, bv = _values(A, B, 65)
    _check(_run(plan, av, bv)[0], mask, _reference(A, B, av, bv))
    c2.close()  # frees the plan with the context
    assert not plan.ptr
    plan.close()


# ---------------------------------------------------------------- 9. host layer
@pytest.mark.parametrize("mode", MODES)
def test_masked_host_layer(mode):
    g = np.load(os.path.join(GOLDEN, "ref", "x_powerlaw_400_aat0_16x16.npz"))
    A = (int(g["A__m"]), int(g["A__n"]), g["A__rowpointer"], g["A__columnindex"])
    B = (int(g["B__m"]), int(g["B__n"]), g["B__rowpointer"], g["B__columnindex"])
    mask = _from_keys(A[0], A[1], _keys(A))  # the operand's own pattern
    av, bv = _values(A, B, 71)
    Cm = T.Matrix.from_csr(*mask, np.full(len(mask[3]), np.nan))
    st = T.spgemm_masked(T.Matrix.from_csr(*A, av), T.Matrix.from_csr(*B, bv), Cm, mode)
    got = Cm.csr()
    np.testing.assert_array_equal(got[2], mask[2])
    np.testing.assert_array_equal(got[3], mask[3])
    _check(got[4], mask, _reference(A, B, av, bv))
    assert st["path"] == 5 and st["nnzCub"] == int(g["nnzCub"]) and st["nnzC"] == len(mask[3])
