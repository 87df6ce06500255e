"""Element-wise union, intersection and difference of CSR matrices
(tsg_dev_ewise / Context.ewise, Context.spgemm_accum, tsg_ewise_csr).  The
expected results come from numpy on row * n + column keys (union1d, intersect1d,
setdiff1d) and numpy's separately rounded alpha * a, beta * b and op; every
comparison of row pointers, columns and values is exact."""
import ctypes as C
import fractions
import functools
import os

import numpy as np
import pytest

from conftest import FIXTURES
from spgemm_amd import _lib, synth
from spgemm_amd import tilespgemm as T

pytestmark = pytest.mark.gpu

PACKED_CAP, WAVE_CAP, TILE = 32, 512, 2048  # (kEwisePackedLen, kEwiseWaveLen, kEwiseTile of tsg_internal.h)
ERR_INVALID, ERR_OOM = -1, -3
MODES = ("union", "intersect", "difference")
OPS = {"plus": np.add, "times": np.multiply, "min": np.fmin, "max": np.fmax, "first": lambda x, y: x,
       "second": lambda x, y: y}
SCALARS = ((1.0, 1.0), (2.5, -1.0), (1.0 / 3.0, 1e-3))


@pytest.fixture(scope="module")
def ctx():
    from spgemm_amd.device import Context
    c = Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- helpers
def _csr(m, n, rows):
    rows = [np.asarray(r, dtype=np.int64) for r in rows]
    assert len(rows) == m
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = (np.concatenate(rows) if m else np.zeros(0)).astype(np.int32)
    return m, n, rp, ci


def _dev(M, val=None):
    """the pattern on the device, without values unless val is given"""
    import torch
    from spgemm_amd.device import DeviceCSR
    m, n, rp, ci = M[:4]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    return DeviceCSR(m, n, t(rp, np.int32), t(ci, np.int32), None if val is None else t(val, np.float64))


def _keys(rp, ci, n):
    """row * n + column of every entry (ascending for a pattern with sorted rows)"""
    rows = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp.astype(np.int64)))
    return rows * n + ci.astype(np.int64)


def _from_keys(m, n, keys):
    keys = np.unique(np.asarray(keys, dtype=np.int64))
    rp = np.concatenate([[0], np.cumsum(np.bincount(keys // n, minlength=m))]).astype(np.int32)
    return m, n, rp, (keys % n).astype(np.int32)


def _expect(A, B, mode, op="plus", alpha=1.0, beta=1.0, av=None, bv=None):
    """(rowptr, col, values or None, both) by numpy"""
    m, n = A[:2]
    ka, kb = _keys(A[2], A[3], n), _keys(B[2], B[3], n)
    k = {"union": np.union1d, "intersect": np.intersect1d, "difference": np.setdiff1d}[mode](ka, kb)
    both = len(np.intersect1d(ka, kb))
    _, _, rp, ci = _from_keys(m, n, k)
    if av is None:
        return rp, ci, None, both
    xa = np.float64(alpha) * av  # (each rounded once)
    in_a, in_b = np.isin(k, ka), np.isin(k, kb)
    ia = np.minimum(np.searchsorted(ka, k), max(len(ka) - 1, 0))
    ib = np.minimum(np.searchsorted(kb, k), max(len(kb) - 1, 0))
    va = xa[ia] if len(ka) else np.zeros(len(k))
    if mode == "difference":
        return rp, ci, va, both
    if bv is None:  # (only where the op reads no b: first under intersect)
        assert mode == "intersect" and op == "first"
        return rp, ci, va, both
    yb = np.float64(beta) * bv
    vb = yb[ib] if len(kb) else np.zeros(len(k))
    vv = np.where(in_a & in_b, OPS[op](va, vb), np.where(in_a, va, vb))
    return rp, ci, vv, both


def _run(ctx, A, B, mode, op="plus", alpha=1.0, beta=1.0, av=None, bv=None, dA=None, dB=None):
    """(rowptr, col, values or None, info, stats) of a call, copied to the host"""
    c, info, st = ctx.ewise(dA if dA is not None else _dev(A, av), dB if dB is not None else _dev(B, bv), mode, op,
                            alpha, beta)
    assert c.m == A[0] and c.n == A[1]
    _, _, rp, ci, vv = ctx.to_host(c)
    assert rp[0] == 0 and rp[-1] == c.nnz == info["nnzC"] == st["nnzC"]
    assert st["path"] == T.PATH_EWISE == 7 and st["nnzCub"] == info["nnzA"] + info["nnzB"] == len(A[3]) + len(B[3])
    assert bool(c.columnindex) == (c.nnz > 0)
    assert bool(c.value) == (c.nnz > 0 and av is not None)
    ctx.reset()
    return rp, ci, (vv if av is not None else None), info, st


def _check(ctx, A, B, mode, op="plus", alpha=1.0, beta=1.0, av=None, bv=None):
    wrp, wci, wvv, both = _expect(A, B, mode, op, alpha, beta, av, bv)
    rp, ci, vv, info, st = _run(ctx, A, B, mode, op, alpha, beta, av, bv)
    np.testing.assert_array_equal(rp, wrp, err_msg=f"{mode} {op}")
    np.testing.assert_array_equal(ci, wci, err_msg=f"{mode} {op}")
    assert info["both"] == both and info["nnzC"] == len(wci)
    if av is not None:
        assert vv is not None and vv.tobytes() == wvv.tobytes(), (mode, op, alpha, beta)
    return info


def _values(M, seed):
    """random fp64 values; odd seeds (the A operands') with stored zeros, which are entries like any other
    (in one operand only: min / max of a 0.0 and a -0.0 would be unspecified)"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(len(M[3])) * np.exp(rng.uniform(-3, 3, len(M[3])))
    if seed % 2:
        v[::7] = 0.0
    return v


# ---------------------------------------------------------------- 1. class edges
EDGE_LENS = [0, 1, 2, 31, 32, 33, 511, 512, 513, 2047, 2048, 2049, 4096, 4097, 3 * 2048 + 1]
EDGE_N = 20000


@functools.lru_cache(maxsize=None)
def _edge_case():
    """one row per (L, split of L between A and B, overlap of the two rows)"""
    rng = np.random.default_rng(12)
    arows, brows, lens = [], [], []
    for L in EDGE_LENS:
        for la, lb in ((L, 0), (0, L), (-(-L // 2), L // 2), (max(L - 1, 0), min(1, L))):
            for overlap in ("none", "all", "half"):
                small = min(la, lb)
                common = {"none": 0, "all": small, "half": small // 2}[overlap]
                cols = rng.choice(EDGE_N, size=la + lb - common, replace=False)
                shared, rest = cols[:common], cols[common:]
                a = np.sort(np.concatenate([shared, rest[:la - common]]))
                b = np.sort(np.concatenate([shared, rest[la - common:]]))
                assert len(a) == la and len(b) == lb and len(np.intersect1d(a, b)) == common
                arows.append(a)
                brows.append(b)
                lens.append(L)
    m = len(lens)
    return _csr(m, EDGE_N, arows), _csr(m, EDGE_N, brows), np.array(lens)


def _edge_classes(lens):
    packed = int(((lens >= 1) & (lens <= PACKED_CAP)).sum())
    wave = int(((lens > PACKED_CAP) & (lens <= WAVE_CAP)).sum())
    tile = lens[lens > WAVE_CAP]
    return [packed, wave, len(tile)], int((-(-tile // TILE)).sum())


@pytest.mark.parametrize("valued", [False, True], ids=["structural", "valued"])
@pytest.mark.parametrize("mode", MODES)
def test_ewise_class_edges(ctx, mode, valued):
    A, B, lens = _edge_case()
    av, bv = (_values(A, 1), _values(B, 2)) if valued else (None, None)
    info = _check(ctx, A, B, mode, "plus", 1.0, 1.0, av, bv)
    classes, units = _edge_classes(lens)
    assert info["rows_class"] == classes and info["units"] == units
    assert all(c > 0 for c in classes) and sum(classes) == int((lens > 0).sum())


# ---------------------------------------------------------------- 2. merge-path cuts
CUT_N = 40000


def _cut_pairs():
    ar = np.arange
    out = {"equal": (ar(10000), ar(10000)), "evens_odds": (ar(0, 20000, 2), ar(1, 20000, 2)),
           "a_below_b": (ar(0, 7000), ar(20000, 26000)), "b_below_a": (ar(20000, 26000), ar(0, 7000))}
    for k in range(2046, 2051):
        out[f"shift{k}"] = (ar(0, 6000), ar(k, k + 6000))
    for seed in range(3):
        rng = np.random.default_rng(100 + seed)
        out[f"random{seed}"] = (np.sort(rng.choice(CUT_N, size=int(rng.integers(3000, 15000)), replace=False)),
                                np.sort(rng.choice(CUT_N, size=int(rng.integers(3000, 15000)), replace=False)))
    return out


@pytest.mark.parametrize("name", list(_cut_pairs()))
def test_ewise_merge_path_cuts(ctx, name):
    """one long row cut into units (and the same row eight times: units of
    different rows in one launch); a pair a == b at or beside every cut"""
    a, b = _cut_pairs()[name]
    for reps in (1, 8):
        A, B = _csr(reps, CUT_N, [a] * reps), _csr(reps, CUT_N, [b] * reps)
        av, bv = _values(A, 3), _values(B, 4)
        units = reps * -(-(len(a) + len(b)) // TILE)
        for mode in MODES:
            info = _check(ctx, A, B, mode)
            assert info["rows_class"] == [0, 0, reps] and info["units"] == units
            _check(ctx, A, B, mode, "plus", 1.0, 1.0, av, bv)


# ---------------------------------------------------------------- 3. empty operands
def _small_pair():
    rng = np.random.default_rng(5)
    n, m = 3000, 40
    lens = [0, 3, 20, 40, 300, 700, 0, 5] * 5
    rows = lambda s: [np.sort(np.random.default_rng(s + i).choice(n, size=l, replace=False))
                      for i, l in enumerate(rng.permutation(lens))]
    return _csr(m, n, rows(10)), _csr(m, n, rows(500))


@pytest.mark.parametrize("valued", [False, True], ids=["structural", "valued"])
def test_ewise_empty_operands(ctx, valued):
    import torch
    from spgemm_amd.device import DeviceCSR
    A, B = _small_pair()
    m, n = A[:2]
    E = _csr(m, n, [np.zeros(0)] * m)
    val = lambda M, s: _values(M, s) if valued else None
    for X, Y in ((A, E), (E, B), (E, E)):
        # an operand without entries: columnindex NULL (an empty tensor's pointer)
        dX, dY = _dev(X, val(X, 7)), _dev(Y, val(Y, 8))
        for d in (dX, dY):
            assert d.nnz > 0 or d.struct().columnindex is None
        if valued and X is E:  # (a valued call needs a value pointer for A even where it has no entry)
            dX = DeviceCSR(m, n, dX.rowptr, dX.col, torch.zeros(1, dtype=torch.float64, device="cuda"))
        for mode in MODES:
            wrp, wci, wvv, both = _expect(X, Y, mode, "plus", 1.0, 1.0, val(X, 7), val(Y, 8))
            rp, ci, vv, info, _ = _run(ctx, X, Y, mode, av=val(X, 7), bv=val(Y, 8), dA=dX, dB=dY)
            np.testing.assert_array_equal(rp, wrp)
            np.testing.assert_array_equal(ci, wci)
            assert both == info["both"] == 0
            if valued:
                assert vv.tobytes() == wvv.tobytes()
    # rows empty in one operand only (A and B have them at different rows)
    la, lb = np.diff(A[2]), np.diff(B[2])
    assert ((la == 0) & (lb > 0)).any() and ((la > 0) & (lb == 0)).any()
    for mode in MODES:
        _check(ctx, A, B, mode, "max", 1.0, 1.0, val(A, 7), val(B, 8))
    # an empty result: columnindex and value NULL, the row pointers all zero
    disjoint = _csr(m, n, [np.setdiff1d(np.arange(50), r)[:7] for r in np.split(A[3], A[2][1:-1])])
    for X, Y, mode in ((A, disjoint, "intersect"), (A, A, "difference")):
        c, info, st = ctx.ewise(_dev(X, val(X, 7)), _dev(Y, val(Y, 8)), mode)
        assert (c.m, c.n, c.nnz, c.columnindex, c.value) == (m, n, 0, None, None) and c.rowpointer
        assert not ctx.to_host(c)[2].any() and info["nnzC"] == st["nnzC"] == 0
        assert info["both"] == (0 if mode == "intersect" else len(A[3]))
        ctx.reset()


# ---------------------------------------------------------------- 4. ops and scalars, bit for bit
@functools.lru_cache(maxsize=None)
def _mixed_case():
    """rows of all three classes, about half of each row's columns shared"""
    rng = np.random.default_rng(31)
    n = 30000
    lens = np.concatenate([rng.integers(0, 17, 300), rng.integers(20, 250, 60), rng.integers(600, 5000, 8)])
    lens = rng.permutation(lens)
    arows, brows = [], []
    for l in lens:
        cols = rng.choice(n, size=int(l) + int(l) // 2, replace=False)
        arows.append(np.sort(cols[:int(l)]))
        brows.append(np.sort(cols[int(l) // 2:]))
    A, B = _csr(len(lens), n, arows), _csr(len(lens), n, brows)
    return A, B, _values(A, 9), _values(B, 10)


def _fused_differs(alpha, beta, a, b):
    """whether a fused multiply-add on either product would change alpha * a + beta * b"""
    F = fractions.Fraction
    xa, yb = np.float64(alpha) * a, np.float64(beta) * b
    sep = xa + yb
    fa = float(F(float(alpha)) * F(float(a)) + F(float(yb)))
    fb = float(F(float(xa)) + F(float(beta)) * F(float(b)))
    return fa != sep or fb != sep


@pytest.mark.parametrize("op", list(OPS))
def test_ewise_ops_and_scalars_bit_for_bit(ctx, op):
    A, B, av, bv = _mixed_case()
    n = A[1]
    for alpha, beta in SCALARS:
        if op == "plus" and (alpha, beta) != (1.0, 1.0):
            # the case holds an entry that tells the separately rounded sum from a contracted one
            ka, kb = _keys(A[2], A[3], n), _keys(B[2], B[3], n)
            k = np.intersect1d(ka, kb)[:400]
            pa, pb = av[np.searchsorted(ka, k)], bv[np.searchsorted(kb, k)]
            assert any(_fused_differs(alpha, beta, x, y) for x, y in zip(pa, pb))
        for mode in ("union", "intersect"):
            info = _check(ctx, A, B, mode, op, alpha, beta, av, bv)
            assert all(c > 0 for c in info["rows_class"])
    if op == "plus":
        for alpha, beta in SCALARS:  # difference: alpha * a, whatever op and beta are
            _check(ctx, A, B, "difference", op, alpha, beta, av, bv)


def test_ewise_null_value_rules(ctx):
    A, B, av, bv = _mixed_case()
    # B's values are never read by a difference, nor by first under an intersection: B.value may be NULL
    for mode, op in (("difference", "plus"), ("difference", "second"), ("intersect", "first")):
        _check(ctx, A, B, mode, op, 2.5, -1.0, av, None)
    # every other valued call needs them
    live = ctx.pool_stats()["live_blocks"]
    for mode, op in (("union", "plus"), ("union", "first"), ("intersect", "plus"), ("intersect", "second")):
        with pytest.raises(_lib.TsgError) as e:
            ctx.ewise(_dev(A, av), _dev(B), mode, op)
        assert e.value.rc == ERR_INVALID and ctx.pool_stats()["live_blocks"] == live
    # A.value NULL: the structural call, whatever B carries -- no value comes back
    rp, ci, vv, info, _ = _run(ctx, A, B, "union", dA=_dev(A), dB=_dev(B, np.full(len(B[3]), np.nan)))
    wrp, wci, _, _ = _expect(A, B, "union")
    np.testing.assert_array_equal(rp, wrp)
    np.testing.assert_array_equal(ci, wci)
    assert vv is None


# ---------------------------------------------------------------- 5. validation
def _valid_pair():
    A = _csr(3, 6, [np.array([0, 2, 5]), np.array([1, 4]), np.array([3])])
    B = _csr(3, 6, [np.array([2, 3]), np.zeros(0), np.array([0, 3, 5])])
    return A, B


def _raw(ctx, dA, dB, mode, op):
    a, b, c = dA.struct(), dB.struct(), _lib.DevCSR(7, 7, 7, 1, 1, 1)
    info = _lib.EwiseInfo()
    rc = _lib.lib().tsg_dev_ewise(ctx.ptr, C.byref(a), C.byref(b), mode, op, 1.0, 1.0, None, C.byref(c),
                                  C.byref(info), None)
    return rc, c


@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("kind", ["row_unsorted", "col_repeated", "col_n", "col_neg", "rp_broken", "shape_m",
                                  "shape_n", "mode_3", "op_6", "op_neg"])
def test_ewise_validation(ctx, kind, side):
    A, B = _valid_pair()
    m, n, rp, ci = A if side == "A" else B
    rp, ci = rp.copy(), ci.copy()
    mode, op = 0, 0
    if kind == "row_unsorted":
        ci[0], ci[1] = ci[1], ci[0]
    elif kind == "col_repeated":
        ci[1] = ci[0]
    elif kind == "col_n":
        ci[-1] = n
    elif kind == "col_neg":
        ci[0] = -1
    elif kind == "rp_broken":
        rp[-1] += 1  # (rowpointer[m] != nnz)
    elif kind == "shape_m":
        m, rp = m + 1, np.concatenate([rp, rp[-1:]])
    elif kind == "shape_n":
        n = n + 1
    elif kind == "mode_3":
        mode = 3
    else:
        op = 6 if kind == "op_6" else -1
    bad = (m, n, rp, ci)
    for valued in (False, True):
        val = (lambda M: np.ones(len(M[3]))) if valued else (lambda M: None)
        dA, dB = (_dev(bad, val(bad)), _dev(B, val(B))) if side == "A" else (_dev(A, val(A)), _dev(bad, val(bad)))
        live = ctx.pool_stats()["live_blocks"]
        rc, c = _raw(ctx, dA, dB, mode, op)
        assert rc == ERR_INVALID, (kind, side, valued)
        assert (c.m, c.n, c.nnz, c.rowpointer, c.columnindex, c.value) == (0, 0, 0, None, None, None)
        assert ctx.pool_stats()["live_blocks"] == live
    # the context stays usable: a valid call succeeds
    for md in MODES:
        _check(ctx, A, B, md, "plus", 1.0, 1.0, np.ones(len(A[3])), np.ones(len(B[3])))


# ---------------------------------------------------------------- 6. error contract
def test_ewise_allocation_failures(ctx):
    A, B, lens = _edge_case()
    av, bv = _values(A, 1), _values(B, 2)
    dA, dB = _dev(A, av), _dev(B, bv)
    before = ctx.pool_stats()
    c, info, _ = ctx.ewise(dA, dB, "union", "plus")
    assert all(k > 0 for k in info["rows_class"])
    clean = ctx.to_host(c)
    nalloc = ctx.pool_stats()["allocs"] - before["allocs"]
    ctx.reset()
    assert 8 <= nalloc < 80
    live = ctx.pool_stats()["live_blocks"]
    assert live == before["live_blocks"]
    for nth in range(nalloc):
        assert ctx.fail_alloc(nth) is False
        with pytest.raises(_lib.TsgError) as e:
            ctx.ewise(dA, dB, "union", "plus")
        assert e.value.rc == ERR_OOM, nth
        assert ctx.pool_stats()["live_blocks"] == live, nth
        assert ctx.fail_alloc(-1) is False, nth  # (it fired: nothing left pending)
        c, _, _ = ctx.ewise(dA, dB, "union", "plus")  # the next call equals the clean result
        again = ctx.to_host(c)
        ctx.reset()
        for x, y in zip(clean[2:], again[2:]):
            assert x.tobytes() == y.tobytes(), nth
    assert ctx.fail_alloc(nalloc) is False
    ctx.ewise(dA, dB, "union", "plus")  # (one allocation short of the injection: it stays pending)
    ctx.reset()
    assert ctx.fail_alloc(-1) is True


# ---------------------------------------------------------------- 7. reproducibility
def test_ewise_is_reproducible(ctx):
    A, B, av, bv = _mixed_case()
    runs = [_run(ctx, A, B, "union", "plus", 1.0 / 3.0, 1e-3, av, bv) for _ in range(2)]
    for x, y in zip(runs[0][:3], runs[1][:3]):
        assert x.tobytes() == y.tobytes()
    wrp, wci, wvv, both = _expect(A, B, "union", "plus", 1.0 / 3.0, 1e-3, av, bv)
    rp, ci, vv, info, st = runs[0]
    assert st["path"] == 7 and st["nnzC"] == len(wci) == info["nnzC"] and info["both"] == both > 0
    assert info["nnzA"] == len(A[3]) and info["nnzB"] == len(B[3]) and st["t_e2e_ms"] > 0
    assert st["numtileA"] == st["numtileB"] == st["numblkC"] == -1
    assert vv.tobytes() == wvv.tobytes()


# ---------------------------------------------------------------- 8. few long rows
def test_ewise_few_long_rows(ctx):
    """a BFS Visited matrix's shape: 8 rows of 100,000 entries each, every row
    cut into 98 units"""
    n, m = 200000, 8
    rng = np.random.default_rng(41)
    rows = lambda: [np.sort(rng.choice(n, size=n // 2, replace=False)) for _ in range(m)]
    A, B = _csr(m, n, rows()), _csr(m, n, rows())
    for mode in ("union", "difference"):
        info = _check(ctx, A, B, mode)
        assert info["rows_class"] == [0, 0, m] and info["units"] == m * -(-n // TILE)
    _check(ctx, A, B, "union", "min", 1.0, 1.0, _values(A, 43), _values(B, 44))


# ---------------------------------------------------------------- 9. BFS on the device
def test_ewise_bfs_keeps_visited_on_the_device(ctx):
    """tests/test_gpu_symbolic_masked.py's multi-source BFS with Visited u= N done
    by Context.ewise: only the level sets come to the host"""
    n, _, rp, ci, _ = synth.rmat(scale_n=2000, seed=7)
    deg = np.diff(rp)
    src = np.flatnonzero(deg > 0)[:: max(1, int((deg > 0).sum()) // 8)][:8]
    assert len(src) == 8
    want = np.full((8, n), -1)
    for s, v0 in enumerate(src):
        want[s, v0] = 0
        frontier = [int(v0)]
        while frontier:
            nxt = []
            for u in frontier:
                for v in ci[rp[u]:rp[u + 1]]:
                    if want[s, v] < 0:
                        want[s, v] = want[s, u] + 1
                        nxt.append(int(v))
            frontier = nxt
    level = np.full((8, n), -1)
    level[np.arange(8), src] = 0
    dA = _dev((n, n, rp, ci))
    F = visited = _dev(_from_keys(8, n, np.arange(8) * n + src))
    depth = 0
    while F.nnz:
        depth += 1
        assert depth <= n
        c, _, _ = ctx.spgemm_symbolic(F, dA, "pattern", mask=visited, complement=True)
        F = ctx.to_torch(c)
        if F.nnz:
            v, info, _ = ctx.ewise(visited, F)
            assert v.value is None and info["both"] == 0 and info["nnzC"] == visited.nnz + F.nnz
            visited = ctx.to_torch(v)
        ctx.reset()
        _, _, nrp, nci, _ = F.to_host()
        k = _keys(nrp, nci, n)
        assert (level[k // n, k % n] == -1).all()  # (nothing visited comes back)
        level[k // n, k % n] = depth
    np.testing.assert_array_equal(level, want)
    assert depth - 1 == want.max() >= 2
    _, _, vrp, vci, vvv = visited.to_host()
    assert vvv is None
    np.testing.assert_array_equal(_keys(vrp, vci, n), np.flatnonzero(want.ravel() >= 0))


# ---------------------------------------------------------------- 10. Bellman-Ford
def test_ewise_bellman_ford(ctx):
    """D = min(D, D min.+ A) until D stops changing, 4 sources, integer weights
    (every path sum exact), against a numpy Bellman-Ford"""
    n, _, rp, ci, _ = synth.rmat(scale_n=2000, seed=7)
    rng = np.random.default_rng(51)
    w = rng.integers(1, 10, size=len(ci)).astype(np.float64)
    deg = np.diff(rp)
    src = np.flatnonzero(deg > 0)[:: max(1, int((deg > 0).sum()) // 4)][:4]
    rows = np.repeat(np.arange(n), deg)
    want = np.full((4, n), np.inf)
    want[np.arange(4), src] = 0.0
    for _ in range(n):
        nxt = want.copy()
        for s in range(4):
            np.minimum.at(nxt[s], ci, want[s, rows] + w)
        if np.array_equal(nxt, want):
            break
        want = nxt
    dA = _dev((n, n, rp, ci), w)
    D = _dev(_from_keys(4, n, np.arange(4) * n + src), np.zeros(4))
    for it in range(n):
        Dn = ctx.spgemm_accum(D, D, dA, semiring="min_plus")
        ctx.reset()
        same = (Dn.nnz == D.nnz and bool((Dn.rowptr == D.rowptr).all()) and bool((Dn.col == D.col).all())
                and bool((Dn.val == D.val).all()))
        D = Dn
        if same:
            break
    assert 2 <= it < n
    _, _, drp, dci, dvv = D.to_host()
    k = _keys(drp, dci, n)
    np.testing.assert_array_equal(k, np.flatnonzero(np.isfinite(want).ravel()))  # the unreachable are absent
    np.testing.assert_array_equal(dvv, want.ravel()[k])
    assert len(k) < 4 * n


# ---------------------------------------------------------------- 11. spgemm_accum
@pytest.mark.parametrize("masked", [None, False, True], ids=["unmasked", "mask", "complement"])
def test_ewise_spgemm_accum(ctx, masked):
    Am = synth.random_csr(300, 400, nnz_per_row=6, seed=61)
    Bm = synth.random_csr(400, 500, nnz_per_row=7, seed=62)
    rng = np.random.default_rng(63)
    # small integers: the product's sums are exact, so two runs of it agree bit for bit whatever their order
    av = rng.integers(-9, 10, len(Am[3])).astype(np.float64)
    bv = rng.integers(-9, 10, len(Bm[3])).astype(np.float64)
    dA, dB = _dev(Am[:4], av), _dev(Bm[:4], bv)
    C0 = _from_keys(300, 500, rng.integers(0, 300 * 500, size=9000))
    c0v = rng.standard_normal(len(C0[3]))
    dC0 = _dev(C0, c0v)
    mask = _dev(_from_keys(300, 500, rng.integers(0, 300 * 500, size=60000)))
    if masked is None:
        P, _, _ = ctx.spgemm_semiring(dA, dB, "plus_times")
        got = ctx.spgemm_accum(dC0, dA, dB)
    else:
        P, _, _ = ctx.spgemm_masked_sparse(dA, dB, mask, complement=masked)
        got = ctx.spgemm_accum(dC0, dA, dB, mask=mask, complement=masked)
    ctx.reset()
    _, _, prp, pci, pvv = P.to_host()
    assert 0 < len(pci)
    wrp, wci, wvv, both = _expect(C0, (300, 500, prp, pci), "union", "plus", 1.0, 1.0, c0v, pvv)
    assert 0 < both < len(pci)
    _, _, rp, ci, vv = got.to_host()
    np.testing.assert_array_equal(rp, wrp)
    np.testing.assert_array_equal(ci, wci)
    assert vv.tobytes() == wvv.tobytes()
    # and it is the ewise union of C0 with the product obtained separately
    c, _, _ = ctx.ewise(dC0, P, "union", "plus")
    _, _, erp, eci, evv = ctx.to_host(c)
    ctx.reset()
    assert (erp.tobytes(), eci.tobytes(), evv.tobytes()) == (rp.tobytes(), ci.tobytes(), vv.tobytes())


# ---------------------------------------------------------------- 12. host layer
def test_ewise_host_layer():
    import scipy.sparse as sp
    import _oracle as O
    oA = O.OMat.load(os.path.join(FIXTURES, "x_powerlaw_400.mtx"))
    m, n, rp, ci, vv = oA.csr()
    assert m == n
    S = sp.csr_matrix((np.asarray(vv, dtype=np.float64), np.asarray(ci), np.asarray(rp)), shape=(m, n))
    S.sum_duplicates()
    S.sort_indices()
    St = S.T.tocsr()
    St.sort_indices()
    A4 = (m, n, S.indptr.astype(np.int32), S.indices.astype(np.int32))
    B4 = (m, n, St.indptr.astype(np.int32), St.indices.astype(np.int32))
    av, bv = S.data.astype(np.float64), St.data.astype(np.float64)
    A, B = T.Matrix.from_csr(*A4, av), T.Matrix.from_csr(*B4, bv)
    for mode in MODES:
        wrp, wci, wvv, _ = _expect(A4, B4, mode, "plus", 2.0, 0.5, av, bv)
        Cm, st = T.ewise(A, B, mode, "plus", 2.0, 0.5)
        cm, cn, crp, cci, cvv = Cm.csr()
        assert (cm, cn) == (m, n) and st["path"] == T.PATH_EWISE and st["nnzC"] == len(wci)
        np.testing.assert_array_equal(crp, wrp)
        np.testing.assert_array_equal(cci, wci)
        assert cvv.tobytes() == wvv.tobytes()
        # structural: a Matrix without values
        Cs, _ = T.ewise(T.Matrix.from_csr(*A4, None), T.Matrix.from_csr(*B4, None), mode)
        _, _, srp, sci, svv = Cs.csr()
        np.testing.assert_array_equal(srp, wrp)
        np.testing.assert_array_equal(sci, wci)
        assert len(svv) == 0 and not Cs.s.value
    # an operand as read from a file with unsorted rows and repeated entries is refused
    U = T.mmio_allinone(os.path.join(FIXTURES, "x_int_unsorted_dup_77.mtx"))
    with pytest.raises(_lib.TsgError) as e:
        T.ewise(U, T.Matrix.alias(U))
    assert e.value.rc == ERR_INVALID
    for bad in (dict(mode=3), dict(op=6), dict(mode="nonsense"), dict(op="nonsense")):
        with pytest.raises(_lib.TsgError) as e:
            T.ewise(A, B, **bad)
        assert e.value.rc == ERR_INVALID
