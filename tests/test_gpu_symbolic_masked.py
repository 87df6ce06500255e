"""Masked symbolic SpGEMM (tsg_dev_spgemm_symbolic_masked /
Context.spgemm_symbolic(mask=...), tsg_spgemm_csr_symbolic_masked) and the
masked product with GraphBLAS semantics built on it (spgemm_masked_sparse).
The unmasked pattern comes from the oracle's Gustavson on unit values (scipy on
unit values for the larger cases, as tests/test_gpu_symbolic.py builds it); the
expected pattern is its per-row intersection with the mask (plain sense) or
difference from it (complement), taken in numpy on row * n + column keys.  Every
comparison of row pointers and columns is exact."""
import ctypes as C
import functools
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

PACKED_CAP, SET_WAVE_CAP, SET_CAP, WINDOW_CAP = 32, 512, 4096, 65536
W = 131072
ERR_INVALID, ERR_OOM, ERR_OVERFLOW = -1, -3, -4
SENSES = (False, True)


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


def _keys(rp, ci, n):
    """row * n + column of every entry (ascending for a pattern with sorted rows)"""
    rows = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp.astype(np.int64)))
    return rows * n + ci.astype(np.int64)


def _from_keys(m, n, keys):
    keys = np.unique(np.asarray(keys, dtype=np.int64))
    rp = np.concatenate([[0], np.cumsum(np.bincount(keys // n, minlength=m))]).astype(np.int32)
    return m, n, rp, (keys % n).astype(np.int32)


def _restrict(ref, mask, comp):
    """the reference pattern's rows intersected with the mask's (comp: minus the mask's)"""
    m, n = mask[:2]
    k = _keys(ref[0], ref[1], n)
    k = k[np.isin(k, _keys(mask[2], mask[3], n)) != comp]
    return _from_keys(m, n, k)[2:]


def _mask_of_rows(m, n, rows):
    return _csr(m, n, [np.unique(np.asarray(r, dtype=np.int64)) for r in rows])


def _random_mask(ref, m, n, seed, extra):
    """about half of the reference's entries and `extra` positions drawn over the whole matrix"""
    rng = np.random.default_rng(seed)
    k = _keys(ref[0], ref[1], n)
    return _from_keys(m, n, np.concatenate([k[rng.random(len(k)) < 0.5], rng.integers(0, m * n, size=extra)]))


def _sym(ctx, A, B, mask, comp, mode="pattern", dmask=None):
    """(rowptr, col, info, stats) of a masked symbolic call, copied to the host"""
    c, info, st = ctx.spgemm_symbolic(_dev(A), _dev(B), mode, mask=dmask if dmask is not None else _dev(mask),
                                      complement=comp)
    assert c.value is None and c.m == A[0] and c.n == B[1]
    _, _, rp, ci, vv = ctx.to_host(c)
    assert vv is None or c.nnz == 0
    assert rp[0] == 0 and rp[-1] == c.nnz == info["nnzC"] == st["nnzC"]
    assert st["path"] == T.PATH_SYMBOLIC == 6 and st["nnzCub"] == info["products"]
    assert bool(c.columnindex) == (mode == "pattern" and c.nnz > 0)
    ctx.reset()
    return rp, ci, info, st


def _check(ctx, A, B, mask, ref, senses=SENSES, mode="pattern"):
    out = []
    for comp in senses:
        wrp, wci = _restrict(ref, mask, comp)
        rp, ci, info, _ = _sym(ctx, A, B, mask, comp, mode)
        np.testing.assert_array_equal(rp, wrp, err_msg=f"complement={comp}")
        if mode == "pattern":
            np.testing.assert_array_equal(ci, wci, err_msg=f"complement={comp}")
        else:
            assert len(ci) == 0
        out.append(info)
    return out


def _unmasked(ctx, A, B, mode="pattern"):
    c, info, _ = ctx.spgemm_symbolic(_dev(A), _dev(B), mode)
    _, _, rp, ci, _ = ctx.to_host(c)
    ctx.reset()
    return rp, ci, info


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
def test_masked_symbolic_fixtures(ctx, path, aat):
    """the mask: A's own pattern, its rows sorted and de-duplicated (of a
    rectangular A against A^T, whose product is m x m: the columns below m)"""
    oA = O.OMat.load(path)
    m, n, rp, ci, _ = oA.csr()
    A = (m, n, rp, ci)
    B = O.transpose(oA).csr()[:4] if aat else A
    k = _keys(rp, ci, n)
    k = k[(k % n) < B[1]]
    mask = _from_keys(m, B[1], (k // n) * B[1] + k % n)
    _check(ctx, A, B, mask, _ref_oracle(A, B))


# ---------------------------------------------------------------- 2. class cap edges
MASK_KINDS = ["empty", "all", "every_other", "first_last", "unreached"]


@functools.lru_cache(maxsize=None)
def _cap_case(cap):
    n = cap + 900
    rng = np.random.default_rng(cap)
    A = _csr(2, n, [rng.choice(n, size=cap, replace=False), rng.choice(n, size=cap + 1, replace=False)])
    B = _csr(n, n, [np.array([i]) for i in range(n)])
    return A, B, _ref_scipy(A, B)


@pytest.mark.parametrize("kind", MASK_KINDS)
@pytest.mark.parametrize("cap", [PACKED_CAP, SET_WAVE_CAP, SET_CAP, WINDOW_CAP])
def test_masked_symbolic_cap_edges(ctx, cap, kind):
    """rows of exactly cap and cap + 1 products on distinct columns (an identity
    B): the fullest a class's set can get, under each shape of mask row"""
    A, B, ref = _cap_case(cap)
    n = B[1]
    rows = []
    for i in range(2):
        c = ref[1][ref[0][i]:ref[0][i + 1]]
        assert len(c) == cap + i
        rows.append({"empty": c[:0], "all": c, "every_other": c[::2], "first_last": c[[0, -1]],
                     "unreached": np.setdiff1d(np.arange(n), c)}[kind])
    infos = _check(ctx, A, B, _mask_of_rows(2, n, rows), ref)
    want = {"empty": (0, 2 * cap + 1), "all": (2 * cap + 1, 0), "every_other": (cap + 1, cap),
            "first_last": (4, 2 * cap - 3), "unreached": (0, 2 * cap + 1)}[kind]
    assert tuple(i["nnzC"] for i in infos) == want
    for i in infos:  # (the classes and the products: the unmasked product's)
        assert i["products"] == 2 * cap + 1 and sum(i["rows_class"]) == 2


# ---------------------------------------------------------------- 3. bitmap ownership edges
EDGE_N = 2 * W + 37
EDGE_ROWS = [
    np.array([0, 31, 32, 63, 64, 511, 512, W - 1, W, W + 511, W + 512, 2 * W - 1, 2 * W, EDGE_N - 1]),
    # first column W + 40: a sorted B's window starts at its word, W + 32 (its threads' shares: 512 columns from there)
    np.array([W + 40, W + 41, W + 63, W + 64, W + 32 + 511, W + 32 + 512, 2 * W + 5, EDGE_N - 1]),
    np.array([5, 100, 511, 700, W - 1]),        # last column W - 1: one window
    np.concatenate([np.arange(0, EDGE_N, 997), [2 * W + 3, EDGE_N - 1]]),  # three windows
    np.array([2 * W, 2 * W + 5, EDGE_N - 1]),
]


@functools.lru_cache(maxsize=None)
def _edge_case(target, b_sorted):
    """every row's B row repeated until the row holds target products or a few more"""
    B = _csr(len(EDGE_ROWS), EDGE_N, EDGE_ROWS)
    if not b_sorted:
        rng = np.random.default_rng(3)
        B = _csr(len(EDGE_ROWS), EDGE_N, [rng.permutation(r) for r in EDGE_ROWS])
    A = _csr(len(EDGE_ROWS), len(EDGE_ROWS), [np.full(-(-target // len(r)), k) for k, r in enumerate(EDGE_ROWS)])
    return A, B, _ref_scipy(A, B)


def _edge_mask_row(kind, c):
    n, inside = EDGE_N, (c >= W) & (c < 2 * W)
    if kind == "alternate":  # every other product column, and the columns next to the others
        return np.concatenate([c[::2], np.setdiff1d(np.clip(np.concatenate([c[1::2] - 1, c[1::2] + 1]), 0, n - 1), c)])
    if kind == "first_last":
        return c[[0, -1]]
    if kind == "below":  # all below the row's first column: below its first word, and within it
        return np.arange(max(int(c[0]) - 70, 0), int(c[0]))
    if kind == "above":
        return np.arange(int(c[-1]) + 1, min(int(c[-1]) + 70, n))
    if kind == "middle_window_out":  # the plain sense leaves the middle window of a three-window row nothing
        return np.concatenate([c[~inside], np.array([W + 1, 2 * W - 2])])
    assert kind == "middle_window_in"  # ... and the complement
    return np.concatenate([c[inside], np.array([W + 1, 2 * W - 2])])


@pytest.mark.parametrize("kind", ["alternate", "first_last", "below", "above", "middle_window_out",
                                  "middle_window_in"])
@pytest.mark.parametrize("b_sorted", [True, False], ids=["sortedB", "unsortedB"])
@pytest.mark.parametrize("target", [5000, 70000], ids=["window", "hub"])
def test_masked_symbolic_bitmap_edges(ctx, target, b_sorted, kind):
    """mask and product columns on either side of a word (31 / 32), of a thread's
    16 words (511 / 512) and of a window or hub segment (131,071 / 131,072), at
    the row's first and last column, wholly below and wholly above the row"""
    A, B, ref = _edge_case(target, b_sorted)
    m = A[0]
    for i, r in enumerate(EDGE_ROWS):
        np.testing.assert_array_equal(ref[1][ref[0][i]:ref[0][i + 1]], r)
    mask = _mask_of_rows(m, EDGE_N, [_edge_mask_row(kind, r) for r in EDGE_ROWS])
    infos = _check(ctx, A, B, mask, ref)
    want = [0, 0, 0, 0]
    want[2 if target == 5000 else 3] = m
    assert all(i["rows_class"] == want for i in infos)
    total = len(ref[1])
    if kind in ("below", "above"):
        assert [i["nnzC"] for i in infos] == [0, total]
    if kind.startswith("middle"):  # the three-window row's middle window holds nothing, its neighbours do
        comp = kind.endswith("in")
        rp, ci, _, _ = _sym(ctx, A, B, mask, comp)
        row = ci[rp[3]:rp[4]]
        assert not ((row >= W) & (row < 2 * W)).any() and (row < W).any() and (row >= 2 * W).any()


# ---------------------------------------------------------------- 4. identities
@pytest.fixture(scope="module")
def mixed():
    A, B = numeric_mixed_case()
    return A, B, _ref_oracle(A, B)


@pytest.fixture(scope="module")
def hub():
    A, B, _ = hub_rows_case()
    A, B = A[:4], B[:4]
    return A, B, _ref_scipy(A, B)


@pytest.mark.parametrize("case", ["mixed", "hub"])
def test_masked_symbolic_identities(ctx, case, request):
    A, B, ref = request.getfixturevalue(case)
    m, n = A[0], B[1]
    urp, uci, uinfo = _unmasked(ctx, A, B)
    np.testing.assert_array_equal(urp, ref[0])
    np.testing.assert_array_equal(uci, ref[1])
    # the complement of an empty mask (columnindex NULL), and the plain sense of the full pattern: A*B itself
    none = _csr(m, n, [np.zeros(0)] * m)
    full = (m, n, ref[0], ref[1])
    for mask, comp in ((none, True), (full, False)):
        rp, ci, info, _ = _sym(ctx, A, B, mask, comp)
        np.testing.assert_array_equal(rp, urp)
        np.testing.assert_array_equal(ci, uci)
        assert info == uinfo
    for mask, comp in ((none, False), (full, True)):
        rp, ci, info, _ = _sym(ctx, A, B, mask, comp)
        assert not rp.any() and len(ci) == 0 and info["nnzC"] == 0
        assert info["products"] == uinfo["products"] and info["rows_class"] == uinfo["rows_class"]
    # plain(M) and complement(M) part the pattern
    mask = _random_mask(ref, m, n, 21, 20000)
    prp, pci, pinfo, _ = _sym(ctx, A, B, mask, False)
    crp, cci, cinfo, _ = _sym(ctx, A, B, mask, True)
    kp, kc = _keys(prp, pci, n), _keys(crp, cci, n)
    assert len(np.intersect1d(kp, kc)) == 0
    np.testing.assert_array_equal(np.union1d(kp, kc), _keys(ref[0], ref[1], n))
    assert pinfo["nnzC"] + cinfo["nnzC"] == uinfo["nnzC"] and 0 < pinfo["nnzC"] < uinfo["nnzC"]
    np.testing.assert_array_equal(prp, _restrict(ref, mask, False)[0])
    np.testing.assert_array_equal(pci, _restrict(ref, mask, False)[1])


# ---------------------------------------------------------------- 5. hub rows in batches
@pytest.mark.parametrize("budget", [400000, 1], ids=["two-rows-a-batch", "one-row-a-batch"])
def test_masked_symbolic_hub_rows_in_batches(ctx, hub, monkeypatch, budget):
    """4 hub rows of 187,504-byte bitmaps in 2 and in 4 batches: the fill marks a
    batch's bitmaps again and must mask them again"""
    A, B, ref = hub
    monkeypatch.setenv("TSG_SYM_HUB_BYTES", str(budget))
    monkeypatch.setenv("TSG_QUIET", "1")
    mask = _random_mask(ref, A[0], B[1], 22, 50000)
    infos = _check(ctx, A, B, mask, ref)
    assert all(i["rows_class"][3] == 4 for i in infos)
    _check(ctx, A, B, mask, ref, mode="count")


# ---------------------------------------------------------------- 6. unsorted, repeating operands
def test_masked_symbolic_unsorted_repeating_operands(ctx):
    Am = synth.random_csr(300, 2000, nnz_per_row=40, seed=5, unsorted=True, dups=True)
    Bm = synth.random_csr(2000, 300000, nnz_per_row=60, seed=6, unsorted=True, dups=True)
    A, B = Am[:4], Bm[:4]
    ref = _ref_scipy(A, B)
    infos = _check(ctx, A, B, _random_mask(ref, 300, 300000, 23, 100000), ref)
    assert infos[0]["b_rows_sorted"] == 0 and infos[0]["rows_class"][1] > 0 and infos[0]["rows_class"][2] > 0


# ---------------------------------------------------------------- 7. count mode
@pytest.mark.parametrize("comp", SENSES)
def test_masked_symbolic_count_mode(ctx, mixed, comp):
    A, B, ref = mixed
    mask = _random_mask(ref, A[0], B[1], 24, 20000)
    rp, ci, info, _ = _sym(ctx, A, B, mask, comp)
    c, info_c, _ = ctx.spgemm_symbolic(_dev(A), _dev(B), "count", mask=_dev(mask), complement=comp)
    assert c.columnindex is None and c.value is None
    rp_c = ctx.to_host(c)[2]
    ctx.reset()
    np.testing.assert_array_equal(rp_c, rp)
    assert info_c == info and info_c["nnzC"] == rp_c[-1] == c.nnz


# ---------------------------------------------------------------- 8. int32 overflow of the masked total
def test_masked_symbolic_overflow_is_decided_on_the_masked_total(ctx):
    """the 46,400 x 46,400 outer product less one full row: 46,400 * 46,399 =
    2,152,913,600 entries, past int32, counted exactly"""
    k = 46400
    A = _csr(k, 1, [np.array([0])] * k)
    B = _csr(1, k, [np.arange(k)])
    mask = _csr(k, k, [np.zeros(0)] * 17 + [np.arange(k)] + [np.zeros(0)] * (k - 18))
    live = ctx.pool_stats()["live_blocks"]
    with pytest.raises(_lib.TsgError) as e:
        ctx.spgemm_symbolic(_dev(A), _dev(B), "count", mask=_dev(mask), complement=True)
    assert e.value.rc == ERR_OVERFLOW
    assert e.value.info["nnzC"] == k * (k - 1) == 2_152_913_600 > 2 ** 31 - 1
    assert e.value.info["products"] == k * k
    assert ctx.pool_stats()["live_blocks"] == live
    # the plain sense of the same mask fits: the one row
    c, info, _ = ctx.spgemm_symbolic(_dev(A), _dev(B), "count", mask=_dev(mask), complement=False)
    assert info["nnzC"] == k == c.nnz and info["products"] == k * k
    rp = ctx.to_host(c)[2]
    assert rp[17] == 0 and rp[18] == k == rp[-1]
    ctx.reset()


# ---------------------------------------------------------------- 9. validation
def _valid_triple():
    A = _csr(3, 4, [np.array([0, 3]), np.array([1]), np.array([2, 0])])
    B = _csr(4, 6, [np.array([5, 0]), np.array([1]), np.zeros(0), np.array([2, 3])])
    M = _csr(3, 6, [np.array([0, 2, 5]), np.array([1, 4]), np.array([3])])
    return A, B, M


def _raw(ctx, dA, dB, dM, comp, mode):
    a, b, mk, c = dA.struct(), dB.struct(), dM.struct(), _lib.DevCSR(7, 7, 7, 1, 1, 1)
    info = _lib.SymbolicInfo()
    rc = _lib.lib().tsg_dev_spgemm_symbolic_masked(ctx.ptr, C.byref(a), C.byref(b), C.byref(mk), comp, mode, None,
                                                   C.byref(c), C.byref(info), None)
    return rc, c


@pytest.mark.parametrize("kind", ["row_unsorted", "col_repeated", "col_n", "col_neg", "rp_broken", "mask_m",
                                  "mask_n", "complement_2", "mode_unknown"])
def test_masked_symbolic_validation(ctx, kind):
    from spgemm_amd.device import DeviceCSR
    A, B, M = _valid_triple()
    m, n, rp, ci = M
    rp, ci = rp.copy(), ci.copy()
    comp, mode = 1, 0
    if kind == "row_unsorted":
        ci[0], ci[1] = ci[1], ci[0]
    elif kind == "col_repeated":
        ci[1] = ci[0]
    elif kind == "col_n":
        ci[2] = n
    elif kind == "col_neg":
        ci[0] = -1
    elif kind == "rp_broken":
        rp[1], rp[2] = rp[2], rp[1]
    elif kind == "mask_m":
        m, rp = m + 1, np.concatenate([rp, rp[-1:]])
    elif kind == "mask_n":
        n = n + 1
    elif kind == "complement_2":
        comp = 2
    else:
        mode = 7
    dA, dB, dM = _dev(A), _dev(B), _dev((m, n, rp, ci))
    assert isinstance(dM, DeviceCSR) and dM.nnz == len(ci)
    live = ctx.pool_stats()["live_blocks"]
    for md in ((0, 1) if kind != "mode_unknown" else (mode,)):
        rc, c = _raw(ctx, dA, dB, dM, comp, md)
        assert rc == ERR_INVALID, (kind, md)
        assert (c.m, c.n, c.nnz, c.rowpointer, c.columnindex, c.value) == (0, 0, 0, None, None, None)
        assert ctx.pool_stats()["live_blocks"] == live
    if kind != "mode_unknown":
        with pytest.raises(_lib.TsgError) as e:
            ctx.spgemm_symbolic(dA, dB, "pattern", mask=dM, complement=comp)
        assert e.value.rc == ERR_INVALID and ctx.pool_stats()["live_blocks"] == live
    # the same call with a valid mask then succeeds
    _check(ctx, A, B, M, _ref_oracle(A, B))


# ---------------------------------------------------------------- 10. allocation failures
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


def test_masked_symbolic_allocation_failures(ctx):
    A, B = _all_class_case()
    ref = _ref_scipy(A, B)
    mask = _random_mask(ref, A[0], B[1], 25, 30000)
    infos = _check(ctx, A, B, mask, ref)
    assert all(c > 0 for c in infos[0]["rows_class"]), infos[0]
    dA, dB, dM = _dev(A), _dev(B), _dev(mask)
    live = ctx.pool_stats()["live_blocks"]
    nth, done = 0, False
    while not done:
        assert nth < 80
        assert ctx.fail_alloc(nth) is False
        try:
            c, _, _ = ctx.spgemm_symbolic(dA, dB, "pattern", mask=dM, complement=True)
            done = True
        except _lib.TsgError as e:
            assert e.rc == ERR_OOM, nth
            assert ctx.pool_stats()["live_blocks"] == live, nth
            assert ctx.fail_alloc(-1) is False, nth  # (it fired: nothing left pending)
            nth += 1
    assert nth >= 8
    assert ctx.fail_alloc(-1) is True  # (the call that succeeded made fewer allocations: still pending, now cleared)
    _, _, rp, ci, _ = ctx.to_host(c)
    ctx.reset()
    want = _restrict(ref, mask, True)
    np.testing.assert_array_equal(rp, want[0])
    np.testing.assert_array_equal(ci, want[1])


# ---------------------------------------------------------------- 11. the mask's values are not read
def test_masked_symbolic_reads_no_mask_values_and_leaves_inputs_untouched(ctx, mixed):
    import torch
    A, B, ref = mixed
    mask = _random_mask(ref, A[0], B[1], 26, 20000)
    dA, dB = _dev(A, np.full(len(A[3]), np.nan)), _dev(B, np.full(len(B[3]), np.nan))
    dM = _dev(mask, np.full(len(mask[3]), np.nan))
    tensors = (dA.rowptr, dA.col, dA.val, dB.rowptr, dB.col, dB.val, dM.rowptr, dM.col, dM.val)
    before = [t.clone() for t in tensors]
    for comp in SENSES:
        c, _, _ = ctx.spgemm_symbolic(dA, dB, "pattern", mask=dM, complement=comp)
        _, _, rp, ci, vv = ctx.to_host(c)
        ctx.reset()
        assert vv is None
        rp0, ci0, _, _ = _sym(ctx, A, B, mask, comp)  # (val=None everywhere)
        np.testing.assert_array_equal(rp, rp0)
        np.testing.assert_array_equal(ci, ci0)
        np.testing.assert_array_equal(ci, _restrict(ref, mask, comp)[1])
    for t, b in zip(tensors, before):  # (bit for bit: NaNs compared as their integer images)
        assert torch.equal(t.view(torch.int32) if t.dtype == torch.int32 else t.view(torch.int64),
                           b.view(torch.int32) if b.dtype == torch.int32 else b.view(torch.int64))


# ---------------------------------------------------------------- 12. values
class _Products:
    """every element product of A*B, by (row, column): the A entry e and the B
    entry q of each; first: the start of each distinct key's run"""

    def __init__(self, A, B):
        m, _, rpa, cia = A[:4]
        _, n, rpb, cib = B[:4]
        blen = np.diff(rpb.astype(np.int64))[cia]
        e = np.repeat(np.arange(len(cia)), blen)
        q = rpb.astype(np.int64)[cia][e] + np.arange(int(blen.sum())) - np.repeat(np.cumsum(blen) - blen, blen)
        key = np.repeat(np.arange(m, dtype=np.int64), np.diff(rpa))[e] * n + cib[q]
        order = np.argsort(key, kind="stable")
        self.e, self.q, key = e[order], q[order], key[order]
        self.first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
        self.keys = key[self.first]


@pytest.fixture(scope="module")
def mixed_products(mixed):
    A, B, ref = mixed
    p = _Products(A, B)
    np.testing.assert_array_equal(p.keys, _keys(ref[0], ref[1], B[1]))
    return p


@pytest.mark.parametrize("comp", SENSES, ids=["plain", "complement"])
def test_masked_sparse_values(ctx, mixed, mixed_products, comp):
    A, B, ref = mixed
    m, n = A[0], B[1]
    prod = mixed_products
    mask = _random_mask(ref, m, n, 27, 20000)
    wrp, wci = _restrict(ref, mask, comp)
    sel = np.isin(prod.keys, _keys(mask[2], mask[3], n)) != comp  # the reference keys the mask admits
    rng = np.random.default_rng(28)
    av, bv = rng.uniform(0.5, 2.0, len(A[3])), rng.uniform(0.5, 2.0, len(B[3]))
    av[::3] *= -1.0
    dA, dB, dM = _dev(A, av), _dev(B, bv), _dev(mask)
    x = av[prod.e] * bv[prod.q]
    exp = {"plus_times": np.add.reduceat(x, prod.first)[sel],
           "min_plus": np.minimum.reduceat(av[prod.e] + bv[prod.q], prod.first)[sel],
           "max_plus": np.maximum.reduceat(av[prod.e] + bv[prod.q], prod.first)[sel],
           "plus_pair": np.add.reduceat(np.ones(len(x)), prod.first)[sel]}
    mag = np.add.reduceat(np.abs(x), prod.first)[sel]
    for sr in ("plus_times", "min_plus", "max_plus", "plus_pair"):
        runs = []
        for _ in range(1 if sr == "plus_times" else 2):
            Cd, info, st = ctx.spgemm_masked_sparse(dA if sr != "plus_pair" else _dev(A),
                                                    dB if sr != "plus_pair" else _dev(B), dM, complement=comp,
                                                    semiring=sr)
            assert st["path"] == T.PATH_MASKED and info["nnzC"] == len(wci) == Cd.nnz
            np.testing.assert_array_equal(Cd.rowptr.cpu().numpy(), wrp)
            np.testing.assert_array_equal(Cd.col.cpu().numpy(), wci)
            runs.append(Cd.val.cpu().numpy())
        got = runs[0]
        assert not np.isnan(got).any()
        if sr == "plus_times":  # the row-wise leg's bound: 1e-10 relative to sum |a||b| at the entry
            err = np.abs(got - exp[sr])
            assert np.all(err <= 1e-10 * mag), float(np.max(err / mag))
        else:
            np.testing.assert_array_equal(got, exp[sr])
            assert runs[0].tobytes() == runs[1].tobytes()
        if sr in ("min_plus", "max_plus"):  # every entry is reached: none holds the identity
            assert np.isfinite(got).all()
        if sr == "plus_pair":
            assert got.min() >= 1.0
    ctx.reset()


# ---------------------------------------------------------------- 13. BFS
def test_masked_symbolic_multi_source_bfs(ctx):
    """levels of 8 sources on an R-MAT graph by N = F*A<!Visited> per step; the
    union Visited + N on the host; against a queue BFS on the CPU"""
    n, _, rp, ci, _ = synth.rmat(scale_n=2000, seed=7)
    A = (n, n, rp, ci)
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
    F = _from_keys(8, n, np.arange(8) * n + src)
    visited = F
    dA = _dev(A)
    depth = 0
    while len(F[3]):
        depth += 1
        assert depth <= n
        c, info, _ = ctx.spgemm_symbolic(_dev(F), dA, "pattern", mask=_dev(visited), complement=True)
        _, _, nrp, nci, _ = ctx.to_host(c)
        ctx.reset()
        k = _keys(nrp, nci, n)
        assert (level[k // n, k % n] == -1).all()  # (nothing visited comes back)
        level[k // n, k % n] = depth
        F = (8, n, nrp, nci)
        visited = _from_keys(8, n, np.concatenate([_keys(visited[2], visited[3], n), k]))
    np.testing.assert_array_equal(level, want)
    assert depth - 1 == want.max() >= 2


# ---------------------------------------------------------------- 14. host layer
@pytest.mark.parametrize("name", ["x_int_unsorted_dup_77", "x_rect_50x130"])
def test_masked_host_layer(name):
    oA = O.OMat.load(os.path.join(FIXTURES, name + ".mtx"))
    m, n, rp, ci, vv = oA.csr()
    bm, bn, brp, bci, bvv = O.transpose(oA).csr()
    A4, B4 = (m, n, rp, ci), (bm, bn, brp, bci)
    ref = _ref_oracle(A4, B4)
    mask = _random_mask(ref, m, bn, 29, 300)
    full = O.gustavson(O.OMat.from_csr(*A4, vv), O.OMat.from_csr(*B4, bvv)).csr()
    fmag = O.gustavson(O.OMat.from_csr(*A4, np.abs(vv)), O.OMat.from_csr(*B4, np.abs(bvv))).csr()
    np.testing.assert_array_equal(full[3], ref[1])
    A, B = T.Matrix.from_csr(m, n, rp, ci, vv), T.Matrix.from_csr(bm, bn, brp, bci, bvv)
    Mk = T.Matrix.from_csr(m, bn, mask[2], mask[3], np.full(len(mask[3]), np.nan))
    for comp in SENSES:
        wrp, wci = _restrict(ref, mask, comp)
        sel = np.isin(_keys(ref[0], ref[1], bn), _keys(mask[2], mask[3], bn)) != comp
        Cm, st = T.spgemm_symbolic_masked(A, B, Mk, complement=comp)
        cm, cn, crp, cci, cvv = Cm.csr()
        assert (cm, cn) == (m, bn) and len(cvv) == 0 and not Cm.s.value
        np.testing.assert_array_equal(crp, wrp)
        np.testing.assert_array_equal(cci, wci)
        assert st["path"] == 6 and st["nnzC"] == len(wci)
        Cc, st = T.spgemm_symbolic_masked(A, B, Mk, complement=comp, mode="count")
        _, _, crp, cci, _ = Cc.csr()
        np.testing.assert_array_equal(crp, wrp)
        assert len(cci) == 0 and Cc.s.nnz == len(wci)
        Cv, st = T.spgemm_masked_sparse(A, B, Mk, complement=comp)
        _, _, crp, cci, cvv = Cv.csr()
        np.testing.assert_array_equal(crp, wrp)
        np.testing.assert_array_equal(cci, wci)
        assert st["path"] == T.PATH_MASKED
        assert np.all(np.abs(cvv - full[4][sel]) <= 1e-10 * fmag[4][sel])
        Cp, _ = T.spgemm_masked_sparse(A, B, Mk, complement=comp, semiring="plus_pair")
        assert np.array_equal(Cp.csr()[3], wci) and (Cp.csr()[4] >= 1.0).all()
    for bad in (dict(complement=2), dict(semiring=9)):
        with pytest.raises(_lib.TsgError) as e:
            T.spgemm_masked_sparse(A, B, Mk, **bad)
        assert e.value.rc == ERR_INVALID
    with pytest.raises(_lib.TsgError) as e:
        T.spgemm_symbolic_masked(A, B, Mk, complement=2)
    assert e.value.rc == ERR_INVALID
