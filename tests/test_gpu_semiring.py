"""Semiring SpGEMM (tsg_dev_numeric_run_semiring / tsg_dev_masked_run_semiring,
tsg_spgemm_csr_semiring / _masked_semiring and their Python layers) against a
numpy reference kept here: every element product (i, j, a, b) expanded with
np.repeat, the semiring's product applied, sorted by (i, j), reduced with
np.minimum / np.maximum / np.add .reduceat, laid on the pattern with the
semiring's identity elsewhere.

Comparison: the five min / max semirings bit for bit (each value is one IEEE
add, multiply, min or max, and min / max do not round); plus_pair exact
integers; plus_times through the new entries within the project's
1e-10 * sum |a||b|.  The value sets make a stray 0.0 lose: positive operands
for the min semirings, negative for the max ones (A positive, B negative for
max_times), and one mixed-sign set for all.  Every run writes into a NaN-filled
c_val."""
import os

import numpy as np
import pytest

from conftest import FIXTURES, GOLDEN
import _oracle as O
from _cases import numeric_mixed_case
from spgemm_amd import _lib
from spgemm_amd import tilespgemm as T
from test_gpu_masked import _edge_case, _from_keys, _keys, _rmat_case
from test_gpu_numeric import _shuffled_rows, _split_case, _window_case

pytestmark = pytest.mark.gpu

SEMIRINGS = ["plus_times", "min_plus", "max_plus", "max_times", "max_min", "min_max", "plus_pair"]
MINMAX = SEMIRINGS[1:6]
IDENTITY = dict(plus_times=0.0, min_plus=np.inf, max_plus=-np.inf, max_times=-np.inf, max_min=-np.inf,
                min_max=np.inf, plus_pair=0.0)
MUL = dict(plus_times=np.multiply, min_plus=np.add, max_plus=np.add, max_times=np.multiply, max_min=np.minimum,
           min_max=np.maximum, plus_pair=lambda a, b: np.ones(len(a)))
ADD = dict(plus_times=np.add, min_plus=np.minimum, max_plus=np.maximum, max_times=np.maximum, max_min=np.maximum,
           min_max=np.minimum, plus_pair=np.add)
MODES = ("dot", "rows", "auto")


@pytest.fixture(scope="module")
def ctx():
    from spgemm_amd.device import Context
    c = Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- the reference
class Products:
    """every element product of A*B's patterns, expanded once per case: the A
    entry e and the B entry q of each, sorted by (row, column); keys are the
    distinct row * n + column, first the start of each key's run"""

    def __init__(self, A, B):
        m, _, rpa, cia = A[:4]
        _, n, rpb, cib = B[:4]
        self.m, self.n = m, n
        blen = np.diff(rpb.astype(np.int64))[cia]
        e = np.repeat(np.arange(len(cia)), blen)
        off = np.arange(int(blen.sum())) - np.repeat(np.cumsum(blen) - blen, blen)
        q = rpb.astype(np.int64)[cia][e] + off
        rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(rpa))
        key = rows[e] * n + cib[q]
        order = np.argsort(key, kind="stable")
        self.e, self.q, key = e[order], q[order], key[order]
        self.first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, int)
        self.keys = key[self.first]

    def pattern(self):
        return _from_keys(self.m, self.n, self.keys)

    def reduce(self, sr, av, bv):
        """per distinct key: the semiring's sum, and sum |a||b| (the plus_times bound's magnitude)"""
        if not len(self.keys):
            return np.zeros(0), np.zeros(0)
        a, b = (av[self.e], bv[self.q]) if sr != "plus_pair" else (self.e, self.q)
        x = MUL[sr](a, b)
        mag = np.add.reduceat(np.abs(x), self.first) if sr == "plus_times" else None
        return ADD[sr].reduceat(x, self.first), mag

    def on(self, pat, sr, av, bv):
        """the reference laid on the pattern pat (which may lack reference keys:
        a mask): (expected, magnitude, reached)"""
        val, mag = self.reduce(sr, av, bv)
        pk = _keys(pat)
        exp, mg, reached = np.full(len(pk), IDENTITY[sr]), np.zeros(len(pk)), np.zeros(len(pk), dtype=bool)
        if len(pk) and len(self.keys):
            pos = np.minimum(np.searchsorted(self.keys, pk), len(self.keys) - 1)
            reached = self.keys[pos] == pk
            exp[reached] = val[pos[reached]]
            if mag is not None:
                mg[reached] = mag[pos[reached]]
        return exp, mg, reached


def _value_sets(sr, na, nb, seed):
    """(tag, a values, b values): the set on which a stray 0.0 would win this
    semiring's sum, and the mixed-sign set every semiring gets"""
    rng = np.random.default_rng(seed)
    pos = lambda k: rng.uniform(0.5, 2.0, k)
    neg = lambda k: rng.uniform(-2.0, -0.5, k)
    out = []
    if sr in ("min_plus", "min_max"):
        out.append(("positive", pos(na), pos(nb)))
    elif sr in ("max_plus", "max_min"):
        out.append(("negative", neg(na), neg(nb)))
    elif sr == "max_times":
        out.append(("a_pos_b_neg", pos(na), neg(nb)))
    out.append(("mixed", rng.uniform(-1, 1, na), rng.uniform(-1, 1, nb)))
    return out


def _compare(got, exp, mag, reached, sr, what):
    assert not np.isnan(got).any(), (what, int(np.isnan(got).sum()))
    assert np.array_equal(got[~reached], exp[~reached]), (what, "an unreached entry is not the identity")
    if sr == "plus_times":
        err = np.abs(got - exp)
        assert np.all(err <= 1e-10 * mag), (what, float(np.max(err / np.maximum(mag, 1e-300))))
    else:
        bad = np.flatnonzero(got != exp)
        assert len(bad) == 0, (what, len(bad), got[bad[:4]], exp[bad[:4]])


def _dev(M):
    from spgemm_amd.device import DeviceCSR
    m, n, rp, ci = M[:4]
    return DeviceCSR.from_host(m, n, rp, ci, np.ones(len(ci)))


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(plan, nout, sr, av, bv):
    """one run into a NaN-filled c_val"""
    import torch
    out = torch.full((nout,), float("nan"), dtype=torch.float64, device="cuda")
    a, b = (None, None) if av is None else (_cuda(av), _cuda(bv))
    got, st = plan.run(a, b, out=out, semiring=sr)
    assert got.data_ptr() == out.data_ptr()
    return got.cpu().numpy(), st


def _check_all_semirings(plan, prod, pat, A, B, seed, what, path):
    for sr in SEMIRINGS:
        for tag, av, bv in _value_sets(sr, len(A[3]), len(B[3]), seed):
            got, st = _run(plan, len(pat[3]), sr, av, bv)
            _compare(got, *prod.on(pat, sr, av, bv), sr, (what, sr, tag))
            assert st["path"] == path and st["nnzC"] == len(pat[3])


def _numeric_case(ctx, A, B, seed, what, pat=None):
    prod = Products(A, B)
    pat = prod.pattern() if pat is None else pat
    plan = ctx.numeric_plan(_dev(A), _dev(B), _dev(pat))
    info = plan.info
    _check_all_semirings(plan, prod, pat, A, B, seed, what, T.PATH_NUMERIC)
    plan.close()
    return info


def _raises_invalid(fn):
    with pytest.raises(_lib.TsgError) as ei:
        fn()
    assert ei.value.rc == -1  # TSG_ERR_INVALID


# ---------------------------------------------------------------- numeric plan
def test_semiring_numeric_mixed_classes(ctx):
    A, B = numeric_mixed_case()
    info = _numeric_case(ctx, A, B, 5, "mixed")
    assert all(c > 0 for c in info["rows_class"]) and info["split_units"] > 0, info


@pytest.mark.parametrize("b_sorted", [True, False], ids=["sortedB", "shuffledB"])
@pytest.mark.parametrize("kind", ["products", "long_b_row"])
def test_semiring_numeric_split_rows(ctx, kind, b_sorted):
    """the identity fill, the global atomic sums, units of one B row's pieces"""
    A, B = _split_case(kind)
    if not b_sorted:
        B = _shuffled_rows(B, 17)
    info = _numeric_case(ctx, A, B, 6, kind)
    assert info["rows_class"][3] >= 1 and info["split_units"] >= 2
    if kind == "long_b_row":
        assert info["split_units"] >= 5 * 2


@pytest.mark.parametrize("b_sorted", [True, False], ids=["sortedB", "shuffledB"])
def test_semiring_numeric_window_rows(ctx, b_sorted):
    """the dense-window kernel: sums combined in registers over runs of equal B
    rows, long B rows straight to the window"""
    A, B = _window_case()
    if not b_sorted:
        B = _shuffled_rows(B, 19)
    info = _numeric_case(ctx, A, B, 12, "window")
    assert info["rows_class"] == [1, 3, 0, 0]


def _superset_case():
    rng = np.random.default_rng(41)
    m, k, n = 300, 300, 400
    rows = [np.sort(rng.choice(k, size=int(rng.integers(0, 12)), replace=False)) for _ in range(m)]
    rows[7] = np.zeros(0, dtype=np.int64)  # no products: its pattern entries are all unreached
    lens = [len(r) for r in rows]
    A = (m, k, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.concatenate(rows).astype(np.int32))
    brows = [np.sort(rng.choice(n, size=int(rng.integers(0, 16)), replace=False)) for _ in range(k)]
    lens = [len(r) for r in brows]
    B = (k, n, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.concatenate(brows).astype(np.int32))
    return A, B


def test_semiring_numeric_superset_pattern(ctx):
    """A*B's pattern plus one extra column per row (three on the row without
    products): the unreached entries equal the identity exactly"""
    A, B = _superset_case()
    prod = Products(A, B)
    m, n = prod.m, prod.n
    rng = np.random.default_rng(42)
    have = set(prod.keys.tolist())
    extra = []
    for i in range(m):
        for _ in range(3 if i == 7 else 1):
            j = int(rng.integers(0, n))
            while i * n + j in have:
                j = (j + 1) % n
            have.add(i * n + j)
            extra.append(i * n + j)
    pat = _from_keys(m, n, np.concatenate([prod.keys, extra]))
    assert len(pat[3]) == len(prod.keys) + m + 2 and pat[2][8] - pat[2][7] == 3
    plan = ctx.numeric_plan(_dev(A), _dev(B), _dev(pat))
    for sr in SEMIRINGS:
        for tag, av, bv in _value_sets(sr, len(A[3]), len(B[3]), 9):
            got, _ = _run(plan, len(pat[3]), sr, av, bv)
            exp, mag, reached = prod.on(pat, sr, av, bv)
            assert (~reached).sum() == m + 2
            assert np.all(got[~reached] == IDENTITY[sr]), (sr, tag)
            _compare(got, exp, mag, reached, sr, ("superset", sr, tag))
    plan.close()


def test_semiring_numeric_repeated_columns(ctx):
    """x_int_unsorted_dup_77: B rows unsorted and repeating a column -- the
    repeats are combined with the semiring's sum"""
    m, n, rp, ci, _ = O.OMat.load(os.path.join(FIXTURES, "x_int_unsorted_dup_77.mtx")).csr()
    A = (m, n, rp, ci)
    k = _keys(A)
    assert len(np.unique(k)) < len(k), "the fixture no longer repeats a column"
    info = _numeric_case(ctx, A, A, 21, "dup_77")
    assert info["b_rows_sorted"] == 0


def test_semiring_numeric_missing_column(ctx):
    """a pattern lacking one column of A*B: TSG_ERR_INVALID under min_plus too;
    the plans stay usable -- the next call on the full pattern's plan is right"""
    A, B = _superset_case()
    prod = Products(A, B)
    pat = prod.pattern()
    m, n, rp, ci = pat
    row = int(np.argmax(np.diff(rp) >= 3))
    rp2 = rp.copy()
    rp2[row + 1:] -= 1
    short = (m, n, rp2, np.delete(ci, rp[row] + 1))
    dA, dB = _dev(A), _dev(B)
    good, bad = ctx.numeric_plan(dA, dB, _dev(pat)), ctx.numeric_plan(dA, dB, _dev(short))
    _, av, bv = _value_sets("min_plus", len(A[3]), len(B[3]), 31)[0]
    _raises_invalid(lambda: _run(bad, len(short[3]), "min_plus", av, bv))
    got, _ = _run(good, len(ci), "min_plus", av, bv)
    _compare(got, *prod.on(pat, "min_plus", av, bv), "min_plus", "after a miss")
    _raises_invalid(lambda: _run(bad, len(short[3]), "min_plus", av, bv))  # (the plan itself is alive, and says so again)
    bad.close()
    good.close()


def test_semiring_unknown_is_rejected_before_launch(ctx):
    A, B = _superset_case()
    prod = Products(A, B)
    pat = prod.pattern()
    dA, dB, dP = _dev(A), _dev(B), _dev(pat)
    _, av, bv = _value_sets("plus_times", len(A[3]), len(B[3]), 32)[0]
    import torch
    for plan, nout in ((ctx.numeric_plan(dA, dB, dP), len(pat[3])), (ctx.masked_plan(dA, dB, dP, mode="dot"), len(pat[3]))):
        for bad in (7, -1):
            out = torch.full((nout,), float("nan"), dtype=torch.float64, device="cuda")
            _raises_invalid(lambda: plan.run(_cuda(av), _cuda(bv), out=out, semiring=bad))
            assert torch.isnan(out).all(), "c_val was written"
        got, _ = _run(plan, nout, "max_plus", av, bv)  # (the plan is still usable)
        _compare(got, *prod.on(pat, "max_plus", av, bv), "max_plus", "after an unknown semiring")
        plan.close()
    plan = ctx.numeric_plan(dA, dB, dP)
    with pytest.raises(ValueError):
        plan.run(_cuda(av), _cuda(bv), semiring="tropical")
    plan.close()


def test_semiring_plus_pair_reads_no_values(ctx):
    """plus_pair with None values == plus_times with all-ones values, exactly"""
    A, B = numeric_mixed_case()
    pat = Products(A, B).pattern()
    plan = ctx.numeric_plan(_dev(A), _dev(B), _dev(pat))
    pair, _ = _run(plan, len(pat[3]), "plus_pair", None, None)
    ones, _ = _run(plan, len(pat[3]), "plus_times", np.ones(len(A[3])), np.ones(len(B[3])))
    plan.close()
    assert pair.tobytes() == ones.tobytes() and pair.min() >= 1 and pair.max() > 1


# ---------------------------------------------------------------- masked plan
@pytest.mark.parametrize("mode", MODES)
def test_semiring_masked_edges(ctx, mode):
    """A rows of 0, 1, 16, 17, 2,048, 2,049 and 5,000 entries, mask entries on an
    empty A row, the unit cuts: the entries no product reaches are the identity"""
    A, B, mask = _edge_case()
    prod = _edge_products()
    rp = mask[2]
    reached = prod.on(mask, "plus_pair", None, None)[2]
    assert reached.sum() > 50 and not reached[rp[0]:rp[1]].any() and not reached[rp[12]:rp[13]].any()
    plan = ctx.masked_plan(_dev(A), _dev(B), _dev(mask), mode=mode)
    if mode != "auto":
        assert (plan.info["rows_dot"] > 0) == (mode == "dot") and (plan.info["rows_rowwise"] > 0) == (mode == "rows")
    _check_all_semirings(plan, prod, mask, A, B, 301, ("edges", mode), T.PATH_MASKED)
    plan.close()


_edge = {}


def _edge_products():
    if not _edge:
        A, B, _ = _edge_case()
        _edge["p"] = Products(A, B)
    return _edge["p"]


def test_semiring_masked_legs_agree_bytewise(ctx):
    """the 20,000-row R-MAT, its own pattern as mask: the sum's order differs
    between the legs and from run to run of the row-wise leg, the bits do not"""
    A = _rmat_case()["A"]
    dA = _dev(A)
    rows, dot = ctx.masked_plan(dA, dA, dA, mode="rows"), ctx.masked_plan(dA, dA, dA, mode="dot")
    assert rows.info["rows_dot"] == 0 and dot.info["rows_rowwise"] == 0 and dot.info["rows_dot"] > 0
    n = len(A[3])
    for sr in MINMAX + ["plus_pair"]:
        for tag, av, bv in _value_sets(sr, n, n, 201):
            g_rows, _ = _run(rows, n, sr, av, bv)
            g_dot, _ = _run(dot, n, sr, av, bv)
            assert not np.isnan(g_rows).any() and g_rows.tobytes() == g_dot.tobytes(), (sr, tag)
            reached = np.isfinite(g_rows)  # (an edge in no triangle is reached by no product)
            assert reached.any() and np.all(g_rows[~reached] == IDENTITY[sr])
    rows.close()
    dot.close()


@pytest.mark.parametrize("mode", MODES)
def test_semiring_triangle_count(ctx, mode):
    """plus_pair on the strict lower triangle, no values at all"""
    import scipy.sparse as sp
    L = _rmat_case()["L"]
    m, n, rp, ci = L
    S = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(m, n))
    want = (S @ S).multiply(S).sum()
    from spgemm_amd.device import DeviceCSR
    import torch
    dL = DeviceCSR(m, n, torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), None)
    plan = ctx.masked_plan(dL, dL, dL, mode=mode)
    got, _ = _run(plan, len(ci), "plus_pair", None, None)
    plan.close()
    assert want > 0 and got.sum() == want  # (small integers: exact in fp64)


# ---------------------------------------------------------------- full product, host layer
def _golden_operands(name, aat):
    g = np.load(os.path.join(GOLDEN, "ref", f"{name}_aat{aat}_16x16.npz"))
    A = (int(g["A__m"]), int(g["A__n"]), g["A__rowpointer"], g["A__columnindex"])
    B = (int(g["B__m"]), int(g["B__n"]), g["B__rowpointer"], g["B__columnindex"])
    return A, B


@pytest.mark.parametrize("name,aat", [("x_powerlaw_400", 0), ("x_rect_50x130", 1)])
def test_semiring_full_product(ctx, name, aat):
    """Context.spgemm_semiring: the product from the operands alone; its pattern
    is ctx.spgemm's"""
    from spgemm_amd.device import DeviceCSR
    A, B = _golden_operands(name, aat)
    prod = Products(A, B)
    pat = prod.pattern()
    c, _ = ctx.spgemm(_dev(A), _dev(B))
    full = ctx.to_host(c)
    ctx.reset()
    np.testing.assert_array_equal(full[2], pat[2])
    np.testing.assert_array_equal(full[3], pat[3])
    for sr in SEMIRINGS:
        for tag, av, bv in _value_sets(sr, len(A[3]), len(B[3]), 71):
            dA = DeviceCSR.from_host(*A, av)
            dB = DeviceCSR.from_host(*B, bv)
            if sr == "plus_pair":
                dA.val = dB.val = None
            C, info, st = ctx.spgemm_semiring(dA, dB, sr)
            m, n, rp, ci, vv = C.to_host()
            np.testing.assert_array_equal(rp, pat[2])
            np.testing.assert_array_equal(ci, pat[3])
            exp, mag, reached = prod.on(pat, sr, av, bv)
            assert reached.all() and info["nnzC"] == len(ci) and st["path"] == T.PATH_NUMERIC
            _compare(vv, exp, mag, reached, sr, (name, sr, tag))
            ctx.reset()  # (the symbolic pass's pattern is the context's; C's tensors are torch's)


def test_semiring_all_pairs_shortest_paths(ctx):
    """a 64-node digraph with an explicit zero diagonal squared six times under
    min_plus (paths of up to 64 edges) against scipy's shortest_path.  The sums
    associate differently there: 1e-12 relative, not bitwise."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import shortest_path
    from spgemm_amd.device import DeviceCSR
    rng = np.random.default_rng(64)
    n = 64
    rows, vals = [], []
    for i in range(n):
        nb = rng.choice(np.delete(np.arange(n), i), size=int(rng.integers(3, 6)), replace=False)
        cols = np.sort(np.concatenate([nb, [i]]))
        w = rng.uniform(0.5, 2.0, len(cols))
        w[cols == i] = 0.0
        rows.append(cols)
        vals.append(w)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci, vv = np.concatenate(rows).astype(np.int32), np.concatenate(vals)
    off = ci != np.repeat(np.arange(n), np.diff(rp))
    G = sp.csr_matrix((vv[off], (np.repeat(np.arange(n), np.diff(rp))[off], ci[off])), shape=(n, n))
    want = shortest_path(G, method="D", directed=True)
    D = DeviceCSR.from_host(n, n, rp, ci, vv)
    for _ in range(6):
        D, _, _ = ctx.spgemm_semiring(D, D, "min_plus")
    _, _, drp, dci, dv = D.to_host()
    got = np.full((n, n), np.inf)
    got[np.repeat(np.arange(n), np.diff(drp)), dci] = dv
    reach = np.isfinite(want)
    assert reach.sum() > n * n // 2 and np.all(np.diag(got) == 0.0)
    assert np.all(np.isinf(got[~reach]) & (got[~reach] > 0))  # (unreachable: absent or +inf)
    assert np.all(np.abs(got[reach] - want[reach]) <= 1e-12 * want[reach])


def test_semiring_host_layer():
    A, B = _golden_operands("x_powerlaw_400", 0)
    prod = Products(A, B)
    pat = prod.pattern()
    _, av, bv = _value_sets("max_min", len(A[3]), len(B[3]), 81)[0]
    Cm, st = T.spgemm_semiring(T.Matrix.from_csr(*A, av), T.Matrix.from_csr(*B, bv), "max_min")
    got = Cm.csr()
    np.testing.assert_array_equal(got[2], pat[2])
    np.testing.assert_array_equal(got[3], pat[3])
    _compare(got[4], *prod.on(pat, "max_min", av, bv), "max_min", "host max_min")
    assert st["path"] == T.PATH_NUMERIC and st["nnzC"] == len(pat[3])
    mask = _from_keys(A[0], A[1], _keys(A))  # the operand's own pattern
    _, av, bv = _value_sets("min_plus", len(A[3]), len(B[3]), 82)[0]
    for mode in ("auto", "dot"):
        Mm = T.Matrix.from_csr(*mask, np.full(len(mask[3]), np.nan))
        st = T.spgemm_masked(T.Matrix.from_csr(*A, av), T.Matrix.from_csr(*B, bv), Mm, mode, semiring="min_plus")
        exp, mag, reached = prod.on(mask, "min_plus", av, bv)
        assert 0 < reached.sum() and st["path"] == T.PATH_MASKED
        _compare(Mm.csr()[4], exp, mag, reached, "min_plus", ("host masked", mode))
    with pytest.raises(_lib.TsgError):
        T.spgemm_semiring(T.Matrix.from_csr(*A, av), T.Matrix.from_csr(*B, bv), 7)
