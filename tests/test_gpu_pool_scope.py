"""The device API's error contract (include/tsg.h): a tsg_dev_* call that fails
has drained its stream, returned every pool block it allocated and zeroed its
output, and the context stays usable.  Checked on a device.Context (the host
layer's lease would hide a leak) with the allocator's two diagnostics: its
counters (pool_stats) and a one-shot allocation failure (fail_alloc), swept
over every allocation a route makes.  Pattern bit-exact, values within 1e-10
relative to |A||B|, against the oracle, as in the routes' own tests."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
from _cases import hub_rows_case, numeric_mixed_case
from test_gpu_band import _banded
from spgemm_amd import synth
from spgemm_amd import tilespgemm as T
from spgemm_amd._lib import DevCSR, DevTiles, NumericInfo, Stats, lib
from spgemm_amd.device import Context, DeviceCSR

pytestmark = pytest.mark.gpu

OK, OOM = 0, -3


def _real(M, seed):
    """the CSR with uniform(-1, 1) values"""
    m, n, rp, ci = M[:4]
    return m, n, rp, ci, np.random.default_rng(seed).uniform(-1, 1, len(ci))


def _oracle_product(A, B):
    """(rowptr, col, values, |A||B| values) of A*B"""
    ref = O.gustavson(O.OMat.from_csr(*A), O.OMat.from_csr(*B)).csr()
    mag = O.gustavson(O.OMat.from_csr(*A[:4], np.abs(A[4])), O.OMat.from_csr(*B[:4], np.abs(B[4]))).csr()
    return ref[2], ref[3], ref[4], mag[4]


def _same_csr(got, ref):
    rp, ci, vv, mag = ref
    np.testing.assert_array_equal(got[0], rp)
    np.testing.assert_array_equal(got[1], ci)
    assert np.all(np.abs(got[2] - vv) <= 1e-10 * mag)


def _pointers(out):
    """the struct's pool arrays: its non-null pointer fields"""
    if isinstance(out, C.c_void_p):  # (a numeric plan: its memory is not the pool's)
        return 0
    return sum(1 for name, tp in out._fields_ if tp is C.c_void_p and getattr(out, name))


def _zeroed(out):
    return not out.value if isinstance(out, C.c_void_p) else bytes(out) == bytes(C.sizeof(out))


def _dev(M):
    return DeviceCSR.from_host(*M)


class SpgemmRoute:
    """one tsg_dev_spgemm call on a forced path"""

    def __init__(self, env, path, A, B):
        self.env, self.path, self.A, self.B = env, path, A, B
        self.ref = None

    def prepare(self):
        self.dA, self.dB = _dev(self.A), _dev(self.B)
        if self.ref is None:
            self.ref = _oracle_product(self.A, self.B)

    def stages(self):
        def spgemm(ctx, state):
            c, st = DevCSR(), Stats()
            rc = lib().tsg_dev_spgemm(ctx.ptr, C.byref(self.dA.struct()), C.byref(self.dB.struct()), 16, 16, None,
                                      C.byref(c), C.byref(st))
            state["C"], state["path"] = c, st.path
            return rc, c
        return [spgemm]

    def result(self, ctx, state):
        assert state["path"] == self.path
        c = state["C"]
        _, _, rp, ci, vv = ctx.to_host(c)
        return rp.copy(), ci.copy(), vv.copy()

    def check(self, res):
        _same_csr(res, self.ref)

    def same(self, res, r0):
        _same_csr(res, (r0[0], r0[1], r0[2], self.ref[3]))

    def cleanup(self, ctx, state):
        pass


class TileApiRoute(SpgemmRoute):
    """tsg_dev_transpose, csr2tile_row_major, csr2tile_col_major, tilespgemm,
    tile2csr in sequence, each on the outputs of the ones before"""

    def __init__(self, A, B):
        super().__init__({}, None, A, B)

    def prepare(self):
        super().prepare()
        self.ref_t = O.transpose(O.OMat.from_csr(*self.A)).csr()

    def stages(self):
        L, a, b = lib(), self.dA.struct(), self.dB.struct()

        def transpose(ctx, s):
            s["At"] = DevCSR()
            return L.tsg_dev_transpose(ctx.ptr, C.byref(a), None, C.byref(s["At"])), s["At"]

        def row_major(ctx, s):
            s["tA"] = DevTiles()
            return L.tsg_dev_csr2tile_row_major(ctx.ptr, C.byref(a), 16, 16, None, C.byref(s["tA"])), s["tA"]

        def col_major(ctx, s):
            s["tB"] = DevTiles()
            return L.tsg_dev_csr2tile_col_major(ctx.ptr, C.byref(b), 16, 16, None, C.byref(s["tB"])), s["tB"]

        def tilespgemm(ctx, s):
            s["tC"] = DevTiles()
            return L.tsg_dev_tilespgemm(ctx.ptr, C.byref(s["tA"]), C.byref(s["tB"]), None, C.byref(s["tC"]),
                                        None), s["tC"]

        def tile2csr(ctx, s):
            s["C"] = DevCSR()
            return L.tsg_dev_tile2csr(ctx.ptr, C.byref(s["tC"]), None, C.byref(s["C"])), s["C"]

        return [transpose, row_major, col_major, tilespgemm, tile2csr]

    def result(self, ctx, state):
        _, _, rp, ci, vv = ctx.to_host(state["C"])
        _, _, trp, tci, tvv = ctx.to_host(state["At"])
        return rp.copy(), ci.copy(), vv.copy(), trp.copy(), tci.copy(), tvv.copy()

    def check(self, res):
        _same_csr(res[:3], self.ref)
        np.testing.assert_array_equal(res[3], self.ref_t[2])
        np.testing.assert_array_equal(res[4], self.ref_t[3])
        np.testing.assert_array_equal(res[5], self.ref_t[4])

    def same(self, res, r0):
        _same_csr(res[:3], (r0[0], r0[1], r0[2], self.ref[3]))
        for x, y in zip(res[3:], r0[3:]):
            np.testing.assert_array_equal(x, y)


class NumericPlanRoute:
    """tsg_dev_numeric_plan_create on the mixed-class patterns"""
    env = {}

    def prepare(self):
        import torch
        A, B = numeric_mixed_case()
        self.A = (*A, np.random.default_rng(5).uniform(-1, 1, len(A[3])))
        self.B = (*B, np.random.default_rng(6).uniform(-1, 1, len(B[3])))
        self.dA, self.dB = _dev(self.A), _dev(self.B)
        self.ref = _oracle_product(self.A, self.B)
        m, n = self.A[0], self.B[1]
        rp, ci = self.ref[0], self.ref[1]
        self.dC = DeviceCSR(m, n, torch.from_numpy(rp.astype(np.int32)).cuda(),
                            torch.from_numpy(ci.astype(np.int32)).cuda(), None)

    def stages(self):
        def create(ctx, s):
            s["plan"], s["info"] = C.c_void_p(), NumericInfo()
            rc = lib().tsg_dev_numeric_plan_create(ctx.ptr, C.byref(self.dA.struct()), C.byref(self.dB.struct()),
                                                   C.byref(self.dC.struct()), None, C.byref(s["plan"]),
                                                   C.byref(s["info"]))
            return rc, s["plan"]
        return [create]

    def result(self, ctx, state):
        import torch
        out = torch.full((len(self.ref[1]),), float("nan"), dtype=torch.float64, device="cuda")
        rc = lib().tsg_dev_numeric_run(ctx.ptr, state["plan"], self.dA.val.data_ptr(), self.dB.val.data_ptr(),
                                       out.data_ptr(), None, None)
        assert rc == OK
        return state["info"].as_dict(), out.cpu().numpy()

    def check(self, res):
        info, vals = res
        assert all(c > 0 for c in info["rows_class"]) and info["nnzC"] == len(self.ref[1])
        assert np.all(np.abs(vals - self.ref[2]) <= 1e-10 * self.ref[3])

    def same(self, res, r0):
        assert res[0] == r0[0]
        assert np.all(np.abs(res[1] - r0[1]) <= 1e-10 * self.ref[3])

    def cleanup(self, ctx, state):
        if state.get("plan"):
            assert lib().tsg_dev_numeric_plan_destroy(ctx.ptr, state["plan"]) == OK
            state["plan"] = C.c_void_p()


def _shuffled_rows(M, seed):
    """the same matrix, every row's entries in a random order"""
    m, n, rp, ci, vv = M
    rng = np.random.default_rng(seed)
    order = np.concatenate([rp[i] + rng.permutation(rp[i + 1] - rp[i]) for i in range(m)]).astype(np.int64)
    return m, n, rp, ci[order], vv[order]


def _routes():
    band = _real(_banded(200, 8, seed=3), 30)
    hub_a, hub_b, _ = hub_rows_case()
    hub_a, hub_b = _real(hub_a, 43), _real(hub_b, 44)
    tiny = _real(synth.random_csr(50, 50, nnz_per_row=4, seed=7), 31)
    ta = _real(synth.random_csr(300, 300, nnz_per_row=4, seed=8), 32)
    tb = _real(synth.random_csr(300, 300, nnz_per_row=4, seed=9), 33)
    rows = {"TSG_PATH": "rows"}
    return {
        "band": SpgemmRoute({"TSG_PATH": "band"}, T.PATH_BAND, band, band),
        "rows-hub": SpgemmRoute(rows, T.PATH_ROWS, hub_a, hub_b),
        "rows-hub-checked-scan": SpgemmRoute({**rows, "TSG_ROWS_CHECKED_SCAN": "1"}, T.PATH_ROWS, hub_a, hub_b),
        "rows-tiny": SpgemmRoute(rows, T.PATH_ROWS, tiny, tiny),
        "tiles-step2-elem": SpgemmRoute({"TSG_PATH": "tiles", "TSG_STEP2_MODE": "elem"}, T.PATH_TILES, ta, tb),
        "tiles-step2-tile": SpgemmRoute({"TSG_PATH": "tiles", "TSG_STEP2_MODE": "tile"}, T.PATH_TILES, ta, tb),
        "tiles-unsorted-b": SpgemmRoute({"TSG_PATH": "tiles"}, T.PATH_TILES, ta, _shuffled_rows(tb, 10)),
        "tile-api": TileApiRoute(ta, tb),
        "numeric-plan": NumericPlanRoute(),
    }


ROUTES = ["band", "rows-hub", "rows-hub-checked-scan", "rows-tiny", "tiles-step2-elem", "tiles-step2-tile",
          "tiles-unsorted-b", "tile-api", "numeric-plan"]


@pytest.fixture(scope="module")
def routes():
    return _routes()


def _run(ctx, route):
    """the route's stages in turn, up to the first that fails: (state, [(rc,
    out, the pool's counters before the stage)])"""
    state, done = {}, []
    for stage in route.stages():
        before = ctx.pool_stats()
        rc, out = stage(ctx, state)
        done.append((rc, out, before))
        if rc != OK:
            break
    return state, done


@pytest.mark.parametrize("name", ROUTES)
def test_failed_allocation_leaks_nothing(routes, name, monkeypatch):
    route = routes[name]
    for k in ("TSG_PATH", "TSG_STEP2_MODE", "TSG_ROWS_CHECKED_SCAN", "TSG_DR_PER_ROW", "TSG_STAGE_EVENTS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in route.env.items():
        monkeypatch.setenv(k, v)
    route.prepare()
    ctx = Context(0)
    try:
        # 1. success leaves only the outputs
        assert ctx.pool_stats()["live_blocks"] == 0
        state, done = _run(ctx, route)
        assert [rc for rc, _, _ in done] == [OK] * len(route.stages())
        first = ctx.pool_stats()
        assert first["live_blocks"] == sum(_pointers(out) for _, out, _ in done)
        r0 = route.result(ctx, state)
        route.check(r0)
        route.cleanup(ctx, state)
        K = first["allocs"]
        assert K > 0
        # 2. a failure at every allocation site
        failed, fell_back = [], []
        for N in range(4 * K + 1):
            ctx.reset()
            assert not ctx.fail_alloc(N)
            state, done = _run(ctx, route)
            if ctx.fail_alloc(-1):  # still pending: the call makes fewer than N + 1 allocations
                assert [rc for rc, _, _ in done] == [OK] * len(route.stages())
                route.cleanup(ctx, state)
                break
            rc, out, before = done[-1]
            assert rc in (OK, OOM), (N, rc)
            if rc == OOM:
                now = ctx.pool_stats()
                assert (now["live_blocks"], now["live_bytes"]) == (before["live_blocks"], before["live_bytes"]), N
                assert _zeroed(out), N
                failed.append(N)
            else:  # a soft fallback took the failure
                assert len(done) == len(route.stages())
                route.same(route.result(ctx, state), r0)
                fell_back.append(N)
            route.cleanup(ctx, state)
        else:
            pytest.fail(f"an injected failure still fired at the {4 * K}th allocation (the first run made {K})")
        print(f"{name}: K = {K}, failed at {len(failed)} sites, fell back at {fell_back}, "
              f"reserved {first['reserved_bytes']}")
        assert failed and failed[0] == 0
        # 3. the context survives
        ctx.reset()
        state, done = _run(ctx, route)
        assert [rc for rc, _, _ in done] == [OK] * len(route.stages())
        route.same(route.result(ctx, state), r0)
        route.cleanup(ctx, state)
        assert ctx.pool_stats()["reserved_bytes"] <= first["reserved_bytes"]
    finally:
        ctx.close()
