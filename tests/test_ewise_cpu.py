"""CPU-side checks of the element-wise interface (no GPU needed): the header
declares the three calls with the agreed argument lists, _lib._SIGS binds them
(c_double exactly at alpha and beta), libtsg.so exports them, tsg_ewise_info is
64 bytes, the Python entry points have the agreed signatures and defaults,
DESIGN.md documents the kernels, and the header no longer calls accumulation
unsupported."""
import ctypes as C
import inspect
import os
import re

from spgemm_amd import _lib

EWISE = ["tsg_dev_ewise", "tsg_ewise_csr", "tsg_binop_name"]


def _declaration(name, ret=r"int"):
    """the header's parameter list of a function, comments removed, one string per parameter"""
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    m = re.search(r"%s\s*\b%s\s*\(([^)]*)\)\s*;" % (ret, name), txt)
    assert m, f"include/tsg.h does not declare {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _names(decl):
    return [p.split()[-1].lstrip("*") for p in decl]


def test_header_declares_the_three_calls():
    syms = _lib.header_symbols()
    for s in EWISE:
        assert s in syms, f"include/tsg.h does not declare {s}"
    d = _declaration("tsg_dev_ewise")
    assert _names(d) == ["ctx", "A", "B", "mode", "op", "alpha", "beta", "stream", "C", "info", "stats"]
    assert d[5] == "double alpha" and d[6] == "double beta" and d[3] == "int mode" and d[4] == "int op"
    assert d[9] == "tsg_ewise_info *info" and d[8] == "tsg_dev_csr *C"
    h = _declaration("tsg_ewise_csr")
    assert _names(h) == ["A", "B", "mode", "op", "alpha", "beta", "C", "stats"]
    assert h[4] == "double alpha" and h[5] == "double beta"
    assert _declaration("tsg_binop_name", ret=r"const char \*") == ["int op"]
    txt = open(_lib.HEADER).read()
    want = {"TSG_PATH_EWISE": 7, "TSG_EWISE_UNION": 0, "TSG_EWISE_INTERSECT": 1, "TSG_EWISE_DIFFERENCE": 2,
            "TSG_BINOP_PLUS": 0, "TSG_BINOP_TIMES": 1, "TSG_BINOP_MIN": 2, "TSG_BINOP_MAX": 3, "TSG_BINOP_FIRST": 4,
            "TSG_BINOP_SECOND": 5}
    for k, v in want.items():
        m = re.search(r"#define\s+%s\s+(-?\d+)\b" % k, txt)
        assert m and int(m.group(1)) == v, k


def test_sigs_bind_the_three_calls_like_the_header():
    for s in EWISE:
        assert s in _lib._SIGS, f"{s} is not bound in _lib._SIGS"
    kind = lambda p: C.c_double if p.startswith("double ") else C.c_int if re.match(r"int \w+$", p) else "ptr"
    for s in ("tsg_dev_ewise", "tsg_ewise_csr"):
        args, res = _lib._SIGS[s]
        decl = _declaration(s)
        assert res is C.c_int and len(args) == len(decl)
        for a, p in zip(args, decl):
            k = kind(p)
            assert (a is C.c_double) == (k is C.c_double), (s, p)
            assert (a is C.c_int) == (k is C.c_int), (s, p)
        assert [i for i, a in enumerate(args) if a is C.c_double] == [_names(decl).index("alpha"),
                                                                      _names(decl).index("beta")]
    dev = _lib._SIGS["tsg_dev_ewise"][0]
    assert dev[1] == dev[2] == dev[8] == C.POINTER(_lib.DevCSR) and dev[9] == C.POINTER(_lib.EwiseInfo)
    assert dev[10] == C.POINTER(_lib.Stats)
    assert _lib._SIGS["tsg_binop_name"] == ([C.c_int], C.c_char_p)


def test_library_exports_the_three_calls():
    L = _lib.lib()
    for s in EWISE:
        assert hasattr(L, s), f"libtsg.so does not export {s}"
        assert getattr(L, s).argtypes == _lib._SIGS[s][0] and getattr(L, s).restype is _lib._SIGS[s][1]
    names = [L.tsg_binop_name(i) for i in range(6)]  # (host only: no device is touched)
    assert names == [b"plus", b"times", b"min", b"max", b"first", b"second"]
    assert L.tsg_binop_name(6) is None and L.tsg_binop_name(-1) is None


def test_ewise_info_layout():
    assert [n for n, _ in _lib.EwiseInfo._fields_] == ["nnzA", "nnzB", "both", "nnzC", "rows_class", "units"]
    assert C.sizeof(_lib.EwiseInfo) == 64
    assert _lib.EwiseInfo.rows_class.size == 24 and _lib.EwiseInfo.units.offset == 56
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    m = re.search(r"typedef\s+struct\s+tsg_ewise_info\s*\{(.*?)\}\s*tsg_ewise_info\s*;", txt, flags=re.S)
    assert m and " ".join(m.group(1).split()) == ("long long nnzA, nnzB; long long both; long long nnzC; "
                                                  "long long rows_class[3]; long long units;")
    # tsg_stats itself does not change
    assert C.sizeof(_lib.Stats) == 8 * 8 + 6 * 8 + 8 + 8


def test_python_entry_points():
    from spgemm_amd import device
    from spgemm_amd import tilespgemm as T
    assert T.PATH_EWISE == 7
    assert T.EWISE_MODES == {"union": 0, "intersect": 1, "difference": 2}
    assert T.BINOPS == {"plus": 0, "times": 1, "min": 2, "max": 3, "first": 4, "second": 5}
    h = inspect.signature(T.ewise).parameters
    assert list(h) == ["A", "B", "mode", "op", "alpha", "beta"]
    assert [h[k].default for k in ("mode", "op", "alpha", "beta")] == ["union", "plus", 1.0, 1.0]
    e = inspect.signature(device.Context.ewise).parameters
    assert list(e) == ["self", "A", "B", "mode", "op", "alpha", "beta", "stream"]
    assert [e[k].default for k in ("mode", "op", "alpha", "beta", "stream")] == ["union", "plus", 1.0, 1.0, None]
    a = inspect.signature(device.Context.spgemm_accum).parameters
    assert list(a) == ["self", "C0", "A", "B", "semiring", "accum", "mask", "complement", "stream"]
    assert [a[k].default for k in ("semiring", "accum", "mask", "complement", "stream")] == ["plus_times", None, None,
                                                                                           False, None]


class _Recorder:
    """stands in for the loaded library: records which symbol a call went to"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


def test_context_ewise_passes_modes_ops_and_scalars(monkeypatch):
    from spgemm_amd import device

    class _Op:
        def struct(self):
            return _lib.DevCSR()

    rec = _Recorder()
    monkeypatch.setattr(device, "lib", lambda: rec)
    ctx = object.__new__(device.Context)
    ctx.ptr = C.c_void_p()
    ctx.ewise(_Op(), _Op())
    ctx.ewise(_Op(), _Op(), "difference", "second", 2.5, -1)
    ctx.ewise(_Op(), _Op(), 3, 6)
    ctx.ewise(_Op(), _Op(), "nonsense", "nonsense")  # (unknown names reach the library as -1: it refuses them)
    assert [c[0] for c in rec.calls] == ["tsg_dev_ewise"] * 4
    assert all(len(c[1]) == len(_lib._SIGS["tsg_dev_ewise"][0]) for c in rec.calls)
    assert [c[1][3:7] for c in rec.calls] == [(0, 0, 1.0, 1.0), (2, 5, 2.5, -1.0), (3, 6, 1.0, 1.0),
                                              (-1, -1, 1.0, 1.0)]
    assert all(isinstance(c[1][5], float) and isinstance(c[1][6], float) for c in rec.calls)
    ctx.ptr = C.c_void_p()  # (nothing to destroy)


def test_design_names_the_section():
    design = open(os.path.join(os.path.dirname(_lib.HEADER), "..", "DESIGN.md")).read()
    assert "### 3.12" in design
    assert design.index("### 3.11") < design.index("### 3.12") < design.index("## 4. Oracle")
    sec = design[design.index("### 3.12"):design.index("## 4. Oracle")]
    for k in ("k_ew_classify", "k_ew_unit_counts", "k_ew_tile_rows", "k_ew_packed", "k_ew_wave", "k_ew_tile"):
        assert k in sec, f"DESIGN.md section 3.12 lacks {k}"
    assert "untested" in sec  # (the int32 overflow of nnz(C): no test of a few seconds reaches it)


def test_header_no_longer_calls_accumulation_unsupported():
    txt = " ".join(re.sub(r"\s*\*\s+", " ", open(_lib.HEADER).read()).split())
    assert not re.search(r"accumulation into an existing C[^.]*(not supported|out of scope)", txt)
    assert "Valued masks remain out of scope" in txt and "tsg_dev_ewise" in txt
    integ = " ".join(open(os.path.join(os.path.dirname(_lib.HEADER), "..", "INTEGRATION.md")).read().split())
    assert not re.search(r"accumulation into an existing C remain", integ)
    assert "Valued masks remain out of scope" in integ
