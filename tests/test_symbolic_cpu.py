"""CPU-side checks of the symbolic SpGEMM interface (no GPU needed): the header
declares the calls and constants, the ctypes tsg_symbolic_info mirrors the
header's struct, the Python constants match, and the class caps the GPU tests
build their cases from are the ones tsg_internal.h names."""
import ctypes as C
import os
import re

from spgemm_amd import _lib

SYMBOLIC = ["tsg_dev_spgemm_symbolic", "tsg_spgemm_csr_symbolic"]
# the class caps and window of DESIGN.md section 3.9 (tests/test_gpu_symbolic.py crafts rows on both sides)
CAPS = dict(kSymPackedProducts=32, kSymSetWaveProducts=512, kSymSetProducts=4096, kSymWindowProducts=65536,
            kSymWindow=131072, kSymHubUnitProducts=4096)


def _define(name):
    txt = open(_lib.HEADER).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1))


def test_header_declares_the_symbolic_functions_and_constants():
    syms = _lib.header_symbols()
    for s in SYMBOLIC:
        assert s in syms, f"include/tsg.h does not declare {s}"
        assert s in _lib._SIGS, f"{s} is not bound in _lib._SIGS"
    assert _define("TSG_SYMBOLIC_PATTERN") == 0
    assert _define("TSG_SYMBOLIC_COUNT") == 1
    assert _define("TSG_PATH_SYMBOLIC") == 6


def _header_struct_fields(name):
    txt = open(_lib.HEADER).read()
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(.+?)\s*\b([A-Za-z_]\w*)\s*(?:\[(\d+)\])?$", decl, flags=re.S)
        out.append((" ".join(m.group(1).split()), m.group(2), int(m.group(3)) if m.group(3) else 0))
    return out


def test_symbolic_info_matches_header():
    ctype = {"long long": C.c_longlong, "int": C.c_int}
    want = []
    for ty, name, count in _header_struct_fields("tsg_symbolic_info"):
        want.append((name, ctype[ty] * count if count else ctype[ty]))
    got = list(_lib.SymbolicInfo._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    assert [n for n, _ in got] == ["products", "nnzC", "rows_class", "units", "b_rows_sorted"]
    for (n, a), (_, b) in zip(got, want):
        assert C.sizeof(a) == C.sizeof(b), n
    assert C.sizeof(_lib.SymbolicInfo) == 8 + 8 + 32 + 8 + 8  # (the int padded to the struct's 8-byte alignment)
    d = _lib.SymbolicInfo().as_dict()
    assert sorted(d) == sorted(n for n, _ in got) and d["rows_class"] == [0, 0, 0, 0]


def test_python_constants_match_header():
    from spgemm_amd import tilespgemm as T
    assert T.PATH_SYMBOLIC == _define("TSG_PATH_SYMBOLIC") == 6
    assert T.SYMBOLIC_MODES == {"pattern": _define("TSG_SYMBOLIC_PATTERN"), "count": _define("TSG_SYMBOLIC_COUNT")}
    assert callable(T.spgemm_symbolic)


def test_class_caps_are_the_documented_ones():
    txt = open(os.path.join(os.path.dirname(_lib.HEADER), "..", "spgemm_amd", "csrc", "tsg_internal.h")).read()
    for name, want in CAPS.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, txt)
        assert m, f"tsg_internal.h does not name {name}"
        assert int(m.group(1)) == want, name
    design = open(os.path.join(os.path.dirname(_lib.HEADER), "..", "DESIGN.md")).read()
    sec = design[design.index("### 3.9"):design.index("## 4. Oracle")]
    for want in ("65,536", "4,096", "131,072"):
        assert want in sec, f"DESIGN.md section 3.9 does not state {want}"
