"""CPU-side checks of the numeric-only SpGEMM interface (no GPU needed): every
tsg_* function include/tsg.h declares is bound in _lib._SIGS and exported by
libtsg.so, and the ctypes tsg_numeric_info mirrors the header's struct."""
import ctypes as C
import os
import re

import pytest

from spgemm_amd import _lib

NUMERIC = ["tsg_dev_numeric_plan_create", "tsg_dev_numeric_run", "tsg_dev_numeric_plan_destroy",
           "tsg_spgemm_csr_numeric"]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_header_declares_the_numeric_functions():
    syms = _lib.header_symbols()
    for s in NUMERIC:
        assert s in syms, f"include/tsg.h does not declare {s}"


def test_every_header_symbol_bound_and_exported(L):
    for s in _lib.header_symbols():
        assert s in _lib._SIGS, f"{s} is not bound in _lib._SIGS"
        assert hasattr(L, s), f"libtsg.so does not export {s}"
    for s in NUMERIC:
        assert getattr(L, s).restype is C.c_int


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


def test_numeric_info_matches_header():
    ctype = {"long long": C.c_longlong, "int": C.c_int}
    want = []
    for ty, name, count in _header_struct_fields("tsg_numeric_info"):
        want.append((name, ctype[ty] * count if count else ctype[ty]))
    got = list(_lib.NumericInfo._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    assert [n for n, _ in got] == ["products", "nnzC", "rows_class", "split_units", "b_rows_sorted"]
    for (n, a), (_, b) in zip(got, want):
        assert C.sizeof(a) == C.sizeof(b), n
    assert C.sizeof(_lib.NumericInfo) == 8 + 8 + 32 + 8 + 8  # (the int padded to the struct's 8-byte alignment)


def test_path_constant_matches_header():
    from spgemm_amd import tilespgemm as T
    txt = open(_lib.HEADER).read()
    assert int(re.search(r"#define\s+TSG_PATH_NUMERIC\s+(\d+)", txt).group(1)) == T.PATH_NUMERIC == 4
