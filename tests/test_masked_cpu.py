"""CPU-side checks of the masked SpGEMM interface (no GPU needed): include/tsg.h
declares the four functions, libtsg.so exports them, the ctypes tsg_masked_info
mirrors the header's struct field for field, and the path and mode constants
match the Python side."""
import ctypes as C
import os
import re

import pytest

from spgemm_amd import _lib

MASKED = ["tsg_dev_masked_plan_create", "tsg_dev_masked_run", "tsg_dev_masked_plan_destroy",
          "tsg_spgemm_csr_masked"]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_header_declares_the_masked_functions():
    syms = _lib.header_symbols()
    for s in MASKED:
        assert s in syms, f"include/tsg.h does not declare {s}"


def test_masked_functions_bound_and_exported(L):
    for s in MASKED:
        assert s in _lib._SIGS, f"{s} is not bound in _lib._SIGS"
        assert hasattr(L, s), f"libtsg.so does not export {s}"
        assert getattr(L, s).restype is C.c_int


def _header_struct_fields(name):
    """(type, field) of every member, one per declarator (`long long a, b;` is two)"""
    txt = open(_lib.HEADER).read()
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        first, *more = [d.strip() for d in decl.split(",")]
        m = re.match(r"(.+?)\s*\b([A-Za-z_]\w*)$", first)
        out.append((m.group(1), m.group(2)))
        out += [(m.group(1), d) for d in more]
    return out


def test_masked_info_matches_header():
    ctype = {"long long": C.c_longlong, "int": C.c_int}
    want = [(name, ctype[ty]) for ty, name in _header_struct_fields("tsg_masked_info")]
    got = list(_lib.MaskedInfo._fields_)
    assert got == want
    assert [n for n, _ in got] == ["products", "nnzM", "rows_rowwise", "rows_dot", "products_rowwise", "dot_work",
                                   "dot_units", "a_rows_sorted", "b_rows_sorted", "b_no_repeats", "dot_eligible"]
    assert C.sizeof(_lib.MaskedInfo) == 7 * 8 + 4 * 4
    assert sorted(_lib.MaskedInfo().as_dict()) == sorted(n for n, _ in got)


def test_masked_constants_match_header():
    from spgemm_amd import tilespgemm as T
    txt = open(_lib.HEADER).read()
    val = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, txt).group(1))
    assert val("TSG_PATH_MASKED") == T.PATH_MASKED == 5
    assert val("TSG_MASKED_AUTO") == T.MASKED_AUTO == T.MASKED_MODES["auto"] == 0
    assert val("TSG_MASKED_ROWS") == T.MASKED_ROWS == T.MASKED_MODES["rows"] == 1
    assert val("TSG_MASKED_DOT") == T.MASKED_DOT == T.MASKED_MODES["dot"] == 2
