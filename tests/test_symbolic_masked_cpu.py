"""CPU-side checks of the masked symbolic SpGEMM interface (no GPU needed): the
header declares the three calls, _lib._SIGS binds them with the header's
argument lists, libtsg.so exports them, tsg_symbolic_info is unchanged, and
Context.spgemm_symbolic's keyword defaults keep the unmasked call on the
symbol it has always used."""
import ctypes as C
import inspect
import re

import pytest

from spgemm_amd import _lib

MASKED = ["tsg_dev_spgemm_symbolic_masked", "tsg_spgemm_csr_symbolic_masked", "tsg_spgemm_csr_masked_sparse"]


def _declaration(name):
    """the header's parameter list of a function, comments removed, one string per parameter"""
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, f"include/tsg.h does not declare {name}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_three_calls():
    syms = _lib.header_symbols()
    for s in MASKED:
        assert s in syms, f"include/tsg.h does not declare {s}"
    d = _declaration("tsg_dev_spgemm_symbolic_masked")
    assert [p.split()[-1].lstrip("*") for p in d] == ["ctx", "A", "B", "Mask", "complement", "mode", "stream",
                                                       "Cpattern", "info", "stats"]
    h = _declaration("tsg_spgemm_csr_symbolic_masked")
    assert [p.split()[-1].lstrip("*") for p in h] == ["A", "B", "Mask", "complement", "mode", "C", "stats"]
    v = _declaration("tsg_spgemm_csr_masked_sparse")
    assert [p.split()[-1].lstrip("*") for p in v] == ["A", "B", "Mask", "complement", "semiring", "C", "stats"]
    txt = open(_lib.HEADER).read()
    assert not re.search(r"complemented or valued masks[^.]*not supported", " ".join(txt.split()))


def test_sigs_bind_the_three_calls_like_the_header():
    ctype = lambda p: C.c_int if re.match(r"int \w+$", p) else "ptr"
    for s in MASKED:
        assert s in _lib._SIGS, f"{s} is not bound in _lib._SIGS"
        args, res = _lib._SIGS[s]
        decl = _declaration(s)
        assert res is C.c_int and len(args) == len(decl)
        for a, p in zip(args, decl):
            assert (a is C.c_int) == (ctype(p) is C.c_int), (s, p)
    dev = _lib._SIGS["tsg_dev_spgemm_symbolic_masked"][0]
    old = _lib._SIGS["tsg_dev_spgemm_symbolic"][0]
    # the unmasked call's list with the mask and the sense put in after B
    assert dev == old[:3] + [C.POINTER(_lib.DevCSR), C.c_int] + old[3:]
    assert dev[8] == C.POINTER(_lib.SymbolicInfo)


def test_library_exports_the_three_calls():
    L = _lib.lib()
    for s in MASKED:
        assert hasattr(L, s), f"libtsg.so does not export {s}"
        assert getattr(L, s).argtypes == _lib._SIGS[s][0] and getattr(L, s).restype is C.c_int


def test_symbolic_info_is_unchanged():
    assert [n for n, _ in _lib.SymbolicInfo._fields_] == ["products", "nnzC", "rows_class", "units", "b_rows_sorted"]
    assert C.sizeof(_lib.SymbolicInfo) == 8 + 8 + 32 + 8 + 8
    txt = open(_lib.HEADER).read()
    assert len(re.findall(r"typedef\s+struct\s+tsg_symbolic_info\b", txt)) == 1
    assert "tsg_symbolic_masked_info" not in txt


class _Recorder:
    """stands in for the loaded library: records which symbol a call went to"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


def test_mask_none_takes_the_unmasked_symbol(monkeypatch):
    from spgemm_amd import device

    sig = inspect.signature(device.Context.spgemm_symbolic).parameters
    assert list(sig)[:5] == ["self", "A", "B", "mode", "stream"]  # (the positional order callers rely on)
    assert sig["mode"].default == "pattern" and sig["mask"].default is None and sig["complement"].default is False
    ms = inspect.signature(device.Context.spgemm_masked_sparse).parameters
    assert list(ms)[:4] == ["self", "A", "B", "Mask"]
    assert (ms["complement"].default, ms["semiring"].default, ms["mode"].default) == (False, "plus_times", "auto")

    class _Op:
        def struct(self):
            return _lib.DevCSR()

    rec = _Recorder()
    monkeypatch.setattr(device, "lib", lambda: rec)
    ctx = object.__new__(device.Context)
    ctx.ptr = C.c_void_p()
    ctx.spgemm_symbolic(_Op(), _Op())
    ctx.spgemm_symbolic(_Op(), _Op(), "count", None)
    assert [c[0] for c in rec.calls] == ["tsg_dev_spgemm_symbolic"] * 2
    assert len(rec.calls[0][1]) == len(_lib._SIGS["tsg_dev_spgemm_symbolic"][0])
    assert rec.calls[1][1][3] == 1
    rec.calls.clear()
    ctx.spgemm_symbolic(_Op(), _Op(), mask=_Op(), complement=True)
    ctx.spgemm_symbolic(_Op(), _Op(), "count", mask=_Op())
    assert [c[0] for c in rec.calls] == ["tsg_dev_spgemm_symbolic_masked"] * 2
    assert len(rec.calls[0][1]) == len(_lib._SIGS["tsg_dev_spgemm_symbolic_masked"][0])
    assert (rec.calls[0][1][4], rec.calls[0][1][5]) == (1, 0) and (rec.calls[1][1][4], rec.calls[1][1][5]) == (0, 1)
    ctx.ptr = C.c_void_p()  # (nothing to destroy)


def test_host_layer_entry_points():
    from spgemm_amd import tilespgemm as T
    a = inspect.signature(T.spgemm_symbolic_masked).parameters
    assert list(a) == ["A", "B", "Mask", "complement", "mode"]
    assert a["complement"].default is False and a["mode"].default == "pattern"
    b = inspect.signature(T.spgemm_masked_sparse).parameters
    assert list(b) == ["A", "B", "Mask", "complement", "semiring"]
    assert b["complement"].default is False and b["semiring"].default == "plus_times"


def test_design_names_the_section():
    import os
    design = open(os.path.join(os.path.dirname(_lib.HEADER), "..", "DESIGN.md")).read()
    assert "### 3.11" in design
    sec = design[design.index("### 3.11"):design.index("## 4. Oracle")]
    for k in ("k_sym_packed", "k_sym_set", "k_sym_window", "k_sym_hub_seg", "k_sym_hub_fill"):
        assert k in sec, f"DESIGN.md section 3.11's resource table lacks {k}"
