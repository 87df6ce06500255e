"""CPU-side checks of the semiring interface (no GPU needed): the header
declares the calls and the TSG_SEMIRING_* constants, libtsg.so exports the
calls and _lib binds them, the Python table matches the header, and the two
host-only calls (identity, name) answer as documented."""
import ctypes as C
import inspect
import math
import re

from spgemm_amd import _lib
from spgemm_amd import tilespgemm as T

FUNCTIONS = ["tsg_semiring_identity", "tsg_semiring_name", "tsg_dev_numeric_run_semiring",
             "tsg_dev_masked_run_semiring", "tsg_spgemm_csr_semiring", "tsg_spgemm_csr_masked_semiring"]
NAMES = ["plus_times", "min_plus", "max_plus", "max_times", "max_min", "min_max", "plus_pair"]
IDENTITY = [0.0, math.inf, -math.inf, -math.inf, -math.inf, math.inf, 0.0]
INVALID = -1  # TSG_ERR_INVALID


def _defines():
    txt = open(_lib.HEADER).read()
    return {n.lower(): int(v) for n, v in re.findall(r"#define\s+TSG_SEMIRING_([A-Z_]+)\s+(\d+)", txt)}


def test_header_declares_the_semiring_functions_and_constants():
    syms = _lib.header_symbols()
    for s in FUNCTIONS:
        assert s in syms, f"include/tsg.h does not declare {s}"
    assert _defines() == {n: i for i, n in enumerate(NAMES)}


def test_library_exports_and_binds_the_functions():
    L = _lib.lib()
    for s in FUNCTIONS:
        assert s in _lib._SIGS, f"{s} is not bound in _lib._SIGS"
        assert getattr(L, s).argtypes == _lib._SIGS[s][0]
    # the semiring is the third argument of the run calls, the last before the stats of the one-shot calls
    for s in ("tsg_dev_numeric_run_semiring", "tsg_dev_masked_run_semiring"):
        assert _lib._SIGS[s][0][2] is C.c_int and len(_lib._SIGS[s][0]) == len(_lib._SIGS[s[:-9]][0]) + 1
    assert _lib._SIGS["tsg_spgemm_csr_semiring"][0][3] is C.c_int
    assert _lib._SIGS["tsg_spgemm_csr_masked_semiring"][0][3:5] == [C.c_int, C.c_int]


def test_python_table_matches_header():
    assert T.SEMIRINGS == _defines() == {n: i for i, n in enumerate(NAMES)}
    assert callable(T.spgemm_semiring) and callable(T.semiring_identity)
    assert inspect.signature(T.spgemm_masked).parameters["semiring"].default == "plus_times"
    from spgemm_amd import device
    for cls in (device.NumericPlan, device.MaskedPlan):
        assert inspect.signature(cls.run).parameters["semiring"].default == "plus_times"
    assert callable(device.Context.spgemm_semiring)


def test_semiring_identity():
    L = _lib.lib()
    for sr, want in enumerate(IDENTITY):
        out = C.c_double(float("nan"))
        assert L.tsg_semiring_identity(sr, C.byref(out)) == 0
        assert out.value == want and math.copysign(1.0, out.value) == math.copysign(1.0, want)
        assert T.semiring_identity(NAMES[sr]) == want == T.semiring_identity(sr)
    for bad in (7, -1):
        out = C.c_double(123.0)
        assert L.tsg_semiring_identity(bad, C.byref(out)) == INVALID
        assert out.value == 123.0
    assert L.tsg_semiring_identity(0, None) == INVALID


def test_semiring_name_round_trips():
    L = _lib.lib()
    for sr, name in enumerate(NAMES):
        assert L.tsg_semiring_name(sr) == name.encode()
        assert T.SEMIRINGS[L.tsg_semiring_name(sr).decode()] == sr
    assert L.tsg_semiring_name(7) is None and L.tsg_semiring_name(-1) is None
