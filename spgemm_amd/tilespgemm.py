"""Host-side mirror of the reference's TileSpGEMM operator interface.

Same names, argument meaning and error behaviour as the reference's host
functions (paths under /root/reference/src), each running the gfx950 HIP
kernels of libtsg.so through the C ABI (include/tsg.h):

  mmio_allinone(path)                -> Matrix        mmio_highlevel.h:593-759
  values_pos_mod10(A)                                  main.cu:111-112
  transpose(A)                       -> Matrix        utils.h:161-198 (on the GPU)
  nnzcub(A, B)                       -> int           main.cu:155-162 (on the GPU)
  csr2tile_row_major(A, tm, tn)                        csr2tile.h:205-277
  csr2tile_col_major(B, tm, tn)                        csr2tile.h:279-506
  tilespgemm(A, B, tm, tn, nnzCub)   -> (C, info)     tilespgemm-cuda.h:2220-2844
  tile2csr(C, tm, tn)                                  tile2csr.h:72-140
  spgemm(A, B, tm, tn)               -> (Matrix, stats)  one-shot CSR -> CSR
  spgemm_numeric(A, B, C)            -> stats         values only, on C's known pattern
  spgemm_masked(A, B, C, mode, semiring) -> stats     A*B at the entries of the mask C only
  spgemm_semiring(A, B, semiring)    -> (Matrix, stats)  the full product over a semiring
  spgemm_symbolic_masked(A, B, M, complement, mode) -> (Matrix, stats)  the pattern of A*B inside / outside M
  spgemm_masked_sparse(A, B, M, complement, semiring) -> (Matrix, stats)  C<M> / C<!M>, reached entries only
  ewise(A, B, mode, op, alpha, beta) -> (Matrix, stats)  element-wise union / intersection / difference

Errors raise TsgError (the reference exits or silently misbehaves instead).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SMatrix, Stats, check, lib

_CSR_FIELDS = ("rowpointer", "columnindex", "value")

# stats["path"]: the CSR-in -> CSR-out route that ran (include/tsg.h TSG_PATH_*)
PATH_TILES, PATH_BAND, PATH_ROWS = 0, 2, 3  # (1: the retired fused path)
PATH_NUMERIC = 4  # spgemm_numeric / NumericPlan.run
PATH_MASKED = 5  # spgemm_masked / MaskedPlan.run
# masked modes (include/tsg.h TSG_MASKED_*): per-row choice | all rows row-wise | all rows on the dot leg
MASKED_AUTO, MASKED_ROWS, MASKED_DOT = 0, 1, 2
MASKED_MODES = {"auto": MASKED_AUTO, "rows": MASKED_ROWS, "dot": MASKED_DOT}
PATH_SYMBOLIC = 6  # spgemm_symbolic / Context.spgemm_symbolic
# symbolic modes (include/tsg.h TSG_SYMBOLIC_*): row pointers and columns | row pointers only
SYMBOLIC_PATTERN, SYMBOLIC_COUNT = 0, 1
SYMBOLIC_MODES = {"pattern": SYMBOLIC_PATTERN, "count": SYMBOLIC_COUNT}


# semirings of the numeric and masked plans (include/tsg.h TSG_SEMIRING_*)
SEMIRINGS = {"plus_times": 0, "min_plus": 1, "max_plus": 2, "max_times": 3, "max_min": 4, "min_max": 5,
             "plus_pair": 6}


PATH_EWISE = 7  # ewise / Context.ewise
# element-wise modes and binary ops (include/tsg.h TSG_EWISE_* / TSG_BINOP_*)
EWISE_MODES = {"union": 0, "intersect": 1, "difference": 2}
BINOPS = {"plus": 0, "times": 1, "min": 2, "max": 3, "first": 4, "second": 5}


def semiring_identity(name):
    """the semiring's additive identity -- what an entry no product reaches gets:
    0.0, +inf or -inf (name: a key of SEMIRINGS or a TSG_SEMIRING_* value)"""
    out = C.c_double(0.0)
    check("tsg_semiring_identity", lib().tsg_semiring_identity(SEMIRINGS.get(name, name), C.byref(out)))
    return out.value


def _view(ptr, n, dt):
    if n <= 0 or not ptr:
        return np.zeros(0, dtype=dt)
    return np.ctypeslib.as_array(ptr, shape=(int(n),)).astype(dt, copy=True)


class Matrix:
    """Owns one SMatrix.  Arrays set from numpy are borrowed (kept alive here and
    detached before tsg_matrix_destroy); library-filled arrays are owned."""

    def __init__(self):
        self.s = SMatrix()
        self._keep = []
        self._borrowed = set()

    def __del__(self):
        try:
            for f in self._borrowed:
                setattr(self.s, f, None)
            if _lib._lib is not None:
                _lib._lib.tsg_matrix_destroy(C.byref(self.s))
        except Exception:
            pass

    @classmethod
    def from_csr(cls, m, n, rowptr, col, val, is_symmetric=0):
        """A Matrix on the given CSR arrays (kept alive here).  val=None gives a pattern: the
        value field stays NULL, which the calls that read no values accept (a
        structural ewise)."""
        o = cls()
        rp = np.ascontiguousarray(rowptr, dtype=np.int32)
        ci = np.ascontiguousarray(col, dtype=np.int32)
        vv = np.ascontiguousarray(val, dtype=np.float64) if val is not None else None  # (None: a pattern, value NULL)
        if rp.shape[0] != m + 1 or (vv is not None and ci.shape[0] != vv.shape[0]) or int(rp[-1]) != ci.shape[0]:
            raise ValueError("inconsistent CSR arrays")
        o._keep = [rp, ci, vv]
        o._borrowed = set(_CSR_FIELDS)
        o.s.m, o.s.n, o.s.nnz, o.s.isSymmetric = m, n, ci.shape[0], is_symmetric
        o.s.rowpointer = rp.ctypes.data_as(C.POINTER(C.c_int))
        o.s.columnindex = ci.ctypes.data_as(C.POINTER(C.c_int))
        if vv is not None:
            o.s.value = vv.ctypes.data_as(C.POINTER(C.c_double))
        return o

    @classmethod
    def alias(cls, A):
        """B := A sharing A's CSR arrays (src/main.cu:145-151)."""
        o = cls()
        o._keep = [A]
        o._borrowed = set(_CSR_FIELDS)
        o.s.m, o.s.n, o.s.nnz = A.s.m, A.s.n, A.s.nnz
        o.s.rowpointer, o.s.columnindex, o.s.value = A.s.rowpointer, A.s.columnindex, A.s.value
        return o

    @property
    def shape(self):
        return (self.s.m, self.s.n)

    def csr(self):
        s = self.s
        return (s.m, s.n, _view(s.rowpointer, s.m + 1, np.int32),
                _view(s.columnindex, s.nnz, np.int32), _view(s.value, s.nnz, np.float64))

    def tiles(self, ptr_rows, mask_words, csc=False):
        s = self.s
        d = dict(tilem=s.tilem, tilen=s.tilen, numtile=s.numtile,
                 tile_ptr=_view(s.tile_ptr, s.tilem + 1, np.int32),
                 tile_columnidx=_view(s.tile_columnidx, s.numtile, np.int32),
                 tile_rowidx=_view(s.tile_rowidx, s.numtile, np.int32),
                 tile_nnz=_view(s.tile_nnz, s.numtile + 1, np.int32),
                 tile_csr_Ptr=_view(s.tile_csr_Ptr, s.numtile * ptr_rows, np.uint16),
                 tile_csr_Col=_view(s.tile_csr_Col, s.nnz, np.uint16),
                 tile_csr_Value=_view(s.tile_csr_Value, s.nnz, np.float64),
                 mask=_view(s.mask, s.numtile * ptr_rows * mask_words, np.uint16))
        if csc:
            d["csc_tile_ptr"] = _view(s.csc_tile_ptr, s.tilen + 1, np.int32)
            d["csc_tile_rowidx"] = _view(s.csc_tile_rowidx, s.numtile, np.int32)
        return d


def mmio_allinone(path):
    A = Matrix()
    check("tsg_mmio_allinone", lib().tsg_mmio_allinone(path.encode(), C.byref(A.s)))
    return A


def values_pos_mod10(A):
    lib().tsg_values_pos_mod10(C.byref(A.s))


def transpose(A):
    B = Matrix()
    check("tsg_transpose", lib().tsg_transpose(C.byref(A.s), C.byref(B.s)))
    return B


def nnzcub(A, B):
    out = C.c_ulonglong(0)
    check("tsg_nnzcub", lib().tsg_nnzcub(C.byref(A.s), C.byref(B.s), C.byref(out)))
    return int(out.value)


def csr2tile_row_major(A, tile_size_m=16, tile_size_n=16):
    check("tsg_csr2tile_row_major", lib().tsg_csr2tile_row_major(C.byref(A.s), tile_size_m, tile_size_n))


def csr2tile_col_major(B, tile_size_m=16, tile_size_n=16):
    check("tsg_csr2tile_col_major", lib().tsg_csr2tile_col_major(C.byref(B.s), tile_size_m, tile_size_n))


def tilespgemm(A, B, tile_size_m=16, tile_size_n=16, nnzCub=0, filename=None):
    """C = A*B on tiled inputs; returns (C, info) where info mirrors the
    reference's out-parameters (src/tilespgemm-cuda.h:2228-2235)."""
    Cm = Matrix()
    nnzC = C.c_ulonglong(0)
    outs = [C.c_double(0) for _ in range(7)]
    rc = lib().tsg_tilespgemm(C.byref(A.s), C.byref(B.s), C.byref(Cm.s), None, None, 0, 0.0, 0.0,
                              C.c_ulonglong(nnzCub), C.byref(nnzC), C.byref(outs[0]), C.byref(outs[1]),
                              C.byref(outs[2]), (filename or "").encode(), C.byref(outs[3]),
                              C.byref(outs[4]), C.byref(outs[5]), C.byref(outs[6]),
                              tile_size_m, tile_size_n)
    check("tsg_tilespgemm", rc)
    info = dict(nnzC=int(nnzC.value), compression_rate=outs[0].value, time_tile=outs[1].value,
                gflops_tile=outs[2].value, time_step1=outs[3].value, time_step2=outs[4].value,
                time_step3=outs[5].value, time_malloc=outs[6].value)
    return Cm, info


def tile2csr(Cm, tile_size_m=16, tile_size_n=16):
    check("tsg_tile2csr", lib().tsg_tile2csr(C.byref(Cm.s), tile_size_m, tile_size_n))


def spgemm_numeric(A, B, Cm):
    """Numeric-only product on a known pattern: Cm's rowpointer / columnindex
    given (strictly ascending columns per row, containing A*B's pattern), Cm's
    values overwritten with those of A*B.  Returns the stats dict."""
    st = Stats()
    check("tsg_spgemm_csr_numeric", lib().tsg_spgemm_csr_numeric(C.byref(A.s), C.byref(B.s), C.byref(Cm.s),
                                                                 C.byref(st)))
    return st.as_dict()


def spgemm_masked(A, B, Cm, mode="auto", semiring="plus_times"):
    """Masked product: Cm's rowpointer / columnindex are the mask (strictly
    ascending columns per row), Cm's values are overwritten with the entries of
    A*B at the mask's positions (0.0 where no product reaches); products
    elsewhere are dropped.  mode: "auto", "rows" or "dot" (or a TSG_MASKED_*
    value).  semiring: a key of SEMIRINGS (or a TSG_SEMIRING_* value): its sum
    and product, its identity where no product reaches.  Returns the stats
    dict."""
    st = Stats()
    check("tsg_spgemm_csr_masked_semiring", lib().tsg_spgemm_csr_masked_semiring(
        C.byref(A.s), C.byref(B.s), C.byref(Cm.s), MASKED_MODES.get(mode, mode), SEMIRINGS.get(semiring, semiring),
        C.byref(st)))
    return st.as_dict()


def spgemm_semiring(A, B, semiring):
    """One-shot CSR -> CSR over a semiring (a key of SEMIRINGS or a
    TSG_SEMIRING_* value): C's pattern is A*B's structural one, its values the
    semiring's sums.  Returns (C Matrix, stats dict of the numeric run)."""
    Cm = Matrix()
    st = Stats()
    check("tsg_spgemm_csr_semiring", lib().tsg_spgemm_csr_semiring(C.byref(A.s), C.byref(B.s), C.byref(Cm.s),
                                                                   SEMIRINGS.get(semiring, semiring), C.byref(st)))
    return Cm, st.as_dict()


def spgemm_symbolic(A, B, mode="pattern"):
    """Symbolic product: the structural pattern of A*B without values (A's and
    B's values are not read).  mode: "pattern" (row pointers and columns) or
    "count" (row pointers only; or a TSG_SYMBOLIC_* value).  Returns (C Matrix
    whose csr() has an empty value array -- and empty columns in count mode --,
    stats dict)."""
    Cm = Matrix()
    st = Stats()
    check("tsg_spgemm_csr_symbolic", lib().tsg_spgemm_csr_symbolic(C.byref(A.s), C.byref(B.s), C.byref(Cm.s),
                                                                   SYMBOLIC_MODES.get(mode, mode), C.byref(st)))
    return Cm, st.as_dict()


def spgemm_symbolic_masked(A, B, Mask, complement=False, mode="pattern"):
    """Masked symbolic product: the pattern of A*B restricted to the entries of
    the structural mask (a Matrix with A's rows and B's columns, columns
    strictly ascending per row; its values are not read), or with
    complement=True to the entries outside it.  mode and the result as in
    spgemm_symbolic."""
    Cm = Matrix()
    st = Stats()
    check("tsg_spgemm_csr_symbolic_masked", lib().tsg_spgemm_csr_symbolic_masked(
        C.byref(A.s), C.byref(B.s), C.byref(Mask.s), int(complement), SYMBOLIC_MODES.get(mode, mode), C.byref(Cm.s),
        C.byref(st)))
    return Cm, st.as_dict()


def spgemm_masked_sparse(A, B, Mask, complement=False, semiring="plus_times"):
    """One-shot C<Mask> (complement=True: C<!Mask>) = A*B over a semiring with
    GraphBLAS mask semantics: C holds exactly the entries that a product
    reaches and the mask admits -- none carries an identity that was merely
    filled in (spgemm_masked writes one at every mask entry).  Returns (C
    Matrix, stats dict of the masked run)."""
    Cm = Matrix()
    st = Stats()
    check("tsg_spgemm_csr_masked_sparse", lib().tsg_spgemm_csr_masked_sparse(
        C.byref(A.s), C.byref(B.s), C.byref(Mask.s), int(complement), SEMIRINGS.get(semiring, semiring),
        C.byref(Cm.s), C.byref(st)))
    return Cm, st.as_dict()


def ewise(A, B, mode="union", op="plus", alpha=1.0, beta=1.0):
    """Element-wise combination of two Matrices of one shape, both with strictly
    ascending columns per row: C's pattern is A u B ("union"), A n B
    ("intersect") or A \\ B ("difference"); an entry stored in both holds
    op(alpha * a, beta * b) (op: a key of BINOPS), one stored in A alone
    alpha * a, in B alone beta * b.  A Matrix A without values makes the call
    structural (C has none either).  mode / op: names, or TSG_EWISE_* /
    TSG_BINOP_* values.  Returns (C Matrix, stats dict)."""
    Cm = Matrix()
    st = Stats()
    md, bo = EWISE_MODES.get(mode, mode), BINOPS.get(op, op)
    # (an unknown name reaches the library as -1, as in Context.ewise: it answers TSG_ERR_INVALID)
    md, bo = (md if isinstance(md, int) else -1), (bo if isinstance(bo, int) else -1)
    check("tsg_ewise_csr", lib().tsg_ewise_csr(C.byref(A.s), C.byref(B.s), md, bo, float(alpha), float(beta),
                                               C.byref(Cm.s), C.byref(st)))
    return Cm, st.as_dict()


def spgemm(A, B, tile_size_m=16, tile_size_n=16):
    """One-shot CSR -> CSR on the GPU; returns (C Matrix, stats dict)."""
    Cm = Matrix()
    st = Stats()
    check("tsg_spgemm_csr", lib().tsg_spgemm_csr(C.byref(A.s), C.byref(B.s), C.byref(Cm.s),
                                                 tile_size_m, tile_size_n, C.byref(st)))
    return Cm, st.as_dict()
