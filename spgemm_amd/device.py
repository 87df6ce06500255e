"""Device-resident pipeline: torch tensors hold the inputs in HBM (PyTorch is
plumbing here: device memory, streams, torch.distributed), libtsg.so runs the
gfx950 kernels on them through the tsg_dev_* C ABI.  No CPU fallback: every
call raises TsgError when the HIP library or device is unavailable.
"""
import ctypes as C

import numpy as np

import weakref

from ._lib import DevCSR, EwiseInfo, MaskedInfo, NumericInfo, PoolStats, Stats, SymbolicInfo, TsgError, check, lib
from .tilespgemm import SEMIRINGS

_PLUS_PAIR = SEMIRINGS["plus_pair"]


class DeviceCSR:
    """A CSR matrix resident on a HIP device (torch tensors own the memory)."""

    def __init__(self, m, n, rowptr, col, val):
        self.m, self.n = int(m), int(n)
        self.rowptr, self.col, self.val = rowptr, col, val
        self.nnz = int(col.numel())

    @classmethod
    def from_host(cls, m, n, rowptr, col, val, device="cuda"):
        import torch
        rp = torch.from_numpy(np.ascontiguousarray(rowptr, dtype=np.int32)).to(device)
        ci = torch.from_numpy(np.ascontiguousarray(col, dtype=np.int32)).to(device)
        vv = torch.from_numpy(np.ascontiguousarray(val, dtype=np.float64)).to(device)
        return cls(m, n, rp, ci, vv)

    def struct(self):
        # (built once: the tensors are fixed for the object's life, and a timing
        # loop should not pay for three data_ptr() calls and a ctypes struct per call)
        s = getattr(self, "_struct", None)
        if s is None:
            # (val=None: a pattern only, for Context.numeric_plan)
            s = self._struct = DevCSR(self.m, self.n, self.nnz, self.rowpointer_ptr(), self.col.data_ptr(),
                                      self.val.data_ptr() if self.val is not None else None)
        return s

    def rowpointer_ptr(self):
        return self.rowptr.data_ptr()

    def to_host(self):
        return (self.m, self.n, self.rowptr.cpu().numpy(), self.col.cpu().numpy(),
                self.val.cpu().numpy() if self.val is not None else None)


def _semiring(semiring):
    """the TSG_SEMIRING_* value of a name or a value (an unknown value is passed
    on: the library answers TSG_ERR_INVALID)"""
    if isinstance(semiring, str):
        try:
            return SEMIRINGS[semiring]
        except KeyError:
            raise ValueError(f"unknown semiring {semiring!r}: one of {sorted(SEMIRINGS)}") from None
    return int(semiring)


def _run_values(plan, a_val, b_val, out, nout, sr):
    """checks a run's value tensors; returns (a pointer, b pointer, out).  The
    values may be None for the semiring that reads none ("plus_pair")."""
    import torch
    f64 = torch.float64
    ptrs = [None, None]
    for i, (t, n) in enumerate(((a_val, plan.A.nnz), (b_val, plan.B.nnz))):
        if t is None and sr == _PLUS_PAIR:
            continue
        if t is None or t.dtype != f64 or not t.is_contiguous() or t.numel() != n or not t.is_cuda:
            raise ValueError("values: contiguous float64 device tensors of the patterns' nnz")
        ptrs[i] = t.data_ptr()
    if out is None:
        out = torch.empty(nout, dtype=f64, device=plan.A.rowptr.device)
    elif out.dtype != f64 or not out.is_contiguous() or out.numel() != nout or not out.is_cuda:
        raise ValueError(f"out: a contiguous float64 device tensor of {nout} entries")
    return ptrs[0], ptrs[1], out


class NumericPlan:
    """A tsg_numeric_plan: C = A*B's values on a known C pattern, for products
    repeated with fixed patterns and changing values.  Holds the three pattern
    matrices (their tensors must stay alive and unchanged while the plan lives).
    The plan's device memory survives Context.reset(); closing the context
    closes its plans."""

    def __init__(self, ctx, A, B, Cpattern, stream=None):
        self.ctx, self.A, self.B, self.Cpattern = ctx, A, B, Cpattern
        self.ptr = C.c_void_p()
        info = NumericInfo()
        a, b, c = A.struct(), B.struct(), Cpattern.struct()
        s = C.c_void_p(stream) if stream else None
        check("tsg_dev_numeric_plan_create", lib().tsg_dev_numeric_plan_create(
            ctx.ptr, C.byref(a), C.byref(b), C.byref(c), s, C.byref(self.ptr), C.byref(info)))
        self.info = info.as_dict()
        self.nnzC = Cpattern.nnz

    def run(self, a_val, b_val, out=None, stream=None, raw=False, semiring="plus_times"):
        """out[0:nnzC] := values of A*B for the f64 device tensors a_val / b_val
        laid on the plan's patterns.  Returns (out, stats).  Raises TsgError
        (TSG_ERR_INVALID) when the pattern lacks a column of A*B.  semiring: a
        name of tilespgemm.SEMIRINGS or a TSG_SEMIRING_* value -- the sum and
        the product of that semiring, its identity where no product reaches;
        "plus_pair" reads no values (a_val / b_val may be None); an unknown
        value raises TsgError (TSG_ERR_INVALID) with out untouched."""
        if not self.ptr:
            raise RuntimeError("numeric plan is closed")
        sr = _semiring(semiring)
        pa, pb, out = _run_values(self, a_val, b_val, out, self.nnzC, sr)
        st = Stats()
        s = C.c_void_p(stream) if stream else None
        check("tsg_dev_numeric_run_semiring", lib().tsg_dev_numeric_run_semiring(
            self.ctx.ptr, self.ptr, sr, pa, pb, out.data_ptr(), s, C.byref(st)))
        return out, (st if raw else st.as_dict())

    def close(self):
        if self.ptr and self.ctx.ptr:
            lib().tsg_dev_numeric_plan_destroy(self.ctx.ptr, self.ptr)
        self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MaskedPlan:
    """A tsg_masked_plan: the entries of A*B at a structural mask's positions
    only, for fixed patterns and changing values.  Holds the three pattern
    matrices (their tensors must stay alive and unchanged while the plan lives).
    The plan's device memory survives Context.reset(); closing the context
    closes its plans.  The dot leg's values are bit-reproducible from run to
    run."""

    def __init__(self, ctx, A, B, Mask, mode="auto", stream=None):
        from .tilespgemm import MASKED_MODES
        self.ctx, self.A, self.B, self.Mask = ctx, A, B, Mask
        self.ptr = C.c_void_p()
        info = MaskedInfo()
        a, b, c = A.struct(), B.struct(), Mask.struct()
        s = C.c_void_p(stream) if stream else None
        check("tsg_dev_masked_plan_create", lib().tsg_dev_masked_plan_create(
            ctx.ptr, C.byref(a), C.byref(b), C.byref(c), MASKED_MODES.get(mode, mode), s, C.byref(self.ptr),
            C.byref(info)))
        self.info = info.as_dict()
        self.nnzM = Mask.nnz

    def run(self, a_val, b_val, out=None, stream=None, raw=False, semiring="plus_times"):
        """out[0:nnzM] := the entries of A*B at the mask's positions for the f64
        device tensors a_val / b_val laid on the plan's patterns (0.0 where no
        product reaches).  Returns (out, stats).  semiring: as in
        NumericPlan.run (the semiring's identity where no product reaches;
        "plus_pair" takes None for a_val / b_val)."""
        if not self.ptr:
            raise RuntimeError("masked plan is closed")
        sr = _semiring(semiring)
        pa, pb, out = _run_values(self, a_val, b_val, out, self.nnzM, sr)
        st = Stats()
        s = C.c_void_p(stream) if stream else None
        check("tsg_dev_masked_run_semiring", lib().tsg_dev_masked_run_semiring(
            self.ctx.ptr, self.ptr, sr, pa, pb, out.data_ptr(), s, C.byref(st)))
        return out, (st if raw else st.as_dict())

    def close(self):
        if self.ptr and self.ctx.ptr:
            lib().tsg_dev_masked_plan_destroy(self.ctx.ptr, self.ptr)
        self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """Owns a tsg_context (device, caching allocator, outputs of the last call)."""

    def __init__(self, device=0):
        self.ptr = C.c_void_p()
        self._plans = weakref.WeakSet()
        check("tsg_context_create", lib().tsg_context_create(device, C.byref(self.ptr)))
        self.device = device

    def close(self):
        if self.ptr:
            for p in list(self._plans):  # (tsg_context_destroy frees the plans still alive)
                p.ptr = C.c_void_p()
            lib().tsg_context_destroy(self.ptr)
            self.ptr = C.c_void_p()

    def numeric_plan(self, A, B, Cpattern, stream=None):
        """A NumericPlan for C = A*B on the patterns of the DeviceCSRs A, B and
        Cpattern (values ignored; C's columns strictly ascending per row and
        containing A*B's pattern).  Raises TsgError (TSG_ERR_INVALID) for a
        malformed pattern."""
        p = NumericPlan(self, A, B, Cpattern, stream)
        self._plans.add(p)
        return p

    def masked_plan(self, A, B, Mask, mode="auto", stream=None):
        """A MaskedPlan for C<Mask> = A*B on the patterns of the DeviceCSRs A, B
        and Mask (values ignored; the mask's columns strictly ascending per
        row).  mode: "auto" (per-row choice of leg), "rows" or "dot".  Raises
        TsgError (TSG_ERR_INVALID) for a malformed pattern, an unknown mode, or
        "dot" on operands the dot leg cannot take."""
        p = MaskedPlan(self, A, B, Mask, mode, stream)
        self._plans.add(p)
        return p

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check("tsg_context_reset", lib().tsg_context_reset(self.ptr))

    def pool_stats(self):
        """The allocator's counters (diagnostics): live_blocks, live_bytes,
        reserved_bytes, allocs."""
        st = PoolStats()
        check("tsg_context_pool_stats", lib().tsg_context_pool_stats(self.ptr, C.byref(st)))
        return st.as_dict()

    def fail_alloc(self, nth):
        """Diagnostics: the nth pool allocation from now (0 = the next) fails once
        with TSG_ERR_OOM; nth < 0 clears it.  Returns whether an earlier
        injection was still pending (had not fired)."""
        rc = lib().tsg_context_fail_alloc(self.ptr, nth)
        if rc < 0:
            raise TsgError("tsg_context_fail_alloc", rc)
        return bool(rc)

    def spgemm(self, A, B, tile_m=16, tile_n=16, stream=None, b_sorted=False, raw=False):
        """C = A*B device CSR in -> device CSR out.  Returns (DevCSR struct with
        context-owned pointers, stats dict).  Valid until the next reset().
        b_sorted=True: the caller found B's rows column-sorted (rows_sorted) and B
        has not changed since -- the per-call check is skipped
        (tsg_dev_spgemm_sorted_b).  raw=True: the stats as the tsg_stats struct
        (its as_dict() later: a timing loop keeps the conversion out)."""
        a, b, c, st = A.struct(), B.struct(), DevCSR(), Stats()
        s = C.c_void_p(stream) if stream else None
        if b_sorted:
            check("tsg_dev_spgemm_sorted_b", lib().tsg_dev_spgemm_sorted_b(
                self.ptr, C.byref(a), C.byref(b), 1, tile_m, tile_n, s, C.byref(c), C.byref(st)))
        else:
            check("tsg_dev_spgemm", lib().tsg_dev_spgemm(self.ptr, C.byref(a), C.byref(b), tile_m, tile_n, s,
                                                         C.byref(c), C.byref(st)))
        return c, (st if raw else st.as_dict())

    def spgemm_symbolic(self, A, B, mode="pattern", stream=None, mask=None, complement=False):
        """The structural pattern of A*B without values: (DevCSR struct with
        context-owned row pointers and -- mode "pattern" -- columns, value null;
        info dict; stats dict).  Valid until the next reset().  mode "count":
        row pointers only (columnindex null, nnz set).  A's and B's values are
        not read (DeviceCSRs with val=None are fine); their rows may be unsorted
        and repeat columns.  Raises TsgError: TSG_ERR_INVALID for malformed
        operands or an unknown mode; TSG_ERR_OVERFLOW when nnz(C) exceeds int32
        -- the error's .info then still holds the exact nnzC.
        mask (a DeviceCSR; its values are not read, val=None is fine; columns
        strictly ascending per row): the masked pass
        (tsg_dev_spgemm_symbolic_masked) -- the pattern of A*B restricted to the
        mask's entries, or with complement=True to the entries outside it (a
        BFS step: spgemm_symbolic(F, A, mask=Visited, complement=True)).  info's
        nnzC is then the masked count; products, rows_class and units stay the
        unmasked product's.  complement: a bool, or an int passed through (the
        library refuses values outside {0, 1})."""
        from .tilespgemm import SYMBOLIC_MODES
        a, b, c, info, st = A.struct(), B.struct(), DevCSR(), SymbolicInfo(), Stats()
        s = C.c_void_p(stream) if stream else None
        md = SYMBOLIC_MODES.get(mode, mode)
        md = md if isinstance(md, int) else -1
        if mask is None:
            name = "tsg_dev_spgemm_symbolic"
            rc = lib().tsg_dev_spgemm_symbolic(self.ptr, C.byref(a), C.byref(b), md, s, C.byref(c), C.byref(info),
                                               C.byref(st))
        else:
            name = "tsg_dev_spgemm_symbolic_masked"
            mk = mask.struct()
            rc = lib().tsg_dev_spgemm_symbolic_masked(self.ptr, C.byref(a), C.byref(b), C.byref(mk), int(complement),
                                                      md, s, C.byref(c), C.byref(info), C.byref(st))
        if rc != 0:
            err = TsgError(name, rc)
            err.info = info.as_dict()
            raise err
        return c, info.as_dict(), st.as_dict()

    def spgemm_masked_sparse(self, A, B, Mask, complement=False, semiring="plus_times", mode="auto", stream=None):
        """C<Mask> (or, complement=True, C<!Mask>) = A*B over a semiring with
        GraphBLAS mask semantics: exactly the entries a product reaches and the
        mask admits.  The masked symbolic pass gives the pattern, which is
        copied into torch tensors; a masked plan on it (mode: the plan's,
        "auto" by default) runs once and is closed before returning.  Returns
        (DeviceCSR in torch tensors, the symbolic pass's info dict, the run's
        stats dict).  "plus_pair" reads no values (A.val / B.val may be None);
        Mask's values are never read."""
        sr = _semiring(semiring)
        c, info, _ = self.spgemm_symbolic(A, B, "pattern", stream, mask=Mask, complement=complement)
        Cp = self.to_torch(c, device=A.rowptr.device, stream=stream)
        plan = self.masked_plan(A, B, Cp, mode, stream)
        try:
            out, st = plan.run(A.val, B.val, stream=stream, semiring=sr)
        finally:
            plan.close()
        return DeviceCSR(Cp.m, Cp.n, Cp.rowptr, Cp.col, out), info, st

    def spgemm_plan(self, A, B, stream=None):
        """A NumericPlan for C = A*B from the operands alone: the symbolic pass
        gives C's pattern, which is copied into torch tensors (so it survives
        reset()) and handed to numeric_plan.  The pattern is plan.Cpattern (a
        DeviceCSR with val=None)."""
        c, _, _ = self.spgemm_symbolic(A, B, "pattern", stream)
        return self.numeric_plan(A, B, self.to_torch(c, device=A.rowptr.device, stream=stream), stream)

    def spgemm_semiring(self, A, B, semiring, stream=None):
        """The full product of the DeviceCSRs A and B over a semiring (a name of
        tilespgemm.SEMIRINGS or a TSG_SEMIRING_* value), from the operands
        alone: spgemm_plan (the symbolic pass gives C's pattern, the same for
        every semiring) plus one run; the plan is closed before returning.
        Returns (DeviceCSR in torch tensors, the plan's info dict, stats dict).
        "plus_pair" reads no values (A.val / B.val may be None)."""
        sr = _semiring(semiring)
        plan = self.spgemm_plan(A, B, stream)
        try:
            out, st = plan.run(A.val, B.val, stream=stream, semiring=sr)
            Cp, info = plan.Cpattern, plan.info
        finally:
            plan.close()
        return DeviceCSR(Cp.m, Cp.n, Cp.rowptr, Cp.col, out), info, st

    def ewise(self, A, B, mode="union", op="plus", alpha=1.0, beta=1.0, stream=None):
        """The element-wise combination of the DeviceCSRs A and B (one shape,
        columns strictly ascending per row): C's pattern is A u B ("union"),
        A n B ("intersect") or A \\ B ("difference"); an entry stored in both
        holds op(alpha * a, beta * b) (op: a name of tilespgemm.BINOPS), one
        stored in A alone alpha * a, in B alone beta * b, each rounded once.
        A.val None: the structural call -- C has no values and none is read
        (Visited u N of a BFS).  Returns (DevCSR struct with context-owned
        pointers, info dict, stats dict), valid until the next reset().  mode /
        op: names, or TSG_EWISE_* / TSG_BINOP_* values passed through (the
        library refuses unknown ones).  Raises TsgError: TSG_ERR_INVALID for
        malformed or unsorted operands; TSG_ERR_OVERFLOW when nnz(C) exceeds
        int32 -- the error's .info then still holds the exact nnzC."""
        from .tilespgemm import BINOPS, EWISE_MODES
        a, b, c, info, st = A.struct(), B.struct(), DevCSR(), EwiseInfo(), Stats()
        s = C.c_void_p(stream) if stream else None
        md, bo = EWISE_MODES.get(mode, mode), BINOPS.get(op, op)
        md, bo = (md if isinstance(md, int) else -1), (bo if isinstance(bo, int) else -1)
        rc = lib().tsg_dev_ewise(self.ptr, C.byref(a), C.byref(b), md, bo, float(alpha), float(beta), s, C.byref(c),
                                 C.byref(info), C.byref(st))
        if rc != 0:
            err = TsgError("tsg_dev_ewise", rc)
            err.info = info.as_dict()
            raise err
        return c, info.as_dict(), st.as_dict()

    def spgemm_accum(self, C0, A, B, semiring="plus_times", accum=None, mask=None, complement=False, stream=None):
        """C0 (+)= A*B: the product over a semiring (spgemm_semiring; with mask,
        spgemm_masked_sparse -- C<mask> or, complement=True, C<!mask>, reached
        entries only) combined with the DeviceCSR C0 by an ewise union with the
        op accum -- by default the semiring's own sum: "plus", "min" or "max".
        An entry of C0 the product does not reach is kept as it is, one the
        product alone holds is taken over.  D = spgemm_accum(D, D, A,
        semiring="min_plus") is a Bellman-Ford step.  Returns a DeviceCSR in
        torch tensors."""
        from .tilespgemm import SEMIRINGS
        sr = _semiring(semiring)
        if accum is None:
            name = {v: k for k, v in SEMIRINGS.items()}.get(sr, "")
            accum = "min" if name.startswith("min") else "max" if name.startswith("max") else "plus"
        if mask is None:
            P, _, _ = self.spgemm_semiring(A, B, sr, stream)
        else:
            P, _, _ = self.spgemm_masked_sparse(A, B, mask, complement, sr, stream=stream)
        if C0.nnz == 0:  # (no values to point at: the library would read the call as structural)
            return P
        c, _, _ = self.ewise(C0, P, "union", accum, stream=stream)
        return self.to_torch(c, device=C0.rowptr.device, stream=stream)

    def rows_sorted(self, M, stream=None):
        """whether every row of the device CSR M is strictly column-sorted"""
        m, out = M.struct(), C.c_int(0)
        s = C.c_void_p(stream) if stream else None
        check("tsg_dev_csr_rows_sorted", lib().tsg_dev_csr_rows_sorted(self.ptr, C.byref(m), s, C.byref(out)))
        return bool(out.value)

    def transpose(self, A, stream=None):
        a, c = A.struct(), DevCSR()
        check("tsg_dev_transpose", lib().tsg_dev_transpose(self.ptr, C.byref(a), stream, C.byref(c)))
        return c

    def to_torch(self, c, device="cuda", stream=None):
        """Copy a context-owned DevCSR into torch tensors (D2D)."""
        import torch
        rp = torch.empty(c.m + 1, dtype=torch.int32, device=device)
        ci = torch.empty(max(c.nnz, 1), dtype=torch.int32, device=device)
        vv = torch.empty(max(c.nnz, 1), dtype=torch.float64, device=device) if c.value or not c.nnz else None
        L = lib()
        check("tsg_memcpy_d2d", L.tsg_memcpy_d2d(self.ptr, rp.data_ptr(), c.rowpointer, 4 * (c.m + 1), stream))
        ncol = c.nnz if c.columnindex else 0  # (a symbolic result: no values, in count mode no columns either)
        if ncol:
            check("tsg_memcpy_d2d", L.tsg_memcpy_d2d(self.ptr, ci.data_ptr(), c.columnindex, 4 * c.nnz, stream))
        if c.nnz and c.value:
            check("tsg_memcpy_d2d", L.tsg_memcpy_d2d(self.ptr, vv.data_ptr(), c.value, 8 * c.nnz, stream))
        return DeviceCSR(c.m, c.n, rp, ci[:ncol], vv[: c.nnz] if vv is not None else None)

    def view_torch(self, c):
        """Zero-copy torch views of a context-owned DevCSR (valid until the next
        reset of this context), via __cuda_array_interface__."""
        import torch

        class _Buf:
            def __init__(self, ptr, n, typestr):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr or 0, False),
                                                 "version": 2, "strides": None}

        dev = torch.device("cuda", torch.cuda.current_device())
        rp = torch.as_tensor(_Buf(c.rowpointer, c.m + 1, "<i4"), device=dev)
        if c.nnz and c.columnindex:
            ci = torch.as_tensor(_Buf(c.columnindex, c.nnz, "<i4"), device=dev)
        else:
            ci = torch.empty(0, dtype=torch.int32, device=dev)
        if c.nnz and c.value:
            vv = torch.as_tensor(_Buf(c.value, c.nnz, "<f8"), device=dev)
        elif c.nnz:
            vv = None  # (a symbolic result: no values)
        else:
            vv = torch.empty(0, dtype=torch.float64, device=dev)
        return DeviceCSR(c.m, c.n, rp, ci, vv)

    def to_host(self, c, stream=None):
        rp = np.empty(c.m + 1, dtype=np.int32)
        ci = np.empty(max(c.nnz, 1), dtype=np.int32)
        vv = np.empty(max(c.nnz, 1), dtype=np.float64) if c.value or not c.nnz else None
        L = lib()
        check("tsg_memcpy_d2h", L.tsg_memcpy_d2h(self.ptr, rp.ctypes.data, c.rowpointer, 4 * (c.m + 1), stream))
        ncol = c.nnz if c.columnindex else 0  # (a symbolic result: no values, in count mode no columns either)
        if ncol:
            check("tsg_memcpy_d2h", L.tsg_memcpy_d2h(self.ptr, ci.ctypes.data, c.columnindex, 4 * c.nnz, stream))
        if c.nnz and c.value:
            check("tsg_memcpy_d2h", L.tsg_memcpy_d2h(self.ptr, vv.ctypes.data, c.value, 8 * c.nnz, stream))
        return c.m, c.n, rp, ci[:ncol], vv[: c.nnz] if vv is not None else None
