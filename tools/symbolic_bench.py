#!/usr/bin/env python3
"""The symbolic pass, measured: the full product (Context.spgemm, the baseline)
against Context.spgemm_symbolic on the same operands, same process, calls
alternating.

For each config (synthetic webbase A*A, cant A*A, mc2depi A*A^T, as bench.py
runs them): both calls are warmed in pairs, then --calls pairs of (spgemm,
spgemm_symbolic) are timed with a host clock around calls that return
synchronised; TSG_SYMBOLIC_COUNT alone is timed the same way.  The pool's
reserved bytes after one call of each kind are taken on fresh contexts.  The
plan's whole creation from the operands (Context.spgemm_plan: symbolic, copy,
numeric_plan) is timed against the detour it replaces (full product, copy,
numeric_plan).  The symbolic pattern is compared with the full product's,
element for element.  Writes profiles/symbolic_<config>.json.  Fails when no
GPU is found.

  python tools/symbolic_bench.py [--configs webbase cant mc2depi] [--calls 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12  # B/s, MI355X specification


def spread(x):
    x = np.asarray(x)
    return dict(median=float(np.median(x)), min=float(x.min()), max=float(x.max()),
                p10=float(np.percentile(x, 10)), p90=float(np.percentile(x, 90)))


def reserved_after(call):
    """the pool's reserved bytes after one call on a fresh context"""
    from spgemm_amd.device import Context
    ctx = Context(0)
    try:
        call(ctx)
        return int(ctx.pool_stats()["reserved_bytes"])
    finally:
        ctx.close()


def run_config(name, calls, warmup):
    import torch
    from spgemm_amd import synth
    from spgemm_amd.device import Context, DeviceCSR
    m, n, rp, ci, _ = synth.GENERATORS[name]()
    rng = np.random.default_rng(20260116)
    ctx = Context(0)
    dA = DeviceCSR.from_host(m, n, rp, ci, rng.uniform(-1, 1, len(ci)))
    if name == "mc2depi":  # A * A^T
        dB = ctx.to_torch(ctx.transpose(dA))
        ctx.reset()
    else:
        dB = DeviceCSR.from_host(m, n, rp, ci, rng.uniform(-1, 1, len(ci)))
    # the operands of the symbolic calls carry no values
    pA = DeviceCSR(dA.m, dA.n, dA.rowptr, dA.col, None)
    pB = DeviceCSR(dB.m, dB.n, dB.rowptr, dB.col, None)
    # parity: the symbolic pattern is the full product's
    c, st_full = ctx.spgemm(dA, dB)
    full = ctx.to_torch(c)
    ctx.reset()
    c, info, _ = ctx.spgemm_symbolic(pA, pB)
    sym = ctx.to_torch(c)
    ctx.reset()
    same = bool(torch.equal(full.rowptr, sym.rowptr) and torch.equal(full.col, sym.col))
    nnzC = full.nnz
    del full, sym
    for _ in range(warmup):
        ctx.spgemm(dA, dB, raw=True)
        ctx.reset()
        ctx.spgemm_symbolic(pA, pB)
        ctx.reset()
        ctx.spgemm_symbolic(pA, pB, "count")
        ctx.reset()
    t_full, t_sym, t_cnt, k_full, k_sym = [], [], [], [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        _, s1 = ctx.spgemm(dA, dB, raw=True)
        t1 = time.perf_counter()
        ctx.reset()
        t2 = time.perf_counter()
        _, _, s2 = ctx.spgemm_symbolic(pA, pB)
        t3 = time.perf_counter()
        ctx.reset()
        t4 = time.perf_counter()
        ctx.spgemm_symbolic(pA, pB, "count")
        t5 = time.perf_counter()
        ctx.reset()
        t_full.append((t1 - t0) * 1e3)
        t_sym.append((t3 - t2) * 1e3)
        t_cnt.append((t5 - t4) * 1e3)
        k_full.append(s1.t_step3_kernel_ms)
        k_sym.append(s2["t_step3_kernel_ms"])
    # the plan from the operands against the detour it replaces
    t_plan, t_detour = [], []
    for i in range(2 + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = ctx.spgemm_plan(pA, pB)
        t1 = time.perf_counter()
        plan.close()
        ctx.reset()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        c, _ = ctx.spgemm(dA, dB)
        dC = ctx.to_torch(c)
        ctx.reset()
        plan = ctx.numeric_plan(dA, dB, dC)
        t3 = time.perf_counter()
        plan.close()
        del dC
        if i >= 2:  # (two warm-up pairs)
            t_plan.append((t1 - t0) * 1e3)
            t_detour.append((t3 - t2) * 1e3)
    ctx.close()
    reserved = dict(
        full=reserved_after(lambda cx: cx.spgemm(dA, dB)),
        symbolic=reserved_after(lambda cx: cx.spgemm_symbolic(pA, pB)),
        count=reserved_after(lambda cx: cx.spgemm_symbolic(pA, pB, "count")))
    nnzA, nnzB, P = dA.nnz, dB.nnz, info["products"]
    # what one phase of the pass must move: a 4 B column per A entry (and its
    # 8 B entry bounds), a 4 B column per product, the row pointers; the fill
    # also a 4 B column per C entry.  Count and fill each walk the products.
    one_phase = 4 * nnzA + 4 * P + 4 * (dA.m + dB.m + dA.m + 3)
    by_products = 2 * one_phase + 4 * nnzC
    med_sym = float(np.median(t_sym))
    return dict(
        config=name + "-synthetic", product="A*A^T" if name == "mc2depi" else "A*A",
        m=dA.m, n=dB.n, nnzA=nnzA, nnzB=nnzB, nnzC=nnzC, calls=calls, warmup=warmup,
        full_path=int(st_full["path"]), pattern_equals_full=same,
        full_ms=spread(t_full), symbolic_ms=spread(t_sym), count_ms=spread(t_cnt),
        full_kernel_ms=spread(k_full), symbolic_kernel_ms=spread(k_sym),
        speedup_median=float(np.median(t_full)) / med_sym,
        reserved_bytes=reserved, info=info,
        plan_from_operands_ms=spread(t_plan), plan_by_full_product_ms=spread(t_detour),
        bytes_by_products=by_products,
        hbm_fraction_by_products=by_products / (med_sym * 1e-3) / HBM_PEAK,
        hbm_peak_bytes_per_s=HBM_PEAK,
        timing="host clock around calls that return synchronised; full, symbolic and count calls alternate in "
               "one process; reserved bytes after one call on a fresh context each",
    )


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["webbase", "cant", "mc2depi"])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--outdir", default=os.path.join(REPO, "profiles"))
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: at least 20")
    import torch
    if not torch.cuda.is_available() or torch.cuda.device_count() < 1:
        sys.exit("symbolic_bench: no GPU found")
    os.makedirs(args.outdir, exist_ok=True)
    for name in args.configs:
        res = run_config(name, args.calls, args.warmup)
        path = os.path.join(args.outdir, f"symbolic_{name}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({k: res[k] for k in ("config", "speedup_median", "pattern_equals_full", "reserved_bytes")} |
                         {"full_ms": res["full_ms"]["median"], "symbolic_ms": res["symbolic_ms"]["median"],
                          "count_ms": res["count_ms"]["median"],
                          "plan_from_operands_ms": res["plan_from_operands_ms"]["median"],
                          "plan_by_full_product_ms": res["plan_by_full_product_ms"]["median"]}), flush=True)
        if not res["pattern_equals_full"]:
            sys.exit(f"symbolic_bench: {name}: the symbolic pattern differs from the full product's")


if __name__ == "__main__":
    main()
