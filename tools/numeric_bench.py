#!/usr/bin/env python3
"""Pattern reuse, measured: the full product (Context.spgemm) against the
numeric-only run on its known pattern (NumericPlan.run), same operands, same
process, calls alternating.

For each config (synthetic webbase, cant, mc2depi; mc2depi as A*A^T, as bench.py
runs it): the pattern comes from a full spgemm, the plan is created (timed),
both paths are warmed, then --calls pairs of (spgemm, plan.run) are timed with
a host clock around calls that return synchronised.  Writes
profiles/numeric_reuse_<config>.json: medians, spreads, plan-creation time, the
plan's info counts, the bytes the numeric pass must move and the resulting
whole-call HBM fraction, and the values' maximum scaled error against the full
product's values on the same inputs.  Fails when no GPU is found.

  python tools/numeric_bench.py [--configs webbase cant mc2depi] [--calls 30]
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
    # the pattern, and the full product's values on these inputs
    c, st_full = ctx.spgemm(dA, dB)
    dC = ctx.to_torch(c)
    ctx.reset()
    t_plan = []
    plan = None
    for _ in range(3):
        if plan is not None:
            plan.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = ctx.numeric_plan(dA, dB, dC)
        t_plan.append((time.perf_counter() - t0) * 1e3)
    out = torch.empty(dC.nnz, dtype=torch.float64, device="cuda")
    # scaled error: |numeric - full| / (|A| * |B|), the magnitudes from a full product of the absolute values
    plan.run(dA.val, dB.val, out=out)
    dAa = DeviceCSR(dA.m, dA.n, dA.rowptr, dA.col, dA.val.abs())
    dBa = DeviceCSR(dB.m, dB.n, dB.rowptr, dB.col, dB.val.abs())
    cm, _ = ctx.spgemm(dAa, dBa)
    mag = ctx.to_torch(cm).val
    ctx.reset()
    err = (out - dC.val).abs()
    scaled = float((err / mag.clamp_min(1e-300)).max())
    for _ in range(warmup):
        ctx.spgemm(dA, dB, raw=True)
        ctx.reset()
        plan.run(dA.val, dB.val, out=out, raw=True)
    t_full, t_num, k_full, k_num = [], [], [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        _, s1 = ctx.spgemm(dA, dB, raw=True)
        t1 = time.perf_counter()
        ctx.reset()
        t2 = time.perf_counter()
        _, s2 = plan.run(dA.val, dB.val, out=out, raw=True)
        t3 = time.perf_counter()
        t_full.append((t1 - t0) * 1e3)
        t_num.append((t3 - t2) * 1e3)
        k_full.append(s1.t_step3_kernel_ms)
        k_num.append(s2.t_step3_kernel_ms)
    info = plan.info
    nnzA, nnzB, nnzC, P = dA.nnz, dB.nnz, dC.nnz, info["products"]
    # what the numeric pass must move: A's pattern and values once, a B entry
    # (column + value) per product, C's columns read, C's values written, the
    # three row-pointer arrays.  (B's rows are re-read per referencing A entry;
    # the caches take part of that, so this is the upper bound of the model,
    # and `compulsory` -- every array once -- the lower.)
    by_products = 12 * nnzA + 12 * P + 4 * nnzC + 8 * nnzC + 4 * (2 * dA.m + dB.m + 3)
    compulsory = 12 * nnzA + 12 * nnzB + 12 * nnzC + 4 * (2 * dA.m + dB.m + 3)
    med_num = float(np.median(t_num))
    res = dict(
        config=name + "-synthetic", product="A*A^T" if name == "mc2depi" else "A*A",
        m=dA.m, n=dB.n, nnzA=nnzA, nnzB=nnzB, calls=calls, warmup=warmup,
        full_path=int(st_full["path"]),
        full_ms=spread(t_full), numeric_ms=spread(t_num),
        full_kernel_ms=spread(k_full), numeric_kernel_ms=spread(k_num),
        speedup_median=float(np.median(t_full)) / med_num,
        plan_create_ms=spread(t_plan), info=info,
        bytes_by_products=by_products, bytes_compulsory=compulsory,
        hbm_fraction_by_products=by_products / (med_num * 1e-3) / HBM_PEAK,
        hbm_fraction_compulsory=compulsory / (med_num * 1e-3) / HBM_PEAK,
        hbm_peak_bytes_per_s=HBM_PEAK,
        max_scaled_error_vs_full=scaled,
        timing="host clock around calls that return synchronised; full and numeric calls alternate in one process",
    )
    plan.close()
    ctx.close()
    return res


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
        sys.exit("numeric_bench: no GPU found")
    os.makedirs(args.outdir, exist_ok=True)
    for name in args.configs:
        res = run_config(name, args.calls, args.warmup)
        path = os.path.join(args.outdir, f"numeric_reuse_{name}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({k: res[k] for k in ("config", "speedup_median", "max_scaled_error_vs_full")} |
                         {"full_ms": res["full_ms"]["median"], "numeric_ms": res["numeric_ms"]["median"],
                          "plan_create_ms": res["plan_create_ms"]["median"]}), flush=True)
        if not res["max_scaled_error_vs_full"] <= 1e-10:
            sys.exit(f"numeric_bench: {name}: scaled error {res['max_scaled_error_vs_full']} past 1e-10")


if __name__ == "__main__":
    main()
