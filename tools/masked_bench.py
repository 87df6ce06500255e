#!/usr/bin/env python3
"""Masked SpGEMM, measured: C<M> = A*A on the mask's pattern only
(MaskedPlan.run) in its three modes -- every row row-wise, every row on the dot
leg, the per-row choice -- on the graph operands of the project's generators:

  rmat     synth.rmat(scale_n=--rmat-rows), mask = A
  rmat_l   its strict lower triangle L, L*L<L> (triangle counting)
  webbase  synth.webbase(n=--webbase-rows), mask = A

One process; per mode the plan is created three times (timed), warmed, then
--calls runs are timed with a host clock around calls that return
synchronised.  Writes profiles/masked_<config>[_<tag>].json: medians and
(min-max) per mode, plan-creation time, the plan's info counts, the bytes a run
must move, and the legs' largest difference scaled by |A| * |B|.  Fails when no
GPU is found.

  python tools/masked_bench.py [--configs rmat rmat_l webbase] [--modes rows dot auto] [--calls 30]
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
    return dict(median=float(np.median(x)), min=float(x.min()), max=float(x.max()))


def operand(name, args):
    from spgemm_amd import synth
    if name == "webbase":
        m, n, rp, ci, _ = synth.webbase(n=args.webbase_rows)
        return m, n, rp, ci
    m, n, rp, ci, _ = synth.rmat(scale_n=args.rmat_rows)
    if name == "rmat_l":  # strict lower triangle (the generator removed duplicates)
        rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
        keep = ci < rows
        rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=m))]).astype(np.int32)
        ci = ci[keep]
    return m, n, rp, ci


def run_config(name, args):
    import torch
    from spgemm_amd.device import Context, DeviceCSR
    m, n, rp, ci = operand(name, args)
    rng = np.random.default_rng(20260116)
    ctx = Context(0)
    dA = DeviceCSR.from_host(m, n, rp, ci, rng.uniform(-1, 1, len(ci)))
    b_val = torch.from_numpy(rng.uniform(-1, 1, len(ci))).cuda()
    out = torch.empty(dA.nnz, dtype=torch.float64, device="cuda")
    modes, outs = {}, {}
    for mode in args.modes:
        t_plan, plan = [], None
        for _ in range(3):
            if plan is not None:
                plan.close()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plan = ctx.masked_plan(dA, dA, dA, mode=mode)
            t_plan.append((time.perf_counter() - t0) * 1e3)
        for _ in range(args.warmup):
            plan.run(dA.val, b_val, out=out, raw=True)
        t_run, t_kern = [], []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            _, st = plan.run(dA.val, b_val, out=out, raw=True)
            t_run.append((time.perf_counter() - t0) * 1e3)
            t_kern.append(st.t_step3_kernel_ms)
        info = plan.info
        outs[mode] = out.clone()
        nnz = dA.nnz
        # what a run must move.  Every array once (the lower bound): A's pattern
        # and values, the mask's columns read and its values written, the row
        # pointers; where the dot leg has rows also B^T's gather (position and
        # value read, value written) and B^T's columns and values read.  By work
        # (the upper bound, the caches take part of it): a B entry (column +
        # value) per row-wise product, a column + value of the shorter list per
        # dot step; the searches' reads of the longer list come on top of both.
        dot = info["rows_dot"] > 0
        compulsory = 12 * nnz + 12 * nnz + 4 * 3 * (m + 1) + (12 * nnz if info["rows_rowwise"] else 0) + \
            ((20 + 12) * nnz + 4 * (n + 1) if dot else 0)
        by_work = compulsory + 12 * info["products_rowwise"] + 12 * info["dot_work"]
        med = float(np.median(t_run))
        modes[mode] = dict(run_ms=spread(t_run), kernel_ms=spread(t_kern), plan_create_ms=spread(t_plan), info=info,
                           bytes_compulsory=compulsory, bytes_by_work=by_work,
                           hbm_fraction_compulsory=compulsory / (med * 1e-3) / HBM_PEAK,
                           hbm_fraction_by_work=by_work / (med * 1e-3) / HBM_PEAK)
        plan.close()
        print(f"masked_bench: {name} {mode}: {med:.3f} ms", file=sys.stderr, flush=True)
    res = dict(config=name, product="A*A<A>", m=m, n=n, nnzA=int(dA.nnz), calls=args.calls, warmup=args.warmup,
               rmat_rows=args.rmat_rows if name != "webbase" else None,
               webbase_rows=args.webbase_rows if name == "webbase" else None, modes=modes,
               hbm_peak_bytes_per_s=HBM_PEAK,
               timing="host clock around calls that return synchronised; one process")
    if "rows" in outs and "dot" in outs:
        # |A| * |B| at the mask's entries: a masked run of the absolute values
        plan = ctx.masked_plan(dA, dA, dA, mode="rows")
        mag, _ = plan.run(dA.val.abs(), b_val.abs())
        plan.close()
        res["max_scaled_diff_rows_vs_dot"] = float(((outs["rows"] - outs["dot"]).abs() / mag.clamp_min(1e-300)).max())
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["rmat", "rmat_l", "webbase"],
                    choices=["rmat", "rmat_l", "webbase"])
    ap.add_argument("--modes", nargs="+", default=["rows", "dot", "auto"], choices=["rows", "dot", "auto"])
    ap.add_argument("--rmat-rows", type=int, default=200_000)
    ap.add_argument("--webbase-rows", type=int, default=1_000_005)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="", help="suffix of the output files (a build variant's name)")
    ap.add_argument("--outdir", default=os.path.join(REPO, "profiles"))
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: at least 20")
    import torch
    if not torch.cuda.is_available() or torch.cuda.device_count() < 1:
        sys.exit("masked_bench: no GPU found")
    os.makedirs(args.outdir, exist_ok=True)
    for name in args.configs:
        res = run_config(name, args)
        path = os.path.join(args.outdir, f"masked_{name}{'_' + args.tag if args.tag else ''}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        line = {"config": name, "tag": args.tag}
        for mode, r in res["modes"].items():
            line[mode + "_ms"] = "%.3f (%.3f-%.3f)" % (r["run_ms"]["median"], r["run_ms"]["min"], r["run_ms"]["max"])
            line[mode + "_plan_ms"] = round(r["plan_create_ms"]["median"], 2)
        if "max_scaled_diff_rows_vs_dot" in res:
            line["max_scaled_diff_rows_vs_dot"] = res["max_scaled_diff_rows_vs_dot"]
        print(json.dumps(line), flush=True)
        if res.get("max_scaled_diff_rows_vs_dot", 0.0) > 2e-10:
            sys.exit(f"masked_bench: {name}: the legs differ by {res['max_scaled_diff_rows_vs_dot']} (scaled)")


if __name__ == "__main__":
    main()
