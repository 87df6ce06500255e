#!/usr/bin/env python3
"""Semiring runs, measured against the arithmetic run on the same plan.

  webbase, cant, mc2depi   one numeric plan each (Context.spgemm_plan: the symbolic
                           pass's pattern; mc2depi as A*A^T, as bench.py runs it)
  rmat                     one masked plan on synth.rmat(scale_n=--rmat-rows) with
                           its own pattern as mask, auto mode

One process per invocation, one plan per config.  For every semiring but
plus_times, --calls pairs of (plus_times run, semiring run) alternate on the
plan, timed with a host clock around calls that return synchronised, after
--warmup pairs.  Values: uniform(0.5, 2) on both operands (finite in every
semiring); plus_pair runs with no values at all.  Writes
profiles/semiring_<config>[_<tag>].json: per semiring the two medians with
(min-max), the kernels' medians from the stats, the ratio of the medians, and
whether two runs of the semiring gave the same bits.  Fails when no GPU is
found.

  python tools/semiring_bench.py [--configs webbase cant mc2depi rmat] [--calls 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def spread(x):
    x = np.asarray(x)
    return dict(median=float(np.median(x)), min=float(x.min()), max=float(x.max()))


def make_plan(name, args):
    """(context, plan, a values, b values, what the plan is)"""
    import torch
    from spgemm_amd import synth
    from spgemm_amd.device import Context, DeviceCSR
    rng = np.random.default_rng(20260116)
    ctx = Context(0)
    if name == "rmat":
        m, n, rp, ci, _ = synth.rmat(scale_n=args.rmat_rows)
        dA = DeviceCSR.from_host(m, n, rp, ci, rng.uniform(0.5, 2, len(ci)))
        b_val = torch.from_numpy(rng.uniform(0.5, 2, len(ci))).cuda()
        plan = ctx.masked_plan(dA, dA, dA, mode="auto")
        return ctx, plan, dA.val, b_val, dict(plan="masked, auto, mask = A", product="A*A<A>", m=m, n=n,
                                              nnzA=dA.nnz, nnzB=dA.nnz, nnz_out=dA.nnz, rmat_rows=args.rmat_rows)
    m, n, rp, ci, _ = synth.GENERATORS[name]()
    dA = DeviceCSR.from_host(m, n, rp, ci, rng.uniform(0.5, 2, len(ci)))
    if name == "mc2depi":  # A * A^T
        dB = ctx.to_torch(ctx.transpose(dA))
        ctx.reset()
    else:
        dB = DeviceCSR.from_host(m, n, rp, ci, rng.uniform(0.5, 2, len(ci)))
    plan = ctx.spgemm_plan(dA, dB)
    ctx.reset()
    return ctx, plan, dA.val, dB.val, dict(plan="numeric, pattern from the symbolic pass",
                                           product="A*A^T" if name == "mc2depi" else "A*A", m=dA.m, n=dB.n,
                                           nnzA=dA.nnz, nnzB=dB.nnz, nnz_out=plan.nnzC)


def run_config(name, args):
    import torch
    from spgemm_amd.tilespgemm import SEMIRINGS
    ctx, plan, a_val, b_val, what = make_plan(name, args)
    out = torch.empty(what["nnz_out"], dtype=torch.float64, device="cuda")
    res = {}
    for sr in SEMIRINGS:
        if sr == "plus_times":
            continue
        va, vb = (None, None) if sr == "plus_pair" else (a_val, b_val)
        first, _ = plan.run(va, vb, semiring=sr)
        again, _ = plan.run(va, vb, semiring=sr)
        same_bits = bool(torch.equal(first.view(torch.int64), again.view(torch.int64)))
        for _ in range(args.warmup):
            plan.run(a_val, b_val, out=out, raw=True)
            plan.run(va, vb, out=out, raw=True, semiring=sr)
        t_base, t_sr, k_base, k_sr = [], [], [], []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            _, s0 = plan.run(a_val, b_val, out=out, raw=True)
            t1 = time.perf_counter()
            _, s1 = plan.run(va, vb, out=out, raw=True, semiring=sr)
            t2 = time.perf_counter()
            t_base.append((t1 - t0) * 1e3)
            t_sr.append((t2 - t1) * 1e3)
            k_base.append(s0.t_step3_kernel_ms)
            k_sr.append(s1.t_step3_kernel_ms)
        res[sr] = dict(plus_times_ms=spread(t_base), semiring_ms=spread(t_sr), plus_times_kernel_ms=spread(k_base),
                       semiring_kernel_ms=spread(k_sr),
                       ratio_median=float(np.median(t_sr)) / float(np.median(t_base)), same_bits_twice=same_bits)
    info = plan.info
    plan.close()
    ctx.close()
    return dict(config=name + ("" if name == "rmat" else "-synthetic"), **what, calls=args.calls, warmup=args.warmup,
                info=info, semirings=res,
                timing="host clock around calls that return synchronised; plus_times and the semiring alternate "
                       "on one plan in one process")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["webbase", "cant", "mc2depi", "rmat"],
                    choices=["webbase", "cant", "mc2depi", "rmat"])
    ap.add_argument("--rmat-rows", type=int, default=200_000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="", help="suffix of the output files (a build variant's name)")
    ap.add_argument("--outdir", default=os.path.join(REPO, "profiles"))
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: at least 20")
    import torch
    if not torch.cuda.is_available() or torch.cuda.device_count() < 1:
        sys.exit("semiring_bench: no GPU found")
    os.makedirs(args.outdir, exist_ok=True)
    for name in args.configs:
        res = run_config(name, args)
        path = os.path.join(args.outdir, f"semiring_{name}{'_' + args.tag if args.tag else ''}.json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        line = {"config": name}
        for sr, r in res["semirings"].items():
            line[sr] = "%.3f vs %.3f ms (x%.2f)" % (r["semiring_ms"]["median"], r["plus_times_ms"]["median"],
                                                     r["ratio_median"])
        print(json.dumps(line), flush=True)
        unstable = [sr for sr, r in res["semirings"].items() if not r["same_bits_twice"]]
        if unstable:
            sys.exit(f"semiring_bench: {name}: two runs differ in their bits: {unstable}")


if __name__ == "__main__":
    main()
