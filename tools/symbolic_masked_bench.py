#!/usr/bin/env python3
"""The masked symbolic pass, measured on the step it was built for: one
multi-source BFS expansion N = F*A<!Visited>.

The graph is synth.rmat(scale_n=200_000); 64 sources; the frontier F (64 x n:
row s holds source s's vertices at depth d) and Visited (all its vertices up
to depth d) are taken from a host BFS at depths 1, 2 and 3.  Timed, per depth,
in one process with the two ways alternating:

  masked      Context.spgemm_symbolic(F, A, mask=Visited, complement=True)
  difference  what a caller does without the masked pass: Context.spgemm_symbolic(F, A),
              then a set difference on the device in torch (row * n + column keys,
              torch.isin against Visited's, the kept columns compacted, the row
              counts scanned)

--warmup pairs, then --calls pairs; a host clock around calls that end
synchronised (the masked call returns synchronised; the difference ends in
torch.cuda.synchronize()).  The two results are compared element for element.
The pool's reserved bytes after one call of each kind are taken on fresh
contexts; the difference's torch temporaries are reported beside them as
torch's peak allocation over one call.  Writes profiles/symbolic_masked_rmat.json.
Fails when no GPU is found.

  python tools/symbolic_masked_bench.py [--calls 30] [--warmup 5] [--scale 200000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SOURCES = 64


def spread(x):
    x = np.asarray(x)
    return dict(median=float(np.median(x)), min=float(x.min()), max=float(x.max()),
                p10=float(np.percentile(x, 10)), p90=float(np.percentile(x, 90)))


def frontiers(n, rp, ci, depths, seed):
    """per depth d: (F, Visited) as host CSR patterns of 64 x n, from a BFS by scipy
    (64-bit counts: scipy drops a sum that comes out 0, and a narrow type wraps to it)"""
    import scipy.sparse as sp
    A = sp.csr_matrix((np.ones(len(ci), dtype=np.int64), ci, rp), shape=(n, n))
    rng = np.random.default_rng(seed)
    src = rng.choice(np.flatnonzero(np.diff(rp) > 0), size=SOURCES, replace=False)
    F = sp.csr_matrix((np.ones(SOURCES, dtype=np.int64), (np.arange(SOURCES), src)), shape=(SOURCES, n))
    V = F.copy()
    out = {}
    for d in range(1, max(depths) + 1):
        nxt = (F @ A).tocsr()
        nxt.data[:] = 1
        nxt = (nxt - nxt.multiply(V)).tocsr()
        nxt.eliminate_zeros()
        F = nxt
        V = (V + F).tocsr()
        V.data[:] = 1
        for M in (F, V):
            M.sort_indices()
        if d in depths:
            out[d] = ((SOURCES, n, F.indptr.astype(np.int32), F.indices.astype(np.int32)),
                      (SOURCES, n, V.indptr.astype(np.int32), V.indices.astype(np.int32)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=int, default=200_000)
    ap.add_argument("--depths", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "symbolic_masked_rmat.json"))
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: at least 20")
    import torch
    if not torch.cuda.is_available() or torch.cuda.device_count() < 1:
        sys.exit("symbolic_masked_bench: no GPU found")
    from spgemm_amd import synth
    from spgemm_amd.device import Context, DeviceCSR

    n, _, rp, ci, _ = synth.rmat(scale_n=args.scale)
    dev = lambda M: DeviceCSR(M[0], M[1], torch.from_numpy(M[2]).cuda(), torch.from_numpy(M[3]).cuda(), None)
    dA = dev((n, n, rp, ci))
    cases = frontiers(n, rp, ci, args.depths, 20260116)

    def masked(cx, dF, dV):
        c, info, st = cx.spgemm_symbolic(dF, dA, mask=dV, complement=True)
        return c, info, st

    def difference(cx, dF, dV, vkeys):
        """the unmasked pattern, then C minus Visited on the device: (rowptr, col)"""
        c, info, _ = cx.spgemm_symbolic(dF, dA)
        C_ = cx.view_torch(c)
        rows = torch.repeat_interleave(torch.arange(C_.m, device="cuda"), torch.diff(C_.rowptr).long())
        keep = torch.isin(rows * n + C_.col.long(), vkeys, assume_unique=True, invert=True)
        col = C_.col[keep]
        cnt = torch.bincount(rows[keep], minlength=C_.m)
        nrp = torch.zeros(C_.m + 1, dtype=torch.int32, device="cuda")
        nrp[1:] = torch.cumsum(cnt, 0)
        torch.cuda.synchronize()
        return nrp, col, info

    results = []
    for d in args.depths:
        F, V = cases[d]
        dF, dV = dev(F), dev(V)
        vrows = torch.repeat_interleave(torch.arange(SOURCES, device="cuda"), torch.diff(dV.rowptr).long())
        vkeys = vrows * n + dV.col.long()  # (the caller's Visited as keys: built once, outside the timed step)
        ctx = Context(0)
        c, info, _ = masked(ctx, dF, dV)
        got = ctx.to_torch(c)
        ctx.reset()
        nrp, col, uinfo = difference(ctx, dF, dV, vkeys)
        ctx.reset()
        same = bool(torch.equal(got.rowptr, nrp) and torch.equal(got.col, col))
        for _ in range(args.warmup):
            masked(ctx, dF, dV)
            ctx.reset()
            difference(ctx, dF, dV, vkeys)
            ctx.reset()
        t_m, t_d, k_m = [], [], []
        for _ in range(args.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, st = masked(ctx, dF, dV)
            t1 = time.perf_counter()
            ctx.reset()
            t2 = time.perf_counter()
            difference(ctx, dF, dV, vkeys)
            t3 = time.perf_counter()
            ctx.reset()
            t_m.append((t1 - t0) * 1e3)
            t_d.append((t3 - t2) * 1e3)
            k_m.append(st["t_step3_kernel_ms"])
        ctx.close()
        reserved = {}
        for name, call in (("masked", lambda cx: masked(cx, dF, dV)),
                           ("difference", lambda cx: difference(cx, dF, dV, vkeys))):
            cx = Context(0)
            try:
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                call(cx)
                reserved[name] = dict(pool_reserved_bytes=int(cx.pool_stats()["reserved_bytes"]),
                                      torch_peak_bytes=int(torch.cuda.max_memory_allocated() - base))
            finally:
                cx.close()
        res = dict(depth=d, nnzF=int(len(F[3])), nnzVisited=int(len(V[3])), products=int(info["products"]),
                   nnz_unmasked=int(uinfo["nnzC"]), nnz_masked=int(info["nnzC"]), rows_class=info["rows_class"],
                   results_equal=same, masked_ms=spread(t_m), difference_ms=spread(t_d),
                   masked_kernel_ms=spread(k_m),
                   masked_over_difference=float(np.median(t_m)) / float(np.median(t_d)),
                   difference_over_masked=float(np.median(t_d)) / float(np.median(t_m)), memory=reserved)
        results.append(res)
        print(json.dumps({k: res[k] for k in ("depth", "nnzF", "nnzVisited", "products", "nnz_unmasked",
                                              "nnz_masked", "results_equal", "masked_over_difference")} |
                         {"masked_ms": res["masked_ms"]["median"], "difference_ms": res["difference_ms"]["median"]}),
              flush=True)
    out = dict(graph=f"synth.rmat(scale_n={args.scale})", n=n, nnzA=int(len(ci)), sources=SOURCES, calls=args.calls,
               warmup=args.warmup, steps=results,
               timing="host clock around calls that end synchronised; masked and difference calls alternate in one "
                      "process; memory after one call of each kind on a fresh context")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not all(r["results_equal"] for r in results):
        sys.exit("symbolic_masked_bench: the masked pattern differs from the set difference's")


if __name__ == "__main__":
    main()
