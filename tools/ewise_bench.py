#!/usr/bin/env python3
"""The element-wise pass (Context.ewise), measured on the two steps it was
built for, each against the same step done in torch.

  bfs      synth.rmat(scale_n=200_000), 64 sources: the BFS loop of DESIGN.md
           section 3.11 on the device, N = F*A<!Visited> by the masked symbolic
           pass, and at every depth the step Visited u= N timed two ways:
             ewise  Context.ewise(Visited, N) (structural union)
             torch  the row * n + column keys of both (Visited's built once,
                    outside the timed step; N's inside it, without a host
                    synchronisation) concatenated, sorted and made unique, the
                    row pointers and columns rebuilt (bincount + cumsum)
  webbase  synth.webbase(): the valued union A + A^T (A^T by Context.transpose)
             ewise  Context.ewise(A, At, "union", "plus")
             torch  (Sa + Sat).coalesce() on sparse COO tensors

Both ways take device CSR arrays (torch: COO for the sparse addition) and end
synchronised; the calls alternate in one process, --warmup pairs then --calls
pairs, a host clock around each; the median and the spread are reported.  The
two results must be equal before anything is timed.  Memory: the pool's
reserved bytes after one ewise call on a fresh context, against torch's peak
allocation over one call of its route.  Each ewise call's fraction of the HBM
roofline is B_alg / t / 8 TB/s with
  B_alg = 4 (nnzA + nnzB)                      the count: both operands' columns
        + w (nnzA + nnzB) + w nnzC             the fill (w = 4 structural, 12 valued)
        + 24 (m + 1)                           the row pointers, both passes
Writes profiles/ewise_rmat.json and profiles/ewise_webbase.json (--out-dir).
Fails when no GPU is found.

  python tools/ewise_bench.py [--calls 30] [--warmup 5] [--scale 200000] [--case bfs webbase] [--max-depth D]
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
HBM_PEAK = 8.0e12  # B/s, MI355X specification


def spread(x):
    x = np.asarray(x)
    return dict(median=float(np.median(x)), min=float(x.min()), max=float(x.max()),
                p10=float(np.percentile(x, 10)), p90=float(np.percentile(x, 90)))


def b_alg(nnz_a, nnz_b, nnz_c, m, valued):
    w = 12 if valued else 4
    return 4 * (nnz_a + nnz_b) + w * (nnz_a + nnz_b) + w * nnz_c + 24 * (m + 1)


def timed_pairs(torch, ctx, ewise_call, torch_call, warmup, calls):
    """alternating calls; (ewise ms, its kernels' ms, torch ms) per pair"""
    for _ in range(warmup):
        ewise_call(ctx)
        ctx.reset()
        torch_call()
    t_e, k_e, t_t = [], [], []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, st = ewise_call(ctx)
        t1 = time.perf_counter()
        ctx.reset()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        torch_call()
        t3 = time.perf_counter()
        t_e.append((t1 - t0) * 1e3)
        k_e.append(st["t_step3_kernel_ms"])
        t_t.append((t3 - t2) * 1e3)
    return t_e, k_e, t_t


def memory(torch, Context, ewise_call, torch_call):
    cx = Context(0)
    try:
        ewise_call(cx)
        pool = int(cx.pool_stats()["reserved_bytes"])
    finally:
        cx.close()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = torch_call()
    peak = int(torch.cuda.max_memory_allocated() - base)
    del out
    return dict(ewise_pool_reserved_bytes=pool, torch_peak_bytes=peak)


def step_record(name, info, m, valued, t_e, k_e, t_t, mem, equal):
    ba = b_alg(info["nnzA"], info["nnzB"], info["nnzC"], m, valued)
    med_e, med_t = float(np.median(t_e)), float(np.median(t_t))
    return dict(step=name, nnzA=int(info["nnzA"]), nnzB=int(info["nnzB"]), both=int(info["both"]),
                nnzC=int(info["nnzC"]), rows_class=info["rows_class"], units=int(info["units"]),
                results_equal=bool(equal), ewise_ms=spread(t_e), ewise_kernel_ms=spread(k_e), torch_ms=spread(t_t),
                ewise_over_torch=med_e / med_t, torch_over_ewise=med_t / med_e, b_alg_bytes=int(ba),
                hbm_fraction_by_b_alg=ba / (med_e * 1e-3) / HBM_PEAK,
                hbm_fraction_by_b_alg_kernels=ba / (float(np.median(k_e)) * 1e-3) / HBM_PEAK, memory=mem)


def bfs_case(torch, args):
    from spgemm_amd import synth
    from spgemm_amd.device import Context, DeviceCSR
    n, _, rp, ci, _ = synth.rmat(scale_n=args.scale)
    dA = DeviceCSR(n, n, torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), None)
    rng = np.random.default_rng(20260116)
    src = np.sort(rng.choice(np.flatnonzero(np.diff(rp) > 0), size=SOURCES, replace=False))
    frp = torch.arange(SOURCES + 1, dtype=torch.int32, device="cuda")
    F = visited = DeviceCSR(SOURCES, n, frp, torch.from_numpy(src.astype(np.int32)).cuda(), None)

    def keys_of(M):
        rows = torch.repeat_interleave(torch.arange(M.m, device="cuda"), torch.diff(M.rowptr).long(),
                                       output_size=M.nnz)  # (the size given: no host synchronisation)
        return rows * n + M.col.long()

    def torch_union(vkeys, N):
        k = torch.unique(torch.cat([vkeys, keys_of(N)]), sorted=True)
        nrp = torch.zeros(N.m + 1, dtype=torch.int32, device="cuda")
        nrp[1:] = torch.cumsum(torch.bincount(k // n, minlength=N.m), 0)
        col = (k % n).int()
        torch.cuda.synchronize()
        return nrp, col

    ctx = Context(0)
    steps, depth = [], 0
    while True:
        depth += 1
        c, _, _ = ctx.spgemm_symbolic(F, dA, "pattern", mask=visited, complement=True)
        F = ctx.to_torch(c)
        ctx.reset()
        if not F.nnz or depth > args.max_depth:
            break
        V, N = visited, F
        vkeys = keys_of(V)  # (a torch-side BFS keeps Visited as keys: built once, outside the timed step)
        ew = lambda cx: cx.ewise(V, N)
        tc = lambda: torch_union(vkeys, N)
        c, info, _ = ew(ctx)
        got = ctx.to_torch(c)
        ctx.reset()
        nrp, col = tc()
        equal = torch.equal(got.rowptr, nrp) and torch.equal(got.col, col)
        if not equal:  # (nothing is timed on unequal results)
            sys.exit(f"ewise_bench: depth {depth}: the ewise union differs from the torch route's")
        t_e, k_e, t_t = timed_pairs(torch, ctx, ew, tc, args.warmup, args.calls)
        steps.append(step_record(f"depth {depth}", info, SOURCES, False, t_e, k_e, t_t,
                                 memory(torch, Context, ew, tc), equal))
        print(json.dumps({k: steps[-1][k] for k in ("step", "nnzA", "nnzB", "nnzC", "results_equal",
                                                    "ewise_over_torch", "hbm_fraction_by_b_alg")} |
                         {"ewise_ms": steps[-1]["ewise_ms"]["median"], "torch_ms": steps[-1]["torch_ms"]["median"]}),
              flush=True)
        visited = got
    ctx.close()
    return dict(case="bfs", graph=f"synth.rmat(scale_n={args.scale})", n=n, nnzA=int(len(ci)), sources=SOURCES,
                steps=steps)


def webbase_case(torch, args):
    from spgemm_amd import synth
    from spgemm_amd.device import Context, DeviceCSR
    n, _, rp, ci, vv = synth.webbase()
    dA = DeviceCSR.from_host(n, n, rp, ci, vv)
    ctx = Context(0)
    dAt = ctx.to_torch(ctx.transpose(dA))
    ctx.reset()

    def coo(M):
        rows = torch.repeat_interleave(torch.arange(M.m, device="cuda"), torch.diff(M.rowptr).long())
        return torch.sparse_coo_tensor(torch.stack([rows, M.col.long()]), M.val, (M.m, M.n)).coalesce()

    Sa, Sat = coo(dA), coo(dAt)

    def torch_add():
        s = (Sa + Sat).coalesce()
        torch.cuda.synchronize()
        return s

    ew = lambda cx: cx.ewise(dA, dAt, "union", "plus")
    c, info, _ = ew(ctx)
    got = ctx.to_torch(c)
    ctx.reset()
    s = torch_add()
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), torch.diff(got.rowptr).long())
    idx = s.indices()
    equal = (idx.shape[1] == got.nnz and torch.equal(idx[0], rows) and torch.equal(idx[1], got.col.long())
             and torch.equal(s.values(), got.val))
    del s
    if not equal:  # (nothing is timed on unequal results)
        sys.exit("ewise_bench: webbase: the ewise sum differs from torch.sparse's")
    t_e, k_e, t_t = timed_pairs(torch, ctx, ew, torch_add, args.warmup, args.calls)
    ctx.close()
    step = step_record("A + A^T", info, n, True, t_e, k_e, t_t, memory(torch, Context, ew, torch_add), equal)
    print(json.dumps({k: step[k] for k in ("step", "nnzA", "nnzB", "nnzC", "results_equal", "ewise_over_torch",
                                           "hbm_fraction_by_b_alg")} |
                     {"ewise_ms": step["ewise_ms"]["median"], "torch_ms": step["torch_ms"]["median"]}), flush=True)
    return dict(case="webbase", graph="synth.webbase()", n=n, nnzA=int(len(ci)), steps=[step])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=int, default=200_000)
    ap.add_argument("--case", nargs="+", default=["bfs", "webbase"], choices=["bfs", "webbase"])
    ap.add_argument("--max-depth", type=int, default=1 << 30, help="bfs: stop after this depth (a profiler's run)")
    ap.add_argument("--out-dir", default=os.path.join(REPO, "profiles"))
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: at least 20")
    import torch
    if not torch.cuda.is_available() or torch.cuda.device_count() < 1:
        sys.exit("ewise_bench: no GPU found")
    os.makedirs(args.out_dir, exist_ok=True)
    for case in args.case:
        res = bfs_case(torch, args) if case == "bfs" else webbase_case(torch, args)
        res.update(calls=args.calls, warmup=args.warmup, hbm_peak_bytes_per_s=HBM_PEAK,
                   timing="host clock around calls that end synchronised; ewise and torch calls alternate in one "
                          "process; memory after one call of each kind (ewise on a fresh context)")
        name = "ewise_rmat.json" if case == "bfs" else "ewise_webbase.json"
        with open(os.path.join(args.out_dir, name), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
