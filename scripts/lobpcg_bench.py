"""The LOBPCG eigensolver (sprs_lobpcg_*) on one GPU: gen.poisson3d(128, 126, 124) — unequal sides, so the spectrum is simple —
f64, k = 4, block 8, the smallest end, tol 1e-8, the default start block, with no preconditioner, Jacobi, FSAI(1) and AMG, beside
`Eigsh` "smallest" with ncv = 32 on the same handle.  Per row: status, iterations (cycles for Eigsh), products, fallbacks, nconv,
wall ms (one warm-up solve of two iterations first, a context synchronise before every clock read), ms per iteration, the true
residual of the leading pair formed on the host.  No speed threshold is set.  One JSON line to stdout and to --out PATH (default
profiles/lobpcg_bench.json).

    python scripts/lobpcg_bench.py [--cap N] [--only none|jacobi|fsai|amg|eigsh] [--out PATH]

The rates of the Gram kernel and of the rotation are taken from a separate run under the profiler (counters and timing never
share a run), capped so that every launch of it does its work (a solve that ends by its cap enqueues no blind launches):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/lobpcg_bench.py --only none --cap 12 --out DIR/run.json
    python scripts/lobpcg_bench.py --stats DIR/.../*_kernel_stats.csv --run DIR/run.json

which prints, for LobGram, LzRotate and LobResid, calls, mean microseconds, the bytes each must move and bytes / time.  With b the
block: LobGram reads 2 b vectors at the start, 4 b in the first iteration and 6 b in every later one; LzRotate (two launches a
step) reads b and writes b at the start, then reads 3 b and writes 2 b; LobResid reads 2 b and writes b."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = (128, 126, 124)
K, BLOCK, NCV, TOL = 4, 8, 32, 1e-8
KINDS = ("none", "jacobi", "fsai", "amg")


def run(args):
    import numpy as np
    import scipy.sparse as sp

    import sprsolve_amd as sa
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    ip, ix, d = gen.poisson3d(*GRID)[:3]
    n = ip.size - 1
    M = sp.csr_matrix((d, ix, ip), shape=(n, n))
    A = sa.HipCsr.new((n, n), ip, ix, d)
    S = sa.Lobpcg.new(A, n, BLOCK)
    rec = dict(grid=list(GRID), n=int(n), nnz=int(ip[-1]), dtype="float64", k=K, block=BLOCK, ncv=NCV, tol=TOL, cap=args.cap, warmup_iters=min(2, args.cap),
               spmv_kernel=A.spmv_route()["kernel"], stream_format=A.stream_format(), rows={})

    def timed(label, solve, warm):
        try:
            warm()
        except sa.error.SolverError:
            pass
        ctx.sync()
        t0 = time.perf_counter()
        try:
            vals, X, info = solve()
            status = "ok"
        except sa.error.InsufficientIterNum as e:
            vals, X, info, status = e.vals, e.X, e.info, "insufficient_iterations"
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3
        its = info["iters"] if "iters" in info else info["restarts"]
        r = dict(status=status, iters=its, matvecs=info["matvecs"], fallbacks=info["restarts"] if "iters" in info else 0, nconv=info["nconv"],
                 wall_ms=round(ms, 2), ms_per_iter=round(ms / max(1, its), 4), vals=[float(v) for v in vals], res=[float(v) for v in info["res"]])
        if X is not None:
            r["true_res0"] = float(np.linalg.norm(M @ X[0] - vals[0] * X[0]))
        rec["rows"][label] = r
        print("%s: %s" % (label, json.dumps(r)), file=sys.stderr, flush=True)

    for kind in KINDS:
        if args.only and kind != args.only:
            continue
        t0 = time.perf_counter()
        if kind == "jacobi":
            P = sa.DiagPrecond.new(M.diagonal().copy())
        elif kind == "fsai":
            P = sa.FSAI.new(A, 1)
        elif kind == "amg":
            P = sa.AMG.new(A)
        else:
            P = None
        ctx.sync()
        setup = (time.perf_counter() - t0) * 1e3
        timed(kind, lambda: S.solve(K, "smallest", precond=P, max_iter=args.cap, tol=TOL),
              lambda: S.solve(K, "smallest", precond=P, max_iter=min(2, args.cap), tol=TOL, vectors=False))
        rec["rows"][kind]["setup_ms"] = round(setup, 2)
        if P is not None:
            P.close()
    if not args.only or args.only == "eigsh":
        E = sa.Eigsh.new(A, n, NCV)
        timed("eigsh", lambda: E.solve(K, "smallest", max_restarts=args.cap, tol=TOL), lambda: E.solve(K, "smallest", max_restarts=2, tol=TOL, vectors=False))
        E.close()
    S.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def stats(args):
    rec = json.load(open(args.run))
    n, b = rec["n"], rec["block"]
    solves = [r["iters"] for label, r in rec["rows"].items() if label != "eigsh"]
    assert all(r["status"] == "insufficient_iterations" for label, r in rec["rows"].items() if label != "eigsh"), "cap the profiled run (--cap)"
    its = [rec["warmup_iters"]] * len(solves) + solves                        # every measured solve has its warm-up
    rows = list(csv.DictReader(open(args.stats)))
    vec = n * 8
    want = {
        "lob_gram_kernel": sum(2 * b + 4 * b + 6 * b * (i - 1) for i in its) * vec,
        "lz_rotate_kernel": sum(2 * (2 * b) + 2 * (5 * b) * i for i in its) * vec,
        "LobResid": sum(3 * b * (i + 1) for i in its) * vec,
    }
    out = {}
    for key, nbytes in want.items():
        sel = [r for r in rows if key in r["Name"]]
        if not sel:
            continue
        calls = sum(int(r["Calls"]) for r in sel)
        ns = sum(float(r["TotalDurationNs"]) for r in sel)
        out[key] = dict(calls=calls, mean_us=round(ns / calls / 1e3, 2), gbytes=round(nbytes / 1e9, 3), tb_per_s=round(nbytes / ns / 1e3, 3))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out["share_of_kernel_time"] = {key: round(sum(float(r["TotalDurationNs"]) for r in rows if key in r["Name"]) / total, 4) for key in want}
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap", type=int, default=3000, help="max_iter of the measured solves (max_restarts for Eigsh)")
    ap.add_argument("--only", choices=KINDS + ("eigsh",))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lobpcg_bench.json"))
    ap.add_argument("--stats", help="a rocprofv3 *_kernel_stats.csv of a run of this script")
    ap.add_argument("--run", help="that run's JSON")
    a = ap.parse_args()
    stats(a) if a.stats else run(a)
