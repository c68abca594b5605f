"""The thick-restart Lanczos eigensolver (sprs_eigsh_*) on one GPU: gen.poisson3d(128, 126, 124) — unequal sides, so the spectrum is
simple — f64, k = 4, ncv = 32, both ends of the spectrum, tol 1e-8, the default start vector, max_restarts capped (--cap) so that a
run ends within a minute whether it converges or not; then the smallest end once more under --short-cap cycles, a run that does not
converge.  Per end: status, cycles, matvecs, nconv, wall ms (one warm-up solve of two
cycles first, a context synchronise before every clock read), ms per cycle, the residual estimates.  No speed threshold is set.
One JSON line to stdout and to --out PATH (default profiles/eigsh_bench.json).

    python scripts/eigsh_bench.py [--cap N] [--only largest|smallest] [--out PATH]

The rotation kernel's rate is taken from a separate run under the profiler (counters and timing never share a run):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/eigsh_bench.py --only largest --cap 12 --out DIR/run.json
    python scripts/eigsh_bench.py --stats DIR/.../*_kernel_stats.csv --run DIR/run.json

which prints, for LzRotate and for GmUpdate (the fused vector kernel beside it in the same run), calls, mean microseconds, the
bytes each must move and bytes / time.  LzRotate moves (m + q) n 8 bytes a call: q = p in a restart, q = k for the eigenvectors;
GmUpdate at step j moves (j + 3) n 8 (v_0 .. v_j and w read, one vector written)."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = (128, 126, 124)
K, NCV, TOL = 4, 32, 1e-8


def restart_size(k, m):
    return min(k + max(k, 4), m - 2)


def run(args):
    import numpy as np

    import sprsolve_amd as sa
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    ip, ix, d = gen.poisson3d(*GRID)[:3]
    n = ip.size - 1
    A = sa.HipCsr.new((n, n), ip, ix, d)
    E = sa.Eigsh.new(A, n, NCV)
    rec = dict(grid=list(GRID), n=int(n), nnz=int(ip[-1]), dtype="float64", k=K, ncv=NCV, p=restart_size(K, NCV), tol=TOL, cap=args.cap, short_cap=args.short_cap,
               spmv_kernel=A.spmv_route()["kernel"], stream_format=A.stream_format(), ends={})
    for which, cap in (("largest", args.cap), ("smallest", args.cap), ("smallest_short", args.short_cap)):
        label, which = which, which.split("_")[0]
        if args.only and label != args.only:
            continue
        try:
            E.solve(K, which, max_restarts=2, tol=TOL, vectors=False)        # warm-up
        except sa.error.SolverError:
            pass
        ctx.sync()
        t0 = time.perf_counter()
        try:
            vals, X, info = E.solve(K, which, max_restarts=cap, tol=TOL)
            status = "ok"
        except sa.error.InsufficientIterNum as e:
            vals, X, info, status = e.vals, e.X, e.info, "insufficient_restarts"
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3
        r = dict(status=status, cycles=info["restarts"], matvecs=info["matvecs"], nconv=info["nconv"], wall_ms=round(ms, 2),
                 ms_per_cycle=round(ms / max(1, info["restarts"]), 4), vals=[float(v) for v in vals], res=[float(v) for v in info["res"]])
        if X is not None:                                                    # the true residual of the leading pair, on the host
            import scipy.sparse as sp
            M = sp.csr_matrix((d, ix, ip), shape=(n, n))
            r["true_res0"] = float(np.linalg.norm(M @ X[0] - vals[0] * X[0]))
        rec["ends"][label] = r
        print("%s: %s" % (label, json.dumps(r)), file=sys.stderr, flush=True)
    E.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def stats(args):
    rec = json.load(open(args.run))
    n, m, p, k = rec["n"], rec["ncv"], rec["p"], rec["k"]
    ends = rec["ends"]
    cycles = sum(e["cycles"] for e in ends.values()) + 2 * len(ends)          # + the warm-up solves of two cycles each
    solves = 2 * len(ends)
    restarts = cycles - solves                                                # every cycle but a solve's last is followed by a restart
    rows = list(csv.DictReader(open(args.stats)))
    out = {}
    for key in ("lz_rotate_kernel", "GmUpdate"):
        sel = [r for r in rows if key in r["Name"]]
        if not sel:
            continue
        calls = sum(int(r["Calls"]) for r in sel)
        ns = sum(float(r["TotalDurationNs"]) for r in sel)
        if key == "lz_rotate_kernel":
            with_vecs = len(ends)                                             # the measured solves form X; the warm-ups do not
            nbytes = (restarts * (m + p) + with_vecs * (m + k)) * n * 8
        else:
            # two GmUpdate launches a step; step j moves (j + 3) n 8 bytes; a solve's first cycle runs j = 0 .. m - 1, the others p .. m - 1
            first = sum(j + 3 for j in range(m))
            later = sum(j + 3 for j in range(p, m))
            nbytes = 2 * (solves * first + (cycles - solves) * later) * n * 8
        out[key] = dict(calls=calls, mean_us=round(ns / calls / 1e3, 2), gbytes=round(nbytes / 1e9, 3), tb_per_s=round(nbytes / ns / 1e3, 3))
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap", type=int, default=1500, help="max_restarts of the measured solves")
    ap.add_argument("--short-cap", type=int, default=20, help="max_restarts of the third run (the smallest end again): one that does not converge")
    ap.add_argument("--only", choices=("largest", "smallest"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eigsh_bench.json"))
    ap.add_argument("--stats", help="a rocprofv3 *_kernel_stats.csv of a run of this script")
    ap.add_argument("--run", help="that run's JSON")
    a = ap.parse_args()
    stats(a) if a.stats else run(a)
