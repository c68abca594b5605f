"""The truncated SVD solver (sprs_svds_*) on one GPU, on two operators: gen.poisson3d(128, 126, 124) — Hermitian positive definite,
so its singular values are its eigenvalues — and the first two thirds of that matrix's columns, a rectangular operator of
comparable size.  f64, k = 4, ncv = 32, the largest triplets, tol 1e-8, the default start vector, max_restarts capped (--cap).
Per operator: status, cycles, products, nconv, wall ms (one warm-up solve of two cycles first, a context synchronise before every
clock read), ms per cycle, the residual estimates and the true residuals of the leading triplet; for the square operator the same
figures of `Eigsh` (ncv = 32, largest) in the same process on the same handle beside them.  No speed threshold is set.
One JSON line to stdout and to --out PATH (default profiles/svds_bench.json).

    python scripts/svds_bench.py [--cap N] [--only square|rect] [--out PATH]

The projected-problem kernels are compared in a separate run of a few cycles under the profiler (timing never shares a run with it):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/svds_bench.py --only square --cap 6 --out DIR/run.json
    python scripts/svds_bench.py --stats DIR/.../*_kernel_stats.csv

which prints, for sv_svd_kernel and lz_ritz_kernel (and the other kernels of the run, grouped), calls, mean microseconds and the
share of the run's kernel time."""
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


def first_columns(ip, ix, d, ncols):
    """The CSR arrays of A[:, :ncols]."""
    import numpy as np
    keep = ix < ncols
    cnt = np.add.reduceat(keep.astype(np.int64), ip[:-1].astype(np.int64))
    cnt[np.diff(ip) == 0] = 0
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), ix[keep].astype(np.int32), d[keep]


def timed(ctx, sa, solve, warm):
    try:
        warm()
    except sa.error.SolverError:
        pass
    ctx.sync()
    t0 = time.perf_counter()
    try:
        out, status = solve(), "ok"
    except sa.error.InsufficientIterNum as e:
        out, status = e, "insufficient_restarts"
    ctx.sync()
    return out, status, (time.perf_counter() - t0) * 1e3


def run(args):
    import numpy as np
    import scipy.sparse as sp

    import sprsolve_amd as sa
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    ip, ix, d = gen.poisson3d(*GRID)[:3]
    n = ip.size - 1
    rec = dict(grid=list(GRID), dtype="float64", k=K, ncv=NCV, p=restart_size(K, NCV), tol=TOL, cap=args.cap, which="largest", operators={})
    for label in ("square", "rect"):
        if args.only and label != args.only:
            continue
        shape = (n, n) if label == "square" else (n, 2 * n // 3)
        a_ip, a_ix, a_d = (ip, ix, d) if label == "square" else first_columns(ip, ix, d, shape[1])
        A = sa.HipCsr.new(shape, a_ip, a_ix, a_d)
        S = sa.Svds.new(A, NCV)
        out, status, ms = timed(ctx, sa, lambda: S.solve(K, "largest", max_restarts=args.cap, tol=TOL),
                                lambda: S.solve(K, "largest", max_restarts=2, tol=TOL, vectors=False))
        s, U, V, info = (out.s, out.U, out.V, out.info) if status != "ok" else out
        M = sp.csr_matrix((a_d, a_ix, a_ip), shape=shape)
        r = dict(rows=int(shape[0]), cols=int(shape[1]), nnz=int(a_ip[-1]), spmv_kernel=A.spmv_route()["kernel"], status=status,
                 cycles=info["restarts"], products=info["matvecs"], nconv=info["nconv"], wall_ms=round(ms, 2),
                 ms_per_cycle=round(ms / max(1, info["restarts"]), 4), s=[float(v) for v in s], res=[float(v) for v in info["res"]],
                 true_res0=[float(np.linalg.norm(M @ V[0] - s[0] * U[0])), float(np.linalg.norm(M.T @ U[0] - s[0] * V[0]))])
        S.close()
        if label == "square":
            E = sa.Eigsh.new(A, n, NCV)
            out, status, ms = timed(ctx, sa, lambda: E.solve(K, "largest", max_restarts=args.cap, tol=TOL),
                                    lambda: E.solve(K, "largest", max_restarts=2, tol=TOL, vectors=False))
            vals, X, einfo = (out.vals, out.X, out.info) if status != "ok" else out
            r["eigsh"] = dict(status=status, cycles=einfo["restarts"], products=einfo["matvecs"], nconv=einfo["nconv"], wall_ms=round(ms, 2),
                              ms_per_cycle=round(ms / max(1, einfo["restarts"]), 4), vals=[float(v) for v in vals])
            E.close()
        rec["operators"][label] = r
        print("%s: %s" % (label, json.dumps(r)), file=sys.stderr, flush=True)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def stats(args):
    rows = list(csv.DictReader(open(args.stats)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {}
    for key in ("sv_svd_kernel", "lz_ritz_kernel", "sv_norm_kernel", "lz_step_kernel", "GmDots", "GmUpdate", "GmScale", "lz_rotate_kernel"):
        sel = [r for r in rows if key in r["Name"]]
        if not sel:
            continue
        calls = sum(int(r["Calls"]) for r in sel)
        ns = sum(float(r["TotalDurationNs"]) for r in sel)
        out[key] = dict(calls=calls, mean_us=round(ns / calls / 1e3, 2), share_pct=round(100.0 * ns / total, 2))
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cap", type=int, default=300, help="max_restarts of the measured solves")
    ap.add_argument("--only", choices=("square", "rect"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svds_bench.json"))
    ap.add_argument("--stats", help="a rocprofv3 *_kernel_stats.csv of a run of this script")
    a = ap.parse_args()
    stats(a) if a.stats else run(a)
