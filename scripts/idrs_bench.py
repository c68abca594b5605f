"""IDR(s) (sprs_idrs_solve_dev) beside BiCGStab and GMRES(30) on the same operator handle: gen.convection_diffusion_2d(1024, 1024),
GMRES's own bench operator, f64, the generator's rhs, x0 = 0, tol 1e-8, one GPU, one build; preconditioned by nothing, Jacobi and
AMG; IDRS with s = 1, 2, 4, 8.  A second run with cx = 4, cy = 3 (convection-dominated) is recorded where at least one baseline
solves that matrix.  Per solver: the status, the products with A (IDR(s): its; BiCGStab: 2 its; GMRES: its + one per cycle), the
wall ms to solution (a context synchronise before every clock read, REPS repeats after one warm-up solve, every figure listed and
the median reported) and the true residual |rhs - A x| / |rhs| formed on the host in double.

Then, in a child process under `rocprofv3 --kernel-trace --stats`, KERNEL_STEPS products at tol 0 of IDR(4) without a
preconditioner and of GMRES(30): calls, mean microseconds and bytes / time of IdrsA (mean over k of 2 (s - k) + 2 vector passes =
7 at s = 4), IdrsB (2 k + 8: 11), IdrsW (3 + s reads, 2 writes: 9), the multi-dot (1 + s: 5) and GMRES's GmUpdate (j + 3: 17.5 over
whole cycles), n 8 bytes a pass.

With --headline-parent DIR (the parent commit's tree, built), `python bench.py --gpus 1 --steps K --warmup W` runs alternately in
DIR and in this tree, HEADLINE_REPS times each, and both series are recorded: this feature adds a translation unit and touches
no existing kernel, so the difference of the medians must lie inside the parent's own spread.  Every figure is from a single
run.  One JSON line to stdout and to --out PATH (default profiles/idrs_bench.json).

    python scripts/idrs_bench.py [--no-profile] [--headline-parent DIR [--headline-only]] [--out PATH]"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = (1024, 1024)
TOL = 1e-8
MAX_PRODUCTS = 20000
S_DIMS = (1, 2, 4, 8)
REPS = 3
KERNEL_STEPS = 200
HEADLINE_REPS = 3
HEADLINE_ARGS = ["--gpus", "1", "--steps", "100", "--warmup", "20"]


def _timed(sa, ctx, np, run, x, n):
    """One warm-up, then REPS timed solves from x = 0 -> (status, its, [ms])."""
    ms = []
    status, its = "ok", 0
    for rep in range(REPS + 1):
        x.zero()
        ctx.sync(); t0 = time.perf_counter()
        try:
            its = run(x)[0]
        except sa.error.InsufficientIterNum as e:
            status, its = "insufficient_iter", e.iters
        except sa.error.BreakDown as e:
            status, its = "breakdown", e.its
        ctx.sync()
        if rep:
            ms.append((time.perf_counter() - t0) * 1e3)
        if status != "ok":
            break
    return status, int(its), ms


def child(out, cx, cy):
    """The timed comparison on one operator in this process; the record goes to `out`."""
    import numpy as np
    import scipy.sparse as sp
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = gen.convection_diffusion_2d(GRID[0], GRID[1], cx=cx, cy=cy)
    n = ip.size - 1
    Ah = sp.csr_matrix((d, ix, ip), shape=(n, n))
    rhs_norm = float(np.linalg.norm(rhs))
    A = sa.HipCsr.new((n, n), ip, ix, d)
    dB = sa.DevVec.from_numpy(rhs)
    x = sa.DevVec(n, "float64", ctx)
    rec = dict(grid=list(GRID), cx=cx, cy=cy, n=int(n), nnz=int(ip[-1]), dtype="float64", tol=TOL, reps=REPS,
               spmv_kernel=A.spmv_route()["kernel"], single_run=True)
    preconds = {"none": None, "jacobi": sa.DiagPrecond.new(np.full(n, 4.0))}
    try:
        preconds["amg"] = sa.AMG.new(A)
    except Exception as e:                                       # (no hierarchy for this matrix: recorded, not hidden)
        rec["amg"] = dict(error=repr(e))
    bicg, gm = sa.BiCGStab.new(A, n), sa.GMRES.new(A, n, 30)
    idrs = {s: sa.IDRS.new(A, n, s) for s in S_DIMS}
    for pname, P in preconds.items():
        solve = lambda S, mi: (lambda xx: S.solve(dB, xx, mi, TOL)) if P is None else (lambda xx: S.precond_solve(P, dB, xx, mi, TOL))
        runs = [("bicgstab", solve(bicg, MAX_PRODUCTS // 2), lambda its: 2 * its), ("gmres30", solve(gm, MAX_PRODUCTS), lambda its: its + (its + 29) // 30)]
        runs += [("idrs%d" % s, solve(idrs[s], MAX_PRODUCTS), lambda its: its) for s in S_DIMS]
        block = {}
        for name, run, products in runs:
            status, its, ms = _timed(sa, ctx, np, run, x, n)
            xh = x.to_numpy()
            true = float(np.linalg.norm(rhs - Ah @ xh)) / rhs_norm
            block[name] = dict(status=status, its=its, products=int(products(its)), ms=[round(t, 3) for t in ms],
                               ms_median=round(statistics.median(ms), 3) if ms else None, true_res=true)
        rec[pname] = block
    with open(out, "w") as f:
        f.write(json.dumps(rec) + "\n")


def child_kernels(out):
    """KERNEL_STEPS products of IDR(4) and of GMRES(30) without a preconditioner, neither of which converges (tol 0)."""
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = gen.convection_diffusion_2d(*GRID)
    n = ip.size - 1
    A = sa.HipCsr.new((n, n), ip, ix, d)
    dB = sa.DevVec.from_numpy(rhs)
    x = sa.DevVec(n, "float64", ctx)
    for S, steps in ((sa.IDRS.new(A, n, 4), KERNEL_STEPS), (sa.GMRES.new(A, n, 30), 60)):
        x.zero()
        try:
            S.solve(dB, x, steps, 0.0)
            raise SystemExit("a fixed-step solve returned early")
        except sa.error.InsufficientIterNum:
            pass
    ctx.sync()
    with open(out, "w") as f:
        f.write(json.dumps(dict(n=int(n), steps=KERNEL_STEPS)) + "\n")


def kernel_stats(path, n):
    """Calls, mean microseconds and bytes / time of the vector kernels from a rocprofv3 kernel-stats table of child_kernels()."""
    passes = {"IdrsA": 7.0, "IdrsB": 11.0, "IdrsW": 9.0, "IdrsDots": 5.0, "GmUpdate": 17.5}
    rows = list(csv.DictReader(open(path)))
    out = {}
    for key, p in passes.items():
        sel = [r for r in rows if key + "I" in r["Name"] or key + "<" in r["Name"]]
        if not sel:
            continue
        calls = sum(int(r["Calls"]) for r in sel)
        ns = sum(float(r["TotalDurationNs"]) for r in sel)
        out[key] = dict(calls=calls, mean_us=round(ns / calls / 1e3, 2), passes=p, bytes_per_call=p * n * 8, tb_per_s=round(p * n * 8.0 * calls / ns / 1e3, 3))
    sel = [r for r in rows if "spmv_" in r["Name"] and int(r["Calls"]) >= 60]
    if sel:
        calls = sum(int(r["Calls"]) for r in sel)
        ns = sum(float(r["TotalDurationNs"]) for r in sel)
        out["spmv"] = dict(calls=calls, mean_us=round(ns / calls / 1e3, 2), kernels=sorted(set(r["Name"][:60] for r in sel)))
    return out


def headline(parent):
    """bench.py's headline in the parent's tree and in this one, alternating."""
    series = {"parent": [], "this": []}
    for _ in range(HEADLINE_REPS):
        for name, root in (("parent", parent), ("this", ROOT)):
            p = subprocess.run([sys.executable, "bench.py"] + HEADLINE_ARGS, cwd=root, check=True, timeout=900, stdout=subprocess.PIPE, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln][-1]
            series[name].append(float(json.loads(line)["value"]))
    med = {k: statistics.median(v) for k, v in series.items()}
    return dict(args=HEADLINE_ARGS, unit="iterations/s", parent=series["parent"], this=series["this"], parent_median=med["parent"], this_median=med["this"],
                parent_spread=max(series["parent"]) - min(series["parent"]), median_difference=med["this"] - med["parent"])


def main(args):
    me = os.path.abspath(__file__)
    if args.headline_only:                                       # add the headline series to the record already at --out
        rec = json.load(open(args.out))
        rec["headline"] = headline(os.path.abspath(args.headline_parent))
        line = json.dumps(rec)
        print(line)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        return
    with tempfile.TemporaryDirectory() as tmp:
        run = os.path.join(tmp, "run.json")
        subprocess.run([sys.executable, me, "--child", run], check=True, timeout=900)
        rec = json.load(open(run))
        hard_run = os.path.join(tmp, "hard.json")
        subprocess.run([sys.executable, me, "--child", hard_run, "--cx", "4.0", "--cy", "3.0"], check=True, timeout=900)
        hard = json.load(open(hard_run))
        solved = [p for p in ("none", "jacobi", "amg") if isinstance(hard.get(p), dict) and "bicgstab" in hard[p]
                  and any(hard[p][b]["status"] == "ok" for b in ("bicgstab", "gmres30"))]
        if solved:
            rec["convection_dominated"] = hard
        if not args.no_profile:
            prof = os.path.join(tmp, "prof.json")
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(tmp, "rp"), "--",
                            sys.executable, me, "--child-kernels", prof], check=True, timeout=600, stdout=subprocess.DEVNULL)
            tables = glob.glob(os.path.join(tmp, "rp", "**", "*_kernel_stats.csv"), recursive=True)
            assert len(tables) == 1, tables
            rec["profiled"] = kernel_stats(tables[0], rec["n"])
    if args.headline_parent:
        rec["headline"] = headline(os.path.abspath(args.headline_parent))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-profile", action="store_true", help="skip the run under rocprofv3")
    ap.add_argument("--headline-parent", metavar="DIR", help="the parent commit's built tree: bench.py alternates between it and this one")
    ap.add_argument("--headline-only", action="store_true", help="with --headline-parent: only that, added to the record at --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "idrs_bench.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--child-kernels", help=argparse.SUPPRESS)
    ap.add_argument("--cx", type=float, default=0.3, help=argparse.SUPPRESS)
    ap.add_argument("--cy", type=float, default=0.2, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.cx, a.cy)
    elif a.child_kernels:
        child_kernels(a.child_kernels)
    else:
        main(a)
