"""Multi-shift CG (sprs_cgshift_solve_dev) beside m separate sprs_cg_solve_dev calls on handles of A + sigma_j I, f64, no
preconditioner, one GPU, one build: gen.poisson3d(128, 128, 128) with the generator's rhs, tol 1e-8, m in {1, 4, 8}, the shifts
diag * 10^e with e spread evenly over [-2, 2] (four decades around the diagonal, 6).  The separate side is the single-solve code,
which this feature leaves untouched.  Per m: the wall ms of one CGShift solve and of the m CG solves together (a context
synchronise before every clock read; REPS alternating repeats after one warm-up of each, every figure listed and the median
reported), the iterations of each column on both sides, and the largest difference of the two sides' solutions.

The traffic model: a separate iteration is one SpMV (S vector passes' worth) and 9 passes, a multi-shift one is one SpMV and
6 + 4 m passes, so m separate solves of equal length against one multi-shift solve predict m (S + 9) / (S + 6 + 4 m); the record
carries that figure with S measured as the SpMV's time over a vector pass's time in the profiled run.

Then, in a child process under `rocprofv3 --kernel-trace --stats`, KERNEL_STEPS iterations at tol 0 (no column converges: all
eight stay active) of the m = 8 solve and of one CG solve on A: calls, mean microseconds and bytes / time of CgShiftSC
((3 + 4 * 8) n 8 bytes a call), CgShiftSB (3 n 8), CgKB (6 n 8) and CgKC (3 n 8), and the SpMV's mean microseconds.  Every figure
is from a single run.  One JSON line to stdout and to --out PATH (default profiles/cg_shift_bench.json).

    python scripts/cg_shift_bench.py [--no-profile] [--out PATH]"""
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

GRID = (128, 128, 128)
DIAG = 6.0
TOL = 1e-8
MAX_ITER = 2000
MS = (1, 4, 8)
REPS = 3
KERNEL_STEPS = 40


def shifts_for(m):
    import numpy as np
    return [float(DIAG * 10.0 ** e) for e in np.linspace(-2.0, 2.0, m)]


def _shifted(ip, ix, d, sigma):
    import numpy as np
    out = d.copy()
    out[np.repeat(np.arange(ip.size - 1), np.diff(ip)) == ix] += sigma
    return out


def child(out):
    """The timed comparison in this process; the record goes to `out`."""
    import numpy as np
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = gen.poisson3d(*GRID)
    n = ip.size - 1
    A = sa.HipCsr.new((n, n), ip, ix, d)
    dB = sa.DevVec.from_numpy(rhs)
    rec = dict(grid=list(GRID), n=int(n), nnz=int(ip[-1]), dtype="float64", tol=TOL, spmv_kernel=A.spmv_route()["kernel"], reps=REPS, single_run=True)
    handles = {}
    for m in MS:
        sh = shifts_for(m)
        for s in sh:
            if s not in handles:
                As = sa.HipCsr.new((n, n), ip, ix, _shifted(ip, ix, d, s))
                handles[s] = (As, sa.CG.new(As, n))
        multi = sa.CGShift.new(A, n, m)
        dX = sa.DevVec(m * n, "float64", ctx)
        xs = [sa.DevVec(n, "float64", ctx) for _ in sh]

        def run_multi():
            ctx.sync(); t0 = time.perf_counter()
            its, res, st = multi.solve(sh, dB, dX, MAX_ITER, TOL)
            ctx.sync()
            assert not np.any(st), st
            return (time.perf_counter() - t0) * 1e3, its

        def run_separate():
            for x in xs:
                x.zero()
            ctx.sync(); t0 = time.perf_counter()
            its = [handles[s][1].solve(dB, x, MAX_ITER, TOL)[0] for s, x in zip(sh, xs)]
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3, its

        run_multi(); run_separate()                              # warm-up of both
        tm, ts = [], []
        for _ in range(REPS):
            a, its_m = run_multi(); b, its_s = run_separate()
            tm.append(a); ts.append(b)
        X = dX.to_numpy().reshape(m, n)
        diff = max(float(np.max(np.abs(X[j] - xs[j].to_numpy())) / max(1.0, float(np.max(np.abs(X[j]))))) for j in range(m))
        mm, sm = statistics.median(tm), statistics.median(ts)
        rec["m%d" % m] = dict(shifts=sh, multi_ms=[round(t, 3) for t in tm], separate_ms=[round(t, 3) for t in ts], multi_ms_median=round(mm, 3),
                              separate_ms_median=round(sm, 3), speedup=round(sm / mm, 3), its_multi=[int(v) for v in its_m],
                              its_separate=[int(v) for v in its_s], max_rel_diff=diff)
        multi.close()
        del dX, xs
    with open(out, "w") as f:
        f.write(json.dumps(rec) + "\n")


def child_kernels(out):
    """KERNEL_STEPS iterations of the m = 8 multi-shift solve and of one CG solve on A, none of which converges (tol 0)."""
    import numpy as np
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = gen.poisson3d(*GRID)
    n = ip.size - 1
    A = sa.HipCsr.new((n, n), ip, ix, d)
    dB = sa.DevVec.from_numpy(rhs)
    multi = sa.CGShift.new(A, n, 8)
    dX = sa.DevVec(8 * n, "float64", ctx)
    its, res, st = multi.solve(shifts_for(8), dB, dX, KERNEL_STEPS, 0.0)
    assert np.all(st == 3), st                                    # every column still running: all eight were active throughout
    x = sa.DevVec(n, "float64", ctx); x.zero()
    try:
        sa.CG.new(A, n).solve(dB, x, KERNEL_STEPS, 0.0)
        raise SystemExit("the fixed-step CG solve returned early")
    except sa.error.InsufficientIterNum:
        pass
    ctx.sync()
    with open(out, "w") as f:
        f.write(json.dumps(dict(n=int(n), steps=KERNEL_STEPS)) + "\n")


def kernel_stats(path, n):
    """Calls, mean microseconds and bytes / time of the vector kernels from a rocprofv3 kernel-stats table of child_kernels()."""
    passes = {"CgShiftSC": 3 + 4 * 8, "CgShiftSB": 3, "CgKB": 6, "CgKC": 3}
    rows = list(csv.DictReader(open(path)))
    out = {}
    for key, p in passes.items():
        sel = [r for r in rows if key + "I" in r["Name"] or key + "<" in r["Name"]]
        if not sel:
            continue
        calls = sum(int(r["Calls"]) for r in sel)
        ns = sum(float(r["TotalDurationNs"]) for r in sel)
        out[key] = dict(calls=calls, mean_us=round(ns / calls / 1e3, 2), bytes_per_call=p * n * 8, tb_per_s=round(p * n * 8.0 * calls / ns / 1e3, 3))
    sel = [r for r in rows if "spmv_" in r["Name"] and int(r["Calls"]) >= KERNEL_STEPS]      # the two solves' SpMVs (one route)
    if sel:
        calls = sum(int(r["Calls"]) for r in sel)
        ns = sum(float(r["TotalDurationNs"]) for r in sel)
        out["spmv"] = dict(calls=calls, mean_us=round(ns / calls / 1e3, 2), kernels=sorted(set(r["Name"][:60] for r in sel)))
    return out


def main(args):
    me = os.path.abspath(__file__)
    with tempfile.TemporaryDirectory() as tmp:
        run = os.path.join(tmp, "run.json")
        subprocess.run([sys.executable, me, "--child", run], check=True, timeout=900)
        rec = json.load(open(run))
        if not args.no_profile:
            prof = os.path.join(tmp, "prof.json")
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(tmp, "rp"), "--",
                            sys.executable, me, "--child-kernels", prof], check=True, timeout=600, stdout=subprocess.DEVNULL)
            tables = glob.glob(os.path.join(tmp, "rp", "**", "*_kernel_stats.csv"), recursive=True)
            assert len(tables) == 1, tables
            ks = kernel_stats(tables[0], rec["n"])
            rec["profiled"] = ks
            if "spmv" in ks and "CgKC" in ks:
                # S: the SpMV in vector passes, a pass timed as a third of CgKC (3 passes) in the same run
                S = ks["spmv"]["mean_us"] / (ks["CgKC"]["mean_us"] / 3.0)
                rec["model"] = dict(S=round(S, 2), **{"m%d" % m: round(m * (S + 9) / (S + 6 + 4 * m), 3) for m in MS})
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-profile", action="store_true", help="skip the run under rocprofv3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cg_shift_bench.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--child-kernels", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child)
    elif a.child_kernels:
        child_kernels(a.child_kernels)
    else:
        main(a)
