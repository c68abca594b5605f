"""The batch BiCGStab (BatchCsr.bicgstab: one launch, one workgroup per system) beside the route a user has without it: one HipCsr
and one BiCGStab handle per system, looped over the batch with the device entry point.  f64, gen.batch_convection_diffusion, x0 = 0,
tol 1e-8, one GPU, one build.  Sizes: n = 256 (16 x 16) and n = 1024 (32 x 32) rows, nbatch in {256, 4096, 16384}.  Per size, in
alternation within one run after one warm-up of each, REPS repeats, every figure listed and the median reported:

  (a)  one bicgstab call on the whole batch, rhs and x in HBM, without and with Jacobi;
  (b)  the loop of solve_dev / precond_solve calls, handle creation outside the timed window, without and with Jacobi (a
       DiagPrecond per system) — over the FIRST min(nbatch, LOOP_SYSTEMS) systems of the batch only: nbatch handles of the
       single-system library are out of proportion (the generator's streams are counter-based, so those systems are the same in
       every nbatch), and its systems / s does not depend on how many follow.

Times are wall milliseconds from a host clock around work that ends in a context synchronise.  Reported: systems / s of both
sides, the mean iterations per system of both over the systems both solved (they differ by the summation order only), how many
systems did not end in Ok, and the largest difference of the two sides' solutions.

Then, in a child process under `rocprofv3 --kernel-trace --stats`, one bicgstab call without Jacobi at nbatch = 4096 for both n:
the kernel's microseconds, and the product's algorithmic bytes over them — every product of system b reads its nnz values
(8 bytes) and the pattern's nnz column indices (4 bytes), and a solve that ends after `its` iterations has formed 1 + 2 its
products.  Every figure is from a single run.  One JSON line to stdout and to --out PATH (default profiles/batch_bench.json).

    python scripts/batch_bench.py [--no-profile] [--out PATH]"""
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

GRIDS = ((16, 16), (32, 32))
NBATCH = (256, 4096, 16384)
LOOP_SYSTEMS = 256
TOL = 1e-8
MAX_ITER = 2000
REPS = 3
PROFILE_NBATCH = 4096


def _diag(ip, ix, v):
    import numpy as np
    return v[np.repeat(np.arange(ip.size - 1), np.diff(ip)) == ix]


def child(out):
    """The timed comparison in this process; the record goes to `out`."""
    import numpy as np
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    rec = dict(dtype="float64", tol=TOL, max_iter=MAX_ITER, reps=REPS, loop_systems=LOOP_SYSTEMS, single_run=True, sizes={})
    for grid in GRIDS:
        n = grid[0] * grid[1]
        loop = None
        for nb in NBATCH:
            ip, ix, V, RHS = gen.batch_convection_diffusion(grid[0], grid[1], nb, np.float64)
            B = sa.BatchCsr.new(n, ip, ix, V)
            dR = sa.DevVec.from_numpy(RHS.ravel()); dX = sa.DevVec(nb * n, np.float64, ctx)
            m = min(nb, LOOP_SYSTEMS)
            if loop is None:                                         # the first m systems are the same in every nbatch
                loop = []
                for b in range(m):
                    A = sa.HipCsr.new((n, n), ip, ix, V[b])
                    loop.append((A, sa.BiCGStab.new(A, n), sa.DiagPrecond.new(_diag(ip, ix, V[b])), sa.DevVec.from_numpy(RHS[b]),
                                 sa.DevVec(n, np.float64, ctx)))

            def run_batch(pc):
                dX.zero()
                ctx.sync(); t0 = time.perf_counter()
                its, res, st = B.bicgstab(dR, dX, MAX_ITER, TOL, precond=pc)
                ctx.sync()
                return (time.perf_counter() - t0) * 1e3, its, st

            def run_loop(pc):
                for h in loop[:m]:
                    h[4].zero()
                its = np.zeros(m, np.int64); st = np.zeros(m, np.int32)
                ctx.sync(); t0 = time.perf_counter()
                for b, (A, s, P, r, x) in enumerate(loop[:m]):
                    try:
                        its[b] = (s.precond_solve(P, r, x, MAX_ITER, TOL) if pc else s.solve(r, x, MAX_ITER, TOL))[0]
                    except sa.error.SolverError as e:
                        st[b] = 1; its[b] = getattr(e, "iters", getattr(e, "its", 0))
                ctx.sync()
                return (time.perf_counter() - t0) * 1e3, its, st

            size = {}
            for pc in (None, "jacobi"):
                run_batch(pc); run_loop(pc)                          # warm-up of both
                ta, tb = [], []
                for _ in range(REPS):
                    a, its_a, st_a = run_batch(pc); b, its_b, st_b = run_loop(pc)
                    ta.append(a); tb.append(b)
                X = dX.to_numpy().reshape(nb, n)
                both = (st_a[:m] == 0) & (st_b == 0)
                diff = max((float(np.max(np.abs(X[j] - loop[j][4].to_numpy())) / max(1.0, float(np.max(np.abs(X[j]))))) for j in np.nonzero(both)[0]),
                           default=0.0)
                ma, mb = statistics.median(ta), statistics.median(tb)
                size["jacobi" if pc else "none"] = dict(
                    batch_ms=[round(t, 3) for t in ta], loop_ms=[round(t, 3) for t in tb], batch_ms_median=round(ma, 3), loop_ms_median=round(mb, 3),
                    batch_systems_per_s=round(nb / ma * 1e3, 1), loop_systems_per_s=round(m / mb * 1e3, 1), ratio=round((nb / ma) / (m / mb), 2),
                    loop_over=int(m), batch_not_ok=int(np.count_nonzero(st_a)), loop_not_ok=int(np.count_nonzero(st_b)),
                    mean_its_batch_all=round(float(its_a.mean()), 2), mean_its_batch=round(float(its_a[:m][both].mean()), 2),
                    mean_its_loop=round(float(its_b[both].mean()), 2), max_its_batch=int(its_a.max()), max_rel_diff=diff)
            rec["sizes"]["n%d_nb%d" % (n, nb)] = dict(n=n, nnz=int(ip[-1]), nbatch=nb, threads=B.info["threads"], lds_bicgstab=B.info["lds_bicgstab"], **size)
            B.close()
            del dR, dX, V, RHS
    with open(out, "w") as f:
        f.write(json.dumps(rec) + "\n")


def child_kernels(out):
    """One bicgstab call without Jacobi per grid at PROFILE_NBATCH systems; the iterations of every system go to `out`."""
    import numpy as np
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    rec = {}
    for grid in GRIDS:
        n = grid[0] * grid[1]
        ip, ix, V, RHS = gen.batch_convection_diffusion(grid[0], grid[1], PROFILE_NBATCH, np.float64)
        B = sa.BatchCsr.new(n, ip, ix, V)
        dR = sa.DevVec.from_numpy(RHS.ravel()); dX = sa.DevVec(PROFILE_NBATCH * n, np.float64, ctx); dX.zero()
        its, res, st = B.bicgstab(dR, dX, MAX_ITER, TOL)
        ctx.sync()
        rec["n%d" % n] = dict(n=n, nnz=int(ip[-1]), nbatch=PROFILE_NBATCH, products=int(np.sum(1 + 2 * its)), not_ok=int(np.count_nonzero(st)))
        B.close()
    with open(out, "w") as f:
        f.write(json.dumps(rec) + "\n")


def kernel_stats(path, runs):
    """The solve kernel's calls and microseconds from a rocprofv3 kernel-trace table of child_kernels(): one call per grid, in
    the order of GRIDS."""
    rows = [r for r in csv.DictReader(open(path)) if "batch_bicgstab_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for r, (key, run) in zip(rows, runs.items()):
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        nbytes = run["products"] * run["nnz"] * 12
        out[key] = dict(kernel_us=round(us, 1), products=run["products"], product_bytes=nbytes, product_tb_per_s=round(nbytes / us / 1e6, 3),
                        systems_per_s_kernel=round(run["nbatch"] / us * 1e6, 1), not_ok=run["not_ok"])
    return out


def main(args):
    me = os.path.abspath(__file__)
    with tempfile.TemporaryDirectory() as tmp:
        run = os.path.join(tmp, "run.json")
        subprocess.run([sys.executable, me, "--child", run], check=True, timeout=1500)
        rec = json.load(open(run))
        if not args.no_profile:
            prof = os.path.join(tmp, "prof.json")
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(tmp, "rp"), "--",
                            sys.executable, me, "--child-kernels", prof], check=True, timeout=600, stdout=subprocess.DEVNULL)
            tables = glob.glob(os.path.join(tmp, "rp", "**", "*_kernel_trace.csv"), recursive=True)
            assert len(tables) == 1, tables
            rec["profiled"] = kernel_stats(tables[0], json.load(open(prof)))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-profile", action="store_true", help="skip the run under rocprofv3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_bench.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--child-kernels", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child)
    elif a.child_kernels:
        child_kernels(a.child_kernels)
    else:
        main(a)
