"""ILU(0) with Jacobi-sweep triangular solves (k = 2 .. 5) beside the exact level-scheduled ILU(0), Jacobi and no preconditioner
(and, for CG, AMG): one GPU, one process, one build, f64, x0 = 0, a seeded uniform right-hand side, tol 1e-8.
  (a) CG on the 7-point 3-D Poisson matrix (gen.poisson3d, 128^3 by default): scripts/amg_bench.py's system.
  (b) GMRES(30) on the non-symmetric 5-point operator (gen.convection_diffusion_2d, 1024 x 1024 by default).
Per row: iterations, ms to solution (after one warm-up solve: median and spread = max - min of three, a context synchronise before
every clock read), the status (a solve that ran out of max_iter reports where it stood: its residual estimate is nan, the true
relative residual is computed), microseconds per preconditioner application (median and spread of three batches of REPS
asynchronous applications and one wait), launches per application, handle-creation ms.  The baselines are the Jacobi and the exact
ILU(0) rows of the same run.  No speed threshold is set.  One JSON line to stdout (and to --out PATH).

usage: python scripts/ilu_sweeps_bench.py [--p3 N] [--cd N] [--only a|b] [--out PATH]      (run on the GPU box, under a `timeout`)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from amg_bench import timed  # noqa: E402
from ilu_bench import REPS, TOL, _diag  # noqa: E402

SWEEPS = (2, 3, 4, 5)
RUNS = 3


def _med_spread(v):
    return float(np.median(v)), float(max(v) - min(v))


def apply_us(sa, call, n):
    """`call(in_ptr, out_ptr)` on device vectors: a warm-up, then RUNS batches of REPS asynchronous applications and one wait."""
    from sprsolve_amd import _lib
    from sprsolve_amd.device import dev_ptr
    ctx = sa.default_ctx(0)
    v = sa.DevVec.from_numpy(np.ones(n)); w = sa.DevVec.from_numpy(np.zeros(n))
    assert call(dev_ptr(v), dev_ptr(w)) == _lib.OK
    us = []
    for _ in range(RUNS):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(REPS):
            call(dev_ptr(v), dev_ptr(w))
        ctx.sync()
        us.append((time.perf_counter() - t0) / REPS * 1e6)
    return _med_spread(us)


def solve(sa, solver, P, ip, ix, d, rhs, cap):
    import scipy.sparse as sp
    n = rhs.size
    ctx = sa.default_ctx(0)
    d_rhs = sa.DevVec.from_numpy(rhs)
    ms = []
    for run in range(RUNS + 1):                              # run 0 is the warm-up
        d_x = sa.DevVec.from_numpy(np.zeros(n))
        ctx.sync()
        t0 = time.perf_counter()
        try:
            its, res = solver.precond_solve(P, d_rhs, d_x, cap, TOL) if P is not None else solver.solve(d_rhs, d_x, cap, TOL)
            status = "ok"
        except sa.error.SolverError as e:
            its, res, status = getattr(e, "iters", getattr(e, "its", -1)), float("nan"), type(e).__name__
        ctx.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    x = d_x.to_numpy()
    A = sp.csr_matrix((d, ix, ip), shape=(n, n))
    med, spread = _med_spread(ms[1:])
    return dict(status=status, iterations=int(its), rel_res=float(res), true_rel_res=float(np.linalg.norm(rhs - A @ x) / np.linalg.norm(rhs)),
                ms_to_solution=med, ms_to_solution_spread=spread, ms_first_solve=ms[0])


def workload(sa, name, make_solver, ip, ix, d, rhs, cap, with_amg):
    from sprsolve_amd import _lib
    L = _lib.lib()
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    rec = dict(n=int(n), nnz=int(ip[-1]), solver=name, tol=TOL, max_iter=cap, spmv_kernel=A.spmv_route()["kernel"], rows={})
    ilu_call = lambda h: (lambda a, b: L.sprs_ilu0_solve_dev_d(h, 0, a, b))
    plain_call = lambda fn, h: (lambda a, b: fn(h, a, b))

    def row(label, pc, create_ms, launches, call):
        r = solve(sa, make_solver(A, n), pc, ip, ix, d, rhs, cap)
        r["create_ms"] = create_ms
        r["launches_per_application"] = launches
        if call is not None:
            r["apply_us"], r["apply_us_spread"] = apply_us(sa, call, n)
        rec["rows"][label] = r
        print("%s %s: %s" % (name, label, json.dumps(r)), file=sys.stderr, flush=True)

    row("none", None, 0.0, 0, None)
    J, ms = timed(sa, lambda: sa.DiagPrecond.new(_diag(ip, ix, d)))
    row("jacobi", J, ms, 1, plain_call(L.sprs_diag_mul_vec_dev_d, J.h))
    E, ms = timed(sa, lambda: sa.ILU0.new(A))
    lv = E.levels
    rec["levels"] = dict(lower=lv["lower_levels"], upper=lv["upper_levels"])
    row("ilu0_exact", E, ms, lv["lower_launches"] + lv["upper_launches"], ilu_call(E.h))
    E.close()
    for k in SWEEPS:
        P, ms = timed(sa, lambda: sa.ILU0.new(A, sweeps=k))
        row("ilu0_sweeps_%d" % k, P, ms, 2 * k - 2, ilu_call(P.h))
        P.close()
    if with_amg:
        M, ms = timed(sa, lambda: sa.AMG.new(A))
        row("amg", M, ms, M.info["launches"], plain_call(L.sprs_amg_mul_vec_dev_d, M.h))
    return rec


def main():
    args = sys.argv[1:]
    opt = lambda k, dflt: int(args[args.index(k) + 1]) if k in args else dflt
    p3, cd = opt("--p3", 128), opt("--cd", 1024)
    only = args[args.index("--only") + 1] if "--only" in args else "ab"
    path = args[args.index("--out") + 1] if "--out" in args else None
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    sa.default_ctx(0)
    out = dict(what="no preconditioner / Jacobi / exact ILU(0) / ILU(0) with k Jacobi sweeps per triangular solve (/ AMG): f64, x0 = 0, seeded "
                    "uniform rhs, tol %g, one GPU, one process; after a warm-up solve, ms_to_solution = median of %d solves and spread = max - min; "
                    "apply_us = median and spread of %d batches of %d asynchronous applications and one wait" % (TOL, RUNS, RUNS, REPS))
    if "a" in only:
        ip, ix, d, _ = gen.poisson3d(p3, p3, p3)
        rhs = gen.uniform(7, ip.size - 1, stream=3)
        out["cg_poisson3d_%d" % p3] = workload(sa, "CG", lambda A, n: sa.CG.new(A, n), ip, ix, d, rhs, 5000, True)
    if "b" in only:
        ip, ix, d, _ = gen.convection_diffusion_2d(cd, cd)
        rhs = gen.uniform(7, ip.size - 1, stream=3)
        out["gmres30_convection_diffusion_2d_%d" % cd] = workload(sa, "GMRES(30)", lambda A, n: sa.GMRES.new(A, n, 30), ip, ix, d, rhs, 30000, False)
    line = json.dumps(out)
    print(line)
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
