"""BiCGStab and MINRES with the applied preconditioners beside Jacobi and no preconditioner: one GPU, one process per step, one
build, f64, x0 = 0, a seeded uniform right-hand side, tol 1e-8.  The steps (--only NAME runs one, so that a driver can put every
GPU step under its own `timeout`; each step merges its record into --out PATH):
  bicg_cd    BiCGStab on the non-symmetric 5-point operator (gen.convection_diffusion_2d, 1024 x 1024 by default):
             none / Jacobi / ILU0(sweeps=5) / AMG
  gmres_cd   GMRES(30) on the same matrix with the same preconditioners, for comparison
  bicg_p3    BiCGStab on the 7-point 3-D Poisson matrix (gen.poisson3d, 128^3 by default): none / Jacobi / ILU0(sweeps=5) / AMG;
             and for the AMG row the ms spent between convergence and the poll that notices it
  minres_p3  MINRES on the same matrix: Jacobi / AMG
Per row (scripts/ilu_sweeps_bench.py's measurement): iterations, ms to solution (after one warm-up solve: median and spread =
max - min of three, a context synchronise before every clock read), microseconds per iteration, the true relative residual,
microseconds per preconditioner application, launches per application, handle-creation ms.  The baseline of every figure is the
Jacobi solve of the same step.  No speed threshold is set: where an applied preconditioner loses in wall time the ratio says so.

ms_after_convergence: once the status word has left ST_RUNNING the solver's own kernels return at their first instruction, but
the handle's launches of the iterations already enqueued still run until the host's next poll (knob "poll", 16 iterations).  The
same solve with max_iter = iterations + 1 stops enqueueing at the iteration whose first kernel sees the convergence (one idle
iteration instead of up to 16); the difference of the two medians is what the idle applications cost.

usage: python scripts/bicg_prec_bench.py [--p3 N] [--cd N] [--only STEP] [--out PATH]      (run on the GPU box, under a `timeout`)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from amg_bench import timed  # noqa: E402
from ilu_bench import REPS, TOL, _diag  # noqa: E402
from ilu_sweeps_bench import RUNS, apply_us, solve  # noqa: E402

SWEEPS = 5
STEPS = ("bicg_cd", "gmres_cd", "bicg_p3", "minres_p3")


def workload(sa, name, make_solver, ip, ix, d, rhs, cap, labels, idle_row=None):
    from sprsolve_amd import _lib
    L = _lib.lib()
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    rec = dict(n=int(n), nnz=int(ip[-1]), solver=name, tol=TOL, max_iter=cap, spmv_kernel=A.spmv_route()["kernel"], rows={})

    def row(label, pc, create_ms, launches, call):
        s = make_solver(A, n)
        r = solve(sa, s, pc, ip, ix, d, rhs, cap)
        r["us_per_iteration"] = r["ms_to_solution"] * 1e3 / max(r["iterations"], 1)
        r["create_ms"] = create_ms
        r["launches_per_application"] = launches
        if call is not None:
            r["apply_us"], r["apply_us_spread"] = apply_us(sa, call, n)
        if label == idle_row and r["status"] == "ok":
            tight = solve(sa, s, pc, ip, ix, d, rhs, r["iterations"] + 1)
            poll = sa.default_ctx(0).get("poll")
            r["poll"] = poll
            r["ms_to_solution_max_iter_tight"] = tight["ms_to_solution"]
            r["tight_status"], r["tight_iterations"] = tight["status"], tight["iterations"]
            r["ms_after_convergence"] = r["ms_to_solution"] - tight["ms_to_solution"]
        rec["rows"][label] = r
        print("%s %s: %s" % (name, label, json.dumps(r)), file=sys.stderr, flush=True)

    if "none" in labels:
        row("none", None, 0.0, 0, None)
    J, ms = timed(sa, lambda: sa.DiagPrecond.new(_diag(ip, ix, d)))
    row("jacobi", J, ms, 1, lambda a, b: L.sprs_diag_mul_vec_dev_d(J.h, a, b))
    if "ilu0_sweeps" in labels:
        P, ms = timed(sa, lambda: sa.ILU0.new(A, sweeps=SWEEPS))
        row("ilu0_sweeps_%d" % SWEEPS, P, ms, 2 * SWEEPS - 2, lambda a, b: L.sprs_ilu0_solve_dev_d(P.h, 0, a, b))
        P.close()
    if "amg" in labels:
        M, ms = timed(sa, lambda: sa.AMG.new(A))
        rec["amg_info"] = M.info
        row("amg", M, ms, M.info["launches"], lambda a, b: L.sprs_amg_mul_vec_dev_d(M.h, a, b))
    j = rec["rows"]["jacobi"]
    for label, r in rec["rows"].items():
        r["iterations_over_jacobi"] = r["iterations"] / max(j["iterations"], 1)
        r["ms_to_solution_over_jacobi"] = r["ms_to_solution"] / j["ms_to_solution"]
    return rec


def main():
    args = sys.argv[1:]
    opt = lambda k, dflt: int(args[args.index(k) + 1]) if k in args else dflt
    p3, cd = opt("--p3", 128), opt("--cd", 1024)
    only = [args[args.index("--only") + 1]] if "--only" in args else list(STEPS)
    path = args[args.index("--out") + 1] if "--out" in args else None
    assert all(s in STEPS for s in only), only
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    sa.default_ctx(0)
    out = {}
    if path and os.path.exists(path):
        with open(path) as f:
            out = json.loads(f.read())
    out["what"] = ("BiCGStab / MINRES (and GMRES(30) for comparison) with no preconditioner / Jacobi / ILU0(sweeps=%d) / AMG: f64, x0 = 0, seeded "
                   "uniform rhs, tol %g, one GPU, one process per step; after a warm-up solve, ms_to_solution = median of %d solves and spread = "
                   "max - min; apply_us = median and spread of %d batches of %d asynchronous applications and one wait; every ratio is against "
                   "the Jacobi row of the same step" % (SWEEPS, TOL, RUNS, RUNS, REPS))
    full = ("none", "ilu0_sweeps", "amg")
    for step in only:
        if step.endswith("_cd"):
            ip, ix, d, _ = gen.convection_diffusion_2d(cd, cd)
        else:
            ip, ix, d, _ = gen.poisson3d(p3, p3, p3)
        rhs = gen.uniform(7, ip.size - 1, stream=3)
        if step == "bicg_cd":
            out["bicgstab_convection_diffusion_2d_%d" % cd] = workload(sa, "BiCGStab", lambda A, n: sa.BiCGStab.new(A, n), ip, ix, d, rhs, 30000, full)
        elif step == "gmres_cd":
            out["gmres30_convection_diffusion_2d_%d" % cd] = workload(sa, "GMRES(30)", lambda A, n: sa.GMRES.new(A, n, 30), ip, ix, d, rhs, 30000, full)
        elif step == "bicg_p3":
            out["bicgstab_poisson3d_%d" % p3] = workload(sa, "BiCGStab", lambda A, n: sa.BiCGStab.new(A, n), ip, ix, d, rhs, 5000, full, idle_row="amg")
        else:
            out["minres_poisson3d_%d" % p3] = workload(sa, "MINRES", lambda A, n: sa.MinRes.new(A, n), ip, ix, d, rhs, 5000, ("amg",))
    line = json.dumps(out)
    print(line)
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
