"""ILU(0) beside Jacobi and no preconditioner, one GPU, one process, one build: CG on the 7-point 3-D Poisson matrix
(gen.poisson3d, 128^3 by default) and GMRES(30) on the non-symmetric 5-point operator (gen.convection_diffusion_2d, 512 x 512 by
default), f64, x0 = 0, tol 1e-8.  Per (solver, preconditioner): iterations to the tolerance, time to solution (a warm solve: the
same solve was run once before), the true relative residual; per preconditioner: microseconds per application (REPS asynchronous
applications on device vectors, one wait); for ILU(0): levels and launches of the lower and the upper solve and the handle-creation
time.  The baseline of every ILU(0) figure is the Jacobi solve of the same run.  One JSON line to stdout (and to --out PATH).

usage: python scripts/ilu_bench.py [--p3 N] [--cd N] [--out PATH]      (run on the GPU box, under a `timeout`)"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

TOL, REPS = 1e-8, 20


def _diag(ip, ix, d):
    return d[np.repeat(np.arange(ip.size - 1), np.diff(ip)) == ix]


def apply_us(sa, fn, handle, n):
    from sprsolve_amd import _lib
    from sprsolve_amd.device import dev_ptr
    ctx = sa.default_ctx(0)
    v = sa.DevVec.from_numpy(np.ones(n)); w = sa.DevVec.from_numpy(np.zeros(n))
    call = (lambda: fn(handle, 0, dev_ptr(v), dev_ptr(w))) if fn.__name__.startswith("sprs_ilu0") else (lambda: fn(handle, dev_ptr(v), dev_ptr(w)))
    assert call() == _lib.OK
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(REPS):
        call()
    ctx.sync()
    return (time.perf_counter() - t0) / REPS * 1e6


def solve(sa, solver, P, ip, ix, d, rhs, cap):
    import scipy.sparse as sp
    n = rhs.size
    ctx = sa.default_ctx(0)
    d_rhs = sa.DevVec.from_numpy(rhs)
    out = {}
    for label in ("cold", "warm"):
        d_x = sa.DevVec.from_numpy(np.zeros(n))
        ctx.sync()
        t0 = time.perf_counter()
        try:
            its, res = solver.precond_solve(P, d_rhs, d_x, cap, TOL) if P is not None else solver.solve(d_rhs, d_x, cap, TOL)
            status = "ok"
        except sa.error.SolverError as e:
            its, res, status = getattr(e, "iters", getattr(e, "its", -1)), float("nan"), type(e).__name__
        ctx.sync()
        out[label] = time.perf_counter() - t0
    x = d_x.to_numpy()
    A = sp.csr_matrix((d, ix, ip), shape=(n, n))
    return dict(status=status, iterations=int(its), rel_res=float(res), true_rel_res=float(np.linalg.norm(rhs - A @ x) / np.linalg.norm(rhs)),
                ms_to_solution=out["warm"] * 1e3, ms_first_solve=out["cold"] * 1e3)


def workload(sa, name, make_solver, ip, ix, d, rhs, cap):
    from sprsolve_amd import _lib
    n = rhs.size
    L = _lib.lib()
    A = sa.HipCsr.new((n, n), ip, ix, d)
    rec = dict(n=int(n), nnz=int(ip[-1]), solver=name, tol=TOL, max_iter=cap, spmv_kernel=A.spmv_route()["kernel"])
    J = sa.DiagPrecond.new(_diag(ip, ix, d))
    sa.default_ctx(0).sync()
    t0 = time.perf_counter()
    P = sa.ILU0.new(A)
    sa.default_ctx(0).sync()
    rec["ilu0_create_ms"] = (time.perf_counter() - t0) * 1e3
    rec["ilu0_levels"] = P.levels
    rec["jacobi_apply_us"] = apply_us(sa, L.sprs_diag_mul_vec_dev_d, J.h, n)
    rec["ilu0_apply_us"] = apply_us(sa, L.sprs_ilu0_solve_dev_d, P.h, n)
    for label, pc in (("none", None), ("jacobi", J), ("ilu0", P)):
        rec[label] = solve(sa, make_solver(A, n), pc, ip, ix, d, rhs, cap)
    j, i = rec["jacobi"], rec["ilu0"]
    rec["ilu0_over_jacobi_iterations"] = i["iterations"] / max(j["iterations"], 1)
    rec["ilu0_over_jacobi_ms_to_solution"] = i["ms_to_solution"] / j["ms_to_solution"]
    return rec


def main():
    args = sys.argv[1:]
    opt = lambda k, dflt: int(args[args.index(k) + 1]) if k in args else dflt
    p3, cd = opt("--p3", 128), opt("--cd", 512)
    path = args[args.index("--out") + 1] if "--out" in args else None
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    sa.default_ctx(0)
    out = dict(what="no preconditioner / Jacobi / ILU(0): iterations and wall time to tol %g, f64, x0 = 0, one GPU, one process; "
                    "apply_us = %d asynchronous applications and one wait" % (TOL, REPS))
    ip, ix, d, rhs = gen.poisson3d(p3, p3, p3)
    out["cg_poisson3d_%d" % p3] = workload(sa, "CG", lambda A, n: sa.CG.new(A, n), ip, ix, d, rhs, 5000)
    ip, ix, d, rhs = gen.convection_diffusion_2d(cd, cd)
    out["gmres30_convection_diffusion_2d_%d" % cd] = workload(sa, "GMRES(30)", lambda A, n: sa.GMRES.new(A, n, 30), ip, ix, d, rhs, 20000)
    line = json.dumps(out)
    print(line)
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
