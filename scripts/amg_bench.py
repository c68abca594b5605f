"""AMG beside ILU(0), Jacobi and no preconditioner, one GPU, one process, one build: CG on the 7-point 3-D Poisson matrix
(gen.poisson3d, 128^3 by default) with a seeded uniform right-hand side (the generator's own A.1 lies in the range of every
aggregation prolongator), f64, x0 = 0, tol 1e-8.  Per preconditioner: iterations to the tolerance, time to solution (a warm solve),
the true relative residual, microseconds per application, launches per application and the handle-creation time; for AMG also
the level sizes.  The baseline of every figure is the Jacobi solve of the same run.  No speed threshold is set.  One JSON line to
stdout (and to --out PATH).

usage: python scripts/amg_bench.py [--p3 N] [--out PATH]      (run on the GPU box, under a `timeout`)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from ilu_bench import REPS, TOL, _diag, apply_us, solve  # noqa: E402


def timed(sa, make):
    ctx = sa.default_ctx(0)
    ctx.sync()
    t0 = time.perf_counter()
    h = make()
    ctx.sync()
    return h, (time.perf_counter() - t0) * 1e3


def main():
    args = sys.argv[1:]
    p3 = int(args[args.index("--p3") + 1]) if "--p3" in args else 128
    path = args[args.index("--out") + 1] if "--out" in args else None
    import sprsolve_amd as sa
    from sprsolve_amd import _lib, gen
    sa.default_ctx(0)
    L = _lib.lib()
    ip, ix, d, _ = gen.poisson3d(p3, p3, p3)
    n = ip.size - 1
    rhs = gen.uniform(7, n, stream=3)
    A = sa.HipCsr.new((n, n), ip, ix, d)
    rec = dict(what="CG on poisson3d(%d^3), seeded uniform rhs, f64, x0 = 0, tol %g: no preconditioner / Jacobi / ILU(0) / AMG; apply_us = %d "
                    "asynchronous applications and one wait; every ratio is against the Jacobi solve of this run" % (p3, TOL, REPS),
               n=int(n), nnz=int(ip[-1]), spmv_kernel=A.spmv_route()["kernel"])
    J, rec["jacobi_create_ms"] = timed(sa, lambda: sa.DiagPrecond.new(_diag(ip, ix, d)))
    I, rec["ilu0_create_ms"] = timed(sa, lambda: sa.ILU0.new(A))
    M, rec["amg_create_ms"] = timed(sa, lambda: sa.AMG.new(A))
    inf, lv = M.info, I.levels
    rec["amg_info"] = inf
    rec["launches_per_application"] = dict(jacobi=1, ilu0=lv["lower_launches"] + lv["upper_launches"], amg=inf["launches"])
    rec["jacobi_apply_us"] = apply_us(sa, L.sprs_diag_mul_vec_dev_d, J.h, n)
    rec["ilu0_apply_us"] = apply_us(sa, L.sprs_ilu0_solve_dev_d, I.h, n)
    rec["amg_apply_us"] = apply_us(sa, L.sprs_amg_mul_vec_dev_d, M.h, n)
    for label, pc in (("none", None), ("jacobi", J), ("ilu0", I), ("amg", M)):
        rec[label] = solve(sa, sa.CG.new(A, n), pc, ip, ix, d, rhs, 5000)
    j = rec["jacobi"]
    for label in ("none", "ilu0", "amg"):
        rec[label + "_over_jacobi_iterations"] = rec[label]["iterations"] / max(j["iterations"], 1)
        rec[label + "_over_jacobi_ms_to_solution"] = rec[label]["ms_to_solution"] / j["ms_to_solution"]
    line = json.dumps(rec)
    print(line)
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
