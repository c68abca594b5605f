"""Multicolour-ordered ILU(0) beside the preconditioners it competes with: one GPU, one process, one build, f64, x0 = 0, a seeded
uniform right-hand side, tol 1e-8.
  (a) gen.poisson3d(128^3): CG with Jacobi, ILU0(), ILU0(sweeps=2), ILU0(order="multicolor") and FSAI(1).
  (b) gen.convection_diffusion_2d(1024, 1024): GMRES(30) and BiCGStab with Jacobi, ILU0(sweeps=5), ILU0(order="multicolor") and AMG.
Per row: iterations, ms to solution (after one warm-up solve: median and spread = max - min of three, a context synchronise before
every clock read), microseconds per preconditioner application (median and spread of three batches of REPS asynchronous
applications and one wait), handle-creation ms (median and spread of three creations); for the ILU(0) rows the levels and launches
of one application.  Per matrix: the colouring (ms, median and spread of three after a warm-up call; colours, rounds) and the
permutation P A P^T with the colour-major order (ms, the handle's stream format included) on their own — the ordered handle's creation contains both without
the handle.  No speed threshold is set.  One JSON line to stdout (and to --out PATH, default profiles/order_bench.json).

usage: python scripts/order_bench.py [--p3 N] [--cd N] [--only ab] [--out PATH]      (run on the GPU box, under a `timeout`)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from fsai_bench import created, timed  # noqa: E402
from ilu_bench import REPS, TOL, _diag  # noqa: E402
from ilu_sweeps_bench import RUNS, _med_spread, apply_us, solve  # noqa: E402


def ordering(sa, A):
    """The two primitives on their own."""
    A.color()                            # warm-up: the first call loads the kernels
    ms = []
    for _ in range(RUNS):
        (col, nc), t = timed(sa, lambda: A.color())
        ms.append(t)
    perm, ptr = sa.color_order(col)
    rec = dict(colors=int(nc), rounds=int(A.color_rounds), largest_color=int(np.diff(ptr).max()), smallest_color=int(np.diff(ptr).min()))
    rec["color_ms"], rec["color_ms_spread"] = _med_spread(ms)
    B, rec["permute_ms"], rec["permute_ms_spread"] = created(sa, lambda: A.permute(perm))
    rec["permuted_stream_format"] = B.stream_format()
    B.close()
    return rec


def workload(sa, name, make_solver, A, ip, ix, d, rhs, cap, precs):
    from sprsolve_amd import _lib
    L = _lib.lib()
    n = rhs.size
    rec = dict(n=int(n), nnz=int(ip[-1]), solver=name, tol=TOL, max_iter=cap, spmv_kernel=A.spmv_route()["kernel"], stream_format=A.stream_format(), rows={})
    ilu_call = lambda h: (lambda a, b: L.sprs_ilu0_solve_dev_d(h, 0, a, b))
    plain_call = lambda fn, h: (lambda a, b: fn(h, a, b))
    makers = {
        "jacobi": (lambda: sa.DiagPrecond.new(_diag(ip, ix, d)), lambda P: plain_call(L.sprs_diag_mul_vec_dev_d, P.h)),
        "ilu0": (lambda: sa.ILU0.new(A), lambda P: ilu_call(P.h)),
        "ilu0_sweeps_2": (lambda: sa.ILU0.new(A, sweeps=2), lambda P: ilu_call(P.h)),
        "ilu0_sweeps_5": (lambda: sa.ILU0.new(A, sweeps=5), lambda P: ilu_call(P.h)),
        "ilu0_multicolor": (lambda: sa.ILU0.new(A, order="multicolor"), lambda P: ilu_call(P.h)),
        "fsai_1": (lambda: sa.FSAI.new(A, power=1), lambda P: plain_call(L.sprs_fsai_mul_vec_dev_d, P.h)),
        "amg": (lambda: sa.AMG.new(A), lambda P: plain_call(L.sprs_amg_mul_vec_dev_d, P.h)),
    }
    for label in precs:
        make, call = makers[label]
        try:
            P, ms, sp_ = created(sa, make)
        except Exception as e:           # (whatever the creation answers is the row)
            rec["rows"][label] = dict(status="creation: %s: %s" % (type(e).__name__, e))
        else:
            r = solve(sa, make_solver(A, n), P, ip, ix, d, rhs, cap)
            r["create_ms"], r["create_ms_spread"] = ms, sp_
            r["apply_us"], r["apply_us_spread"] = apply_us(sa, call(P), n)
            if label.startswith("ilu0"):
                r.update(P.levels)
            rec["rows"][label] = r
            if hasattr(P, "close"):
                P.close()
        print("%s %s: %s" % (name, label, json.dumps(rec["rows"][label])), file=sys.stderr, flush=True)
    return rec


def main():
    args = sys.argv[1:]
    opt = lambda k, dflt: int(args[args.index(k) + 1]) if k in args else dflt
    p3, cd = opt("--p3", 128), opt("--cd", 1024)
    only = args[args.index("--only") + 1] if "--only" in args else "ab"
    path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "order_bench.json")
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    sa.default_ctx(0)
    out = dict(what="Jacobi / ILU(0) natural, by sweeps and multicolour-ordered / FSAI power 1 / AMG: f64, x0 = 0, seeded uniform rhs, tol %g, one GPU, one "
                    "process; after a warm-up solve, ms_to_solution = median of %d solves and spread = max - min; apply_us = median and spread of %d batches "
                    "of %d asynchronous applications and one wait; create_ms, color_ms, permute_ms = median and spread of %d calls" % (TOL, RUNS, RUNS, REPS, RUNS))
    if "a" in only:
        ip, ix, d, _ = gen.poisson3d(p3, p3, p3)
        rhs = gen.uniform(7, p3 ** 3, stream=3)
        A = sa.HipCsr.new((rhs.size, rhs.size), ip, ix, d)
        out["ordering_poisson3d_%d" % p3] = ordering(sa, A)
        print("ordering poisson3d: %s" % json.dumps(out["ordering_poisson3d_%d" % p3]), file=sys.stderr, flush=True)
        out["cg_poisson3d_%d" % p3] = workload(sa, "CG", lambda A, n: sa.CG.new(A, n), A, ip, ix, d, rhs, 5000,
                                               ("jacobi", "ilu0", "ilu0_sweeps_2", "ilu0_multicolor", "fsai_1"))
        A.close()
    if "b" in only:
        ip, ix, d, _ = gen.convection_diffusion_2d(cd, cd)
        rhs = gen.uniform(7, ip.size - 1, stream=3)
        A = sa.HipCsr.new((rhs.size, rhs.size), ip, ix, d)
        out["ordering_convection_diffusion_%d" % cd] = ordering(sa, A)
        print("ordering convection_diffusion: %s" % json.dumps(out["ordering_convection_diffusion_%d" % cd]), file=sys.stderr, flush=True)
        for name, mk in (("GMRES(30)", lambda A, n: sa.GMRES.new(A, n, 30)), ("BiCGStab", lambda A, n: sa.BiCGStab.new(A, n))):
            out["%s_convection_diffusion_%d" % (name.lower().replace("(", "").replace(")", ""), cd)] = workload(
                sa, name, mk, A, ip, ix, d, rhs, 5000, ("jacobi", "ilu0_sweeps_5", "ilu0_multicolor", "amg"))
        A.close()
    line = json.dumps(out)
    print(line)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
