"""Block-Jacobi beside no preconditioner, Jacobi and FSAI(1): one GPU, one process, one build, f64, x0 = 0, a seeded uniform
right-hand side, tol 1e-8.
  (a) gen.coupled_grid(512, 512, 3), blocks of 3 (the unknowns of a node): CG and BiCGStab.
  (b) gen.convection_diffusion_2d(1024, 1024, cx=2.0, cy=0.2), blocks of 32 (pieces of a grid line): GMRES(30) and BiCGStab.
      FSAI takes its matrix as Hermitian positive definite, which this one is not: its row records what its creation answers.
  (c) gen.poisson3d(128^3), blocks of 4 and of 32 (pieces of an x line of an isotropic operator): CG.
Per row: iterations, ms to solution (after one warm-up solve: median and spread = max - min of three, a context synchronise before
every clock read), microseconds per preconditioner application (median and spread of three batches of REPS asynchronous
applications and one wait), handle-creation ms (median and spread of three creations); for block-Jacobi also the slots of its
storage, the model bytes of one application ((slots + 2 n) * 8: the inverse with its padding, `in` and `out`) and the TB/s that
makes of apply_us, beside the same figure of the Jacobi kernel of the same run (3 n * 8 bytes).  The baseline of every figure is the
Jacobi row of the same run.  No speed threshold is set.  One JSON line to stdout (and to --out PATH, default
profiles/bjacobi_bench.json).

usage: python scripts/bjacobi_bench.py [--grid N] [--cd N] [--p3 N] [--only abc] [--out PATH]      (run on the GPU box, under a `timeout`)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from fsai_bench import created  # noqa: E402
from ilu_bench import REPS, TOL, _diag  # noqa: E402
from ilu_sweeps_bench import RUNS, apply_us, solve  # noqa: E402


def workload(sa, name, make_solver, ip, ix, d, rhs, cap, block_sizes, A=None):
    from sprsolve_amd import _lib
    L = _lib.lib()
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d) if A is None else A
    rec = dict(n=int(n), nnz=int(ip[-1]), solver=name, tol=TOL, max_iter=cap, spmv_kernel=A.spmv_route()["kernel"], stream_format=A.stream_format(), rows={})
    plain_call = lambda fn, h: (lambda a, b: fn(h, a, b))

    def row(label, pc, create, call, extra=None):
        r = solve(sa, make_solver(A, n), pc, ip, ix, d, rhs, cap)
        r["create_ms"], r["create_ms_spread"] = create
        if call is not None:
            r["apply_us"], r["apply_us_spread"] = apply_us(sa, call, n)
        r.update(extra(r) if extra else {})
        rec["rows"][label] = r
        print("%s %s: %s" % (name, label, json.dumps(r)), file=sys.stderr, flush=True)

    tbs = lambda nbytes, us: nbytes / (us * 1e-6) / 1e12
    row("none", None, (0.0, 0.0), None)
    J, ms, sp_ = created(sa, lambda: sa.DiagPrecond.new(_diag(ip, ix, d)))
    row("jacobi", J, (ms, sp_), plain_call(L.sprs_diag_mul_vec_dev_d, J.h), lambda r: dict(model_bytes=3 * n * 8, model_tb_s=tbs(3 * n * 8, r["apply_us"])))
    for bs in block_sizes:
        B, ms, sp_ = created(sa, lambda: sa.BlockJacobi.new(A, block_size=bs))
        slots = B.info["slots"]
        nbytes = (slots + 2 * n) * 8
        row("bjacobi_%d" % bs, B, (ms, sp_), plain_call(L.sprs_bjacobi_mul_vec_dev_d, B.h),
            lambda r: dict(slots=slots, padding_share=1.0 - bs * n / slots if n % bs == 0 else None, model_bytes=nbytes, model_tb_s=tbs(nbytes, r["apply_us"])))
        B.close()
    try:
        F, ms, sp_ = created(sa, lambda: sa.FSAI.new(A, power=1))
    except Exception as e:               # (whatever the creation answers is the row)
        rec["rows"]["fsai_1"] = dict(status="creation: %s: %s" % (type(e).__name__, e))
        print("%s fsai_1: %s" % (name, json.dumps(rec["rows"]["fsai_1"])), file=sys.stderr, flush=True)
    else:
        row("fsai_1", F, (ms, sp_), plain_call(L.sprs_fsai_mul_vec_dev_d, F.h), lambda r: dict(nnz_g=F.info["nnz"], max_row=F.info["max_row"]))
        F.close()
    return rec


def main():
    args = sys.argv[1:]
    opt = lambda k, dflt: int(args[args.index(k) + 1]) if k in args else dflt
    grid, cd, p3 = opt("--grid", 512), opt("--cd", 1024), opt("--p3", 128)
    only = args[args.index("--only") + 1] if "--only" in args else "abc"
    path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "bjacobi_bench.json")
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    sa.default_ctx(0)
    out = dict(what="no preconditioner / Jacobi / block-Jacobi / FSAI power 1: f64, x0 = 0, seeded uniform rhs, tol %g, one GPU, one process; after a "
                    "warm-up solve, ms_to_solution = median of %d solves and spread = max - min; apply_us = median and spread of %d batches of %d "
                    "asynchronous applications and one wait; create_ms = median and spread of %d creations; model_bytes of an application: block-Jacobi "
                    "(slots + 2 n) * 8, Jacobi 3 n * 8; model_tb_s = model_bytes / apply_us" % (TOL, RUNS, RUNS, REPS, RUNS))
    if "a" in only:
        ip, ix, d, _ = gen.coupled_grid(grid, grid, 3)
        rhs = gen.uniform(7, ip.size - 1, stream=3)
        A = sa.HipCsr.new((rhs.size, rhs.size), ip, ix, d)
        out["cg_coupled_grid_%d" % grid] = workload(sa, "CG", lambda A, n: sa.CG.new(A, n), ip, ix, d, rhs, 20000, (3,), A)
        out["bicgstab_coupled_grid_%d" % grid] = workload(sa, "BiCGStab", lambda A, n: sa.BiCGStab.new(A, n), ip, ix, d, rhs, 20000, (3,), A)
        A.close()
    if "b" in only:
        ip, ix, d, _ = gen.convection_diffusion_2d(cd, cd, cx=2.0, cy=0.2)
        rhs = gen.uniform(7, ip.size - 1, stream=3)
        A = sa.HipCsr.new((rhs.size, rhs.size), ip, ix, d)
        for name, mk in (("GMRES(30)", lambda A, n: sa.GMRES.new(A, n, 30)), ("BiCGStab", lambda A, n: sa.BiCGStab.new(A, n))):
            out["%s_convection_diffusion_%d" % (name.lower().replace("(", "").replace(")", ""), cd)] = workload(sa, name, mk, ip, ix, d, rhs, 5000, (32,), A)
        A.close()
    if "c" in only:
        ip, ix, d, _ = gen.poisson3d(p3, p3, p3)
        rhs = gen.uniform(7, p3 ** 3, stream=3)
        out["cg_poisson3d_%d" % p3] = workload(sa, "CG", lambda A, n: sa.CG.new(A, n), ip, ix, d, rhs, 5000, (4, 32))
    line = json.dumps(out)
    print(line)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
