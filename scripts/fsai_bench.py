"""FSAI (power 1 and 2) beside no preconditioner, Jacobi, ILU(0) with two Jacobi sweeps per triangular solve and AMG: one GPU,
one process, one build, f64, x0 = 0, a seeded uniform right-hand side, tol 1e-8.
  (a) CG on the 7-point 3-D Poisson matrix (gen.poisson3d, 128^3 by default): scripts/amg_bench.py's system.
  (b) BiCGStab on the same system.
  (c) CG on a variable-coefficient symmetric matrix with the same pattern: gen.poisson3d(values="random"), its strict lower triangle
      mirrored, the diagonal 1 + the sum of the row's |off-diagonals| (strictly dominant, so positive definite).
Per row: iterations, ms to solution (after one warm-up solve: median and spread = max - min of three, a context synchronise before
every clock read), microseconds per preconditioner application (median and spread of three batches of REPS asynchronous
applications and one wait), launches per application, handle-creation ms (median and spread of three creations), and for FSAI
nnz(G), its longest row and sprs_csr_stream_format of G and GH together with the SpMV kernel each takes.  The baseline of every
figure is the Jacobi row of the same run.  No speed threshold is set.  One JSON line to stdout (and to --out PATH, default
profiles/fsai_bench.json).

usage: python scripts/fsai_bench.py [--p3 N] [--only abc] [--out PATH]      (run on the GPU box, under a `timeout`)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from amg_bench import timed  # noqa: E402
from ilu_bench import REPS, TOL, _diag  # noqa: E402
from ilu_sweeps_bench import RUNS, _med_spread, apply_us, solve  # noqa: E402


def created(sa, make):
    """-> (handle, median ms, spread ms) of RUNS creations; the last handle is kept."""
    ms = []
    h = None
    for _ in range(RUNS):
        if h is not None:
            h.close()
        h, t = timed(sa, make)
        ms.append(t)
    return (h,) + _med_spread(ms)


def symmetric_random(gen, p3):
    import scipy.sparse as sp
    ip, ix, d, _ = gen.poisson3d(p3, p3, p3, values="random")
    n = ip.size - 1
    L = sp.tril(sp.csr_matrix((d, ix, ip), shape=(n, n)), -1)
    S = (L + L.T).tocsr()
    S = (S + sp.diags(1.0 + np.asarray(abs(S).sum(axis=1)).ravel())).tocsr()
    S.sort_indices()
    return S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data


def workload(sa, name, make_solver, ip, ix, d, rhs, cap):
    from sprsolve_amd import _lib
    L = _lib.lib()
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    rec = dict(n=int(n), nnz=int(ip[-1]), solver=name, tol=TOL, max_iter=cap, spmv_kernel=A.spmv_route()["kernel"], stream_format=A.stream_format(), rows={})
    plain_call = lambda fn, h: (lambda a, b: fn(h, a, b))

    def row(label, pc, create, launches, call, extra=None):
        r = solve(sa, make_solver(A, n), pc, ip, ix, d, rhs, cap)
        r["create_ms"], r["create_ms_spread"] = create
        r["launches_per_application"] = launches
        if call is not None:
            r["apply_us"], r["apply_us_spread"] = apply_us(sa, call, n)
        r.update(extra or {})
        rec["rows"][label] = r
        print("%s %s: %s" % (name, label, json.dumps(r)), file=sys.stderr, flush=True)

    row("none", None, (0.0, 0.0), 0, None)
    J, ms, sp_ = created(sa, lambda: sa.DiagPrecond.new(_diag(ip, ix, d)))
    row("jacobi", J, (ms, sp_), 1, plain_call(L.sprs_diag_mul_vec_dev_d, J.h))
    P, ms, sp_ = created(sa, lambda: sa.ILU0.new(A, sweeps=2))
    row("ilu0_sweeps_2", P, (ms, sp_), 2, lambda a, b: L.sprs_ilu0_solve_dev_d(P.h, 0, a, b))
    P.close()
    M, ms, sp_ = created(sa, lambda: sa.AMG.new(A))
    row("amg", M, (ms, sp_), M.info["launches"], plain_call(L.sprs_amg_mul_vec_dev_d, M.h))
    M.close()
    for power in (1, 2):
        F, ms, sp_ = created(sa, lambda: sa.FSAI.new(A, power=power))
        G, GH = F.G, F.GH
        inf = F.info
        extra = dict(nnz_g=inf["nnz"], max_row=inf["max_row"], g_stream_format=G.stream_format(), gh_stream_format=GH.stream_format(),
                     g_spmv_kernel=G.spmv_route()["kernel"], gh_spmv_kernel=GH.spmv_route()["kernel"])
        row("fsai_%d" % power, F, (ms, sp_), 2, plain_call(L.sprs_fsai_mul_vec_dev_d, F.h), extra)
        F.close()
    return rec


def main():
    args = sys.argv[1:]
    p3 = int(args[args.index("--p3") + 1]) if "--p3" in args else 128
    only = args[args.index("--only") + 1] if "--only" in args else "abc"
    path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "fsai_bench.json")
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    sa.default_ctx(0)
    out = dict(what="no preconditioner / Jacobi / ILU(0) with 2 Jacobi sweeps per triangular solve / AMG / FSAI power 1 and 2: f64, x0 = 0, seeded "
                    "uniform rhs, tol %g, one GPU, one process; after a warm-up solve, ms_to_solution = median of %d solves and spread = max - min; "
                    "apply_us = median and spread of %d batches of %d asynchronous applications and one wait; create_ms = median and spread of %d "
                    "creations; stream formats as sprs_csr_stream_format: (mode, offsets, pairs), mode 0 plain CSR, 1 offset codes, 2 pair codes"
                    % (TOL, RUNS, RUNS, REPS, RUNS))
    rhs = gen.uniform(7, p3 ** 3, stream=3)
    if "a" in only or "b" in only:
        ip, ix, d, _ = gen.poisson3d(p3, p3, p3)
        if "a" in only:
            out["cg_poisson3d_%d" % p3] = workload(sa, "CG", lambda A, n: sa.CG.new(A, n), ip, ix, d, rhs, 5000)
        if "b" in only:
            out["bicgstab_poisson3d_%d" % p3] = workload(sa, "BiCGStab", lambda A, n: sa.BiCGStab.new(A, n), ip, ix, d, rhs, 5000)
    if "c" in only:
        ip, ix, d = symmetric_random(gen, p3)
        out["cg_variable_coefficients_%d" % p3] = workload(sa, "CG", lambda A, n: sa.CG.new(A, n), ip, ix, d, rhs, 5000)
    line = json.dumps(out)
    print(line)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
