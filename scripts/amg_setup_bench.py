"""The AMG set-up on the device beside the set-up on the host (AMG.new(setup="device") / setup="host"), one GPU, one process, one
build, f64: poisson3d(128^3) solved by CG and convection_diffusion_2d(1024^2) solved by GMRES(30) and BiCGStab, seeded uniform
right-hand sides, x0 = 0, tol 1e-8.  Per system and per set-up: the creation time (median of REPEAT creations after a warm-up
creation, with the spread max - min; the context is synchronised before every clock read), rows, nnz and rounds per level,
microseconds per application, iterations and time to solution, and creation + solve beside Jacobi and FSAI(1) on the same system.
For the device set-up also the per-stage breakdown (AMG.setup_ms, medians of REPEAT further creations under SPRS_CREATE_TRACE,
which drains the stream at every stage boundary: the creation times above are taken without it).  The baseline is the host set-up of the same run.
The verdict line says whether the device set-up is faster than the host set-up by more than the two spreads together.
One JSON line to stdout and to --out PATH (default profiles/amg_setup_bench.json).

usage: python scripts/amg_setup_bench.py [--p3 N] [--cd N] [--out PATH]      (run on the GPU box, under a `timeout`)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from ilu_bench import REPS, TOL, _diag, apply_us, solve  # noqa: E402

REPEAT = 3


def timed(sa, make):
    ctx = sa.default_ctx(0)
    ctx.sync()
    t0 = time.perf_counter()
    h = make()
    ctx.sync()
    return h, (time.perf_counter() - t0) * 1e3


def creation(sa, make):
    """-> (handle of the last creation, median ms, spread ms, all ms)."""
    h, _ = timed(sa, make)                                   # warm-up: code objects, allocator, rocprim's first launches
    h.close()
    ms = []
    for r in range(REPEAT):
        h, t = timed(sa, make)
        ms.append(t)
        if r + 1 < REPEAT:
            h.close()
    return h, float(np.median(ms)), float(max(ms) - min(ms)), ms


def stage_ms(sa, make):
    """Medians of the device set-up's stage clock over REPEAT creations with the clock on, and the median of their totals."""
    os.environ["SPRS_CREATE_TRACE"] = "1"
    try:
        runs = []
        for _ in range(REPEAT):
            h, _t = timed(sa, make)
            runs.append(h.setup_ms)
            h.close()
    finally:
        del os.environ["SPRS_CREATE_TRACE"]
    return {k: float(np.median([s[k] for s in runs])) for k in sa.AMG.STAGES}, float(np.median([sum(s.values()) for s in runs]))


def one_system(sa, L, label, ip, ix, d, rhs, solvers):
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    rec = dict(n=int(n), nnz=int(ip[-1]))
    pcs = {}
    for how in ("host", "device"):
        M, med, spread, ms = creation(sa, lambda: sa.AMG.new(A, setup=how))
        inf = M.info
        rec["amg_" + how] = dict(create_ms=med, create_spread_ms=spread, create_all_ms=ms, rows=inf["rows"], nnz=inf["nnz"], rounds=inf["rounds"],
                                 levels=inf["levels"], launches=inf["launches"], operator_complexity=sum(inf["nnz"]) / inf["nnz"][0],
                                 apply_us=apply_us(sa, L.sprs_amg_mul_vec_dev_d, M.h, n))
        if how == "device":
            rec["amg_device"]["stage_ms"], rec["amg_device"]["create_ms_with_stage_clock"] = stage_ms(sa, lambda: sa.AMG.new(A, setup="device"))
        pcs["amg_" + how] = M
    pcs["jacobi"], med, spread, _ = creation(sa, lambda: sa.DiagPrecond.new(_diag(ip, ix, d)))
    rec["jacobi"] = dict(create_ms=med, create_spread_ms=spread)
    pcs["fsai1"], med, spread, _ = creation(sa, lambda: sa.FSAI.new(A, 1))
    rec["fsai1"] = dict(create_ms=med, create_spread_ms=spread)
    for sname, mk in solvers:
        out = {}
        for pname, pc in pcs.items():
            s = solve(sa, mk(A, n), pc, ip, ix, d, rhs, 20000)
            s["create_plus_solve_ms"] = rec[pname]["create_ms"] + s["ms_to_solution"]
            out[pname] = s
        rec[sname] = out
    h, v = rec["amg_host"], rec["amg_device"]
    gain = h["create_ms"] - v["create_ms"]
    rec["verdict"] = dict(host_ms=h["create_ms"], device_ms=v["create_ms"], gain_ms=gain, spreads_together_ms=h["create_spread_ms"] + v["create_spread_ms"],
                          device_faster_by_more_than_the_spreads=bool(gain > h["create_spread_ms"] + v["create_spread_ms"]),
                          dominant_device_stage=max(v["stage_ms"], key=v["stage_ms"].get))
    for pc in pcs.values():
        pc.close()
    A.close()
    return rec


def main():
    args = sys.argv[1:]
    p3 = int(args[args.index("--p3") + 1]) if "--p3" in args else 128
    cd = int(args[args.index("--cd") + 1]) if "--cd" in args else 1024
    path = args[args.index("--out") + 1] if "--out" in args else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "amg_setup_bench.json")
    import sprsolve_amd as sa
    from sprsolve_amd import _lib, gen
    sa.default_ctx(0)
    L = _lib.lib()
    rec = dict(what="AMG.new(setup=host) against AMG.new(setup=device, seed=0), f64, defaults otherwise; creation ms = median of %d after a warm-up "
                    "creation, spread = max - min; solves: seeded uniform rhs, x0 = 0, tol %g, ms_to_solution = the warm solve; apply_us = %d "
                    "asynchronous applications and one wait; the baseline is the host set-up of this run" % (REPEAT, TOL, REPS))
    ip, ix, d, _ = gen.poisson3d(p3, p3, p3)
    rec["poisson3d_%d" % p3] = one_system(sa, L, "p3", ip, ix, d, gen.uniform(7, ip.size - 1, stream=3), [("cg", lambda A, n: sa.CG.new(A, n))])
    ip, ix, d, _ = gen.convection_diffusion_2d(cd, cd)
    rec["convection_diffusion_2d_%d" % cd] = one_system(sa, L, "cd", ip, ix, d, gen.uniform(7, ip.size - 1, stream=3),
                                                        [("gmres30", lambda A, n: sa.GMRES.new(A, n, 30)), ("bicgstab", lambda A, n: sa.BiCGStab.new(A, n))])
    line = json.dumps(rec)
    print(line)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
