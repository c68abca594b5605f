"""LSMR on a 1 M x 0.5 M operator of the LSMR tests' kind (row i has 1 + (i mod 5) entries, one of them at column i mod n with
4 added), f64, one GPU, one process, one build: ms per iteration as a marginal rate, (T(k2) - T(k1)) / (k2 - k1) under a capped
max_iter at tol = 0 after a warm-up, fused against literal; iterations and time to tol = 1e-8.  One JSON line to stdout.

usage: python scripts/lsmr_bench.py                      the measurement (run on the GPU box)
       python scripts/lsmr_bench.py --kernels            a short fused LSMR solve, and a short CG solve on the 1 M-row symmetric
                                                         banded system for CgKB, to be run under
                                                         `rocprofv3 --kernel-trace --stats -d DIR -- python scripts/lsmr_bench.py --kernels`
                                                         (tracing only: no counters in that run)
       python scripts/lsmr_bench.py --kernel-stats CSV   TB/s of LsKU / LsKV / LsKH / CgKB from that run's *_kernel_stats.csv (no GPU needed)
Each GPU step of a job belongs under its own `timeout`, the steps chained with `&&`."""
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M, N = 1_000_000, 500_000
N_CG = 1_000_000
K_LO, K_HI, WARMUP = 20, 120, 10
# (vector passes, vector length): 8-byte elements read or written per row
PASSES = {"LsKU<": (3, M), "LsKV<": (3, N), "LsKH<": (8, N), "CgKB<": (6, N_CG)}


def system(m, n, seed=0):
    """tests/_lsmr_ref.system's rule, vectorised; a consistent rhs."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    cnt = 1 + np.arange(m) % 5
    ip = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    nnz = int(ip[-1])
    ix = rng.integers(0, n, nnz).astype(np.int32)
    d = rng.uniform(-1, 1, nnz)
    ix[ip[:-1]] = np.arange(m) % n
    d[ip[:-1]] += 4.0
    A = sp.csr_matrix((d, ix, ip), shape=(m, n))
    A.sort_indices()                                     # duplicates of a column stay apart
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, A @ rng.uniform(-1, 1, n)


def fixed(sa, solver, rhs, x, k):
    try:
        solver.solve(rhs, x, k, 0.0)
    except sa.error.InsufficientIterNum as e:
        assert e.iters == k
        return
    raise RuntimeError("the fixed-iteration solve returned early: timing would be invalid")


def measure(sa, A, AH, rhs, mode):
    s = sa.LSMR.new(A, AH)
    s.set_mode(mode)
    x = sa.DevVec(N, np.float64)
    x.zero(); fixed(sa, s, rhs, x, WARMUP)
    t = {}
    for k in (K_LO, K_HI):
        x.zero(); A.ctx.sync()
        t0 = time.perf_counter()
        fixed(sa, s, rhs, x, k)
        A.ctx.sync()
        t[k] = time.perf_counter() - t0
    x.zero(); A.ctx.sync()
    t0 = time.perf_counter()
    try:
        its, res, ares = s.solve(rhs, x, 2000, 1e-8)
        status = "ok"
    except sa.error.SolverError as e:
        its, res, ares, status = 2000, float("nan"), float("nan"), type(e).__name__
    A.ctx.sync()
    dt = time.perf_counter() - t0
    return dict(ms_per_iteration=(t[K_HI] - t[K_LO]) / (K_HI - K_LO) * 1e3, seconds_k_lo=t[K_LO], seconds_k_hi=t[K_HI],
                iterations_to_tol_1e8=its, res=res, ares=ares, status=status, ms_to_tol_1e8=dt * 1e3)


def kernel_stats(path):
    """TB/s of the streaming kernels from rocprofv3's kernel stats (AverageNs per kernel name)."""
    out = {}
    for row in csv.DictReader(open(path)):
        for key, (passes, length) in PASSES.items():
            if key in row["Name"] and "fused_kernel" in row["Name"]:
                ns = float(row["AverageNs"])
                out[key.rstrip("<")] = dict(kernel=row["Name"][:120], calls=int(row["Calls"]), average_us=ns / 1e3, passes=passes,
                                            length=length, TBs=passes * 8.0 * length / ns / 1e3)
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--kernel-stats":
        print(json.dumps(kernel_stats(sys.argv[2])))
        return
    import sprsolve_amd as sa
    sa.default_ctx(0)
    ip, ix, d, b = system(M, N)
    A = sa.HipCsr.new((M, N), ip, ix, d)
    t0 = time.perf_counter()
    AH = A.adjoint()
    adjoint_ms = (time.perf_counter() - t0) * 1e3
    rhs = sa.DevVec.from_numpy(b)
    if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        x = sa.DevVec(N, np.float64); x.zero()
        fixed(sa, sa.LSMR.new(A, AH), rhs, x, 40)
        from sprsolve_amd import gen
        cp, cx, cd, crhs = gen.symmetric_banded(N_CG)
        C = sa.HipCsr.new((N_CG, N_CG), cp, cx, cd)
        xc = np.zeros(N_CG)
        try:
            sa.CG.new(C, N_CG).solve(crhs, xc, 40, 0.0)
        except sa.error.InsufficientIterNum:
            pass
        print(json.dumps(dict(kernels_run=True, route=A.spmv_route(), adjoint_route=AH.spmv_route())))
        return
    out = dict(what="LSMR, f64, %d x %d, one GPU, one process; ms_per_iteration = (T(%d) - T(%d)) / %d at tol 0" % (M, N, K_HI, K_LO, K_HI - K_LO),
               nnz=int(ip[-1]), route=A.spmv_route(), adjoint_route=AH.spmv_route(), adjoint_build_ms=adjoint_ms)
    for mode in ("fused", "literal"):
        out[mode] = measure(sa, A, AH, rhs, mode)
    out["literal_over_fused_ms_per_iteration"] = out["literal"]["ms_per_iteration"] / out["fused"]["ms_per_iteration"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
