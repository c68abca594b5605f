"""CG beside BiCGStab and MINRES on the two Hermitian positive-definite BASELINE workloads, one GPU, one process, one build:
cfg 5 (7-point 3-D Poisson, 500x500x200, the stream the library picks) and cfg 3 (symmetric banded, hbw 4, 1 M rows).
Per solver: iterations to tol = 1e-8, time to that tolerance, and ms per iteration as a marginal rate, (T(k2) - T(k1)) / (k2 - k1)
under a capped max_iter at tol = 0 after a warm-up (bench.py's time_marginal).  One JSON line to stdout.

usage: python scripts/cg_bench.py                      the measurement (run on the GPU box)
       python scripts/cg_bench.py --kernels            a short CG and a short BiCGStab solve on cfg 5, to be run under
                                                       `rocprofv3 --kernel-trace --stats -d DIR -- python scripts/cg_bench.py --kernels`
       python scripts/cg_bench.py --kernel-stats CSV   TB/s of CgKB / CgKC / BicgK5 from that run's *_kernel_stats.csv (no GPU needed)
Each GPU step of a job belongs under its own `timeout`, the steps chained with `&&`."""
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRID = (500, 500, 200)
K_LO, K_HI, WARMUP = 20, 120, 10
# vector passes (8-byte elements read or written per row) of the streaming kernels at cfg 5: f64, no preconditioner, chain route
PASSES = {"CgKB<": 6, "CgKC<": 3, "BicgK5<": 8}     # K5 with s formed again from r and v: reads x, y, r, t, r0, v, writes x, r


def fixed(sa, solver, rhs, x, k):
    try:
        solver.solve(rhs, x, k, 0.0)
    except sa.error.InsufficientIterNum as e:
        assert e.iters == k
        return
    raise RuntimeError("the fixed-iteration solve returned early: timing would be invalid")


def measure(torch, sa, cls, A, n, rhs, dtype, cap):
    s = cls.new(A, n)
    x = torch.zeros(n, dtype=dtype, device=rhs.device)
    fixed(sa, s, rhs, x, WARMUP)
    t = {}
    for k in (K_LO, K_HI):
        x.zero_(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        fixed(sa, s, rhs, x, k)
        torch.cuda.synchronize()
        t[k] = time.perf_counter() - t0
    x.zero_(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        its, res = s.solve(rhs, x, cap, 1e-8)
        status = "ok"
    except sa.error.SolverError as e:
        its, res, status = cap, float("nan"), type(e).__name__
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(ms_per_iteration=(t[K_HI] - t[K_LO]) / (K_HI - K_LO) * 1e3, seconds_k_lo=t[K_LO], seconds_k_hi=t[K_HI],
                iterations_to_tol_1e8=its, rel_res=res, status=status, ms_to_tol_1e8=dt * 1e3)


def cfg5(torch, sa, dev):
    from sprsolve_amd import gen_torch
    nx, ny, nz = GRID
    ip, ix, dv, rhs = gen_torch.poisson3d(nx, ny, nz, device=dev)
    n, nnz = nx * ny * nz, int(ip[-1].item())
    A = sa.HipCsr.from_device((n, n), nnz, ip, ix, dv, adopt=True)
    return A, n, nnz, rhs


def cfg3(torch, sa, dev):
    from sprsolve_amd import gen
    ip, ix, d, rhs = gen.symmetric_banded(1_000_000)
    n = rhs.size
    return sa.HipCsr.new((n, n), ip, ix, d), n, int(ip[-1]), torch.from_numpy(rhs).to(dev)


def kernel_stats(path):
    """TB/s of the streaming kernels from rocprofv3's kernel stats (AverageNs per kernel name), cfg 5's n."""
    n = GRID[0] * GRID[1] * GRID[2]
    out = {}
    for row in csv.DictReader(open(path)):
        for key, passes in PASSES.items():
            if key in row["Name"] and "fused_kernel" in row["Name"]:
                ns = float(row["AverageNs"])
                out[key.rstrip("<")] = dict(kernel=row["Name"][:120], calls=int(row["Calls"]), average_us=ns / 1e3, passes=passes,
                                            TBs=passes * 8.0 * n / ns / 1e3)
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--kernel-stats":
        print(json.dumps(kernel_stats(sys.argv[2])))
        return
    import torch
    import sprsolve_amd as sa
    dev = torch.device("cuda", 0)
    sa.default_ctx(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        A, n, nnz, rhs = cfg5(torch, sa, dev)
        for cls in (sa.CG, sa.BiCGStab):
            x = torch.zeros(n, dtype=torch.float64, device=dev)
            fixed(sa, cls.new(A, n), rhs, x, 40)
        torch.cuda.synchronize()
        print(json.dumps(dict(kernels_run=True, route=A.spmv_route())))
        return
    out = dict(what="CG / BiCGStab / MINRES, f64, no preconditioner, one GPU, one process; ms_per_iteration = (T(%d) - T(%d)) / %d at tol 0"
                    % (K_HI, K_LO, K_HI - K_LO))
    for name, make, cap in (("cfg5_poisson3d_500x500x200", cfg5, 20000), ("cfg3_symmetric_banded_1M", cfg3, 2000)):
        A, n, nnz, rhs = make(torch, sa, dev)
        rec = dict(n=n, nnz=nnz, route=A.spmv_route())
        for label, cls in (("cg", sa.CG), ("bicgstab", sa.BiCGStab), ("minres", sa.MinRes)):
            rec[label] = measure(torch, sa, cls, A, n, rhs, torch.float64, cap)
        rec["cg_over_bicgstab_ms_per_iteration"] = rec["cg"]["ms_per_iteration"] / rec["bicgstab"]["ms_per_iteration"]
        out[name] = rec
        del A
    print(json.dumps(out))


if __name__ == "__main__":
    main()
