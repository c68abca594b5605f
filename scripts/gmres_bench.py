"""GMRES(30) beside BiCGStab on two non-symmetric workloads, one GPU, one process, one build: cfg 5's operator (7-point 3-D
Poisson, 500x500x200) and cfg 2's (1000x1000 5-point grid with Dirichlet rows), each with its x-neighbours perturbed to
(1 +- 0.3) times their value — column row-1 times 1.3, column row+1 times 0.7 — which makes them non-symmetric and leaves five
resp. seven distinct (offset, value) pairs (the route the handle takes is in the output).  Per solver: steps to tol = 1e-8 (GMRES:
Arnoldi steps; BiCGStab: iterations of two SpMVs), time to that tolerance, and ms per step as a marginal rate,
(T(k2) - T(k1)) / (k2 - k1) under a capped max_iter at tol = 0 after a warm-up (bench.py's time_marginal; for GMRES(30) k1 and k2
are whole cycles, so the figure is the mean over a cycle's steps j = 0 .. 29).  One JSON line to stdout.

usage: python scripts/gmres_bench.py                      the measurement (run on the GPU box)
       python scripts/gmres_bench.py --kernels            40 steps of each solver on the cfg-5 workload, to be run under
                                                          `rocprofv3 --kernel-trace --stats -d DIR -- python scripts/gmres_bench.py --kernels`
       python scripts/gmres_bench.py --kernel-stats CSV   TB/s of GmDots / GmUpdate / GmXUpdate / BicgK5 from that run's *_kernel_stats.csv
Each GPU step of a job belongs under its own `timeout`, the steps chained with `&&`."""
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRID = (500, 500, 200)
RESTART = 30
K_LO, K_HI, WARMUP = 30, 120, 30
KERNEL_STEPS = 40            # one full cycle (j = 0 .. 29) and ten steps of the next
B = 8                        # GmDots' basis vectors per launch in f64


def _gmres_passes(steps):
    """Algorithmic vector passes (8-byte elements read or written per row) of the GMRES kernels over `steps` steps from a cycle's
    start, f64, no preconditioner -> {kernel: (launches, passes)}."""
    dots = upd = xup = 0
    nd = nu = nx = 0
    for s in range(steps):
        j = s % RESTART
        chunks = -(-(j + 1) // B)
        dots += 2 * ((j + 1) + chunks); nd += 2 * chunks                 # each launch: w + its basis vectors
        upd += 2 * ((j + 1) + 2); nu += 2                                # w in, out, the basis
        if j == RESTART - 1 or s == steps - 1:
            xup += (j + 1) + 2; nx += 1                                  # x in, out, the basis
    return {"GmDots<": (nd, dots), "GmUpdate<": (nu, upd), "GmXUpdate<": (nx, xup)}


def fixed(sa, solver, rhs, x, k):
    try:
        solver.solve(rhs, x, k, 0.0)
    except sa.error.InsufficientIterNum as e:
        assert e.iters == k
        return
    raise RuntimeError("the fixed-step solve returned early: timing would be invalid")


def measure(torch, sa, make, A, n, rhs, cap):
    s = make(A, n)
    x = torch.zeros(n, dtype=torch.float64, device=rhs.device)
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
    return dict(ms_per_step=(t[K_HI] - t[K_LO]) / (K_HI - K_LO) * 1e3, seconds_k_lo=t[K_LO], seconds_k_hi=t[K_HI],
                steps_to_tol_1e8=its, rel_res=res, status=status, ms_to_tol_1e8=dt * 1e3)


def _perturb_x(torch, ip, ix, dv):
    n = ip.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=ix.device), (ip[1:] - ip[:-1]).to(torch.int64))
    dv[ix == rows - 1] *= 1.3
    dv[ix == rows + 1] *= 0.7
    return dv


def cfg5(torch, sa, dev):
    from sprsolve_amd import gen_torch
    nx, ny, nz = GRID
    ip, ix, dv, rhs = gen_torch.poisson3d(nx, ny, nz, device=dev)
    dv = _perturb_x(torch, ip, ix, dv)
    n, nnz = nx * ny * nz, int(ip[-1].item())
    return sa.HipCsr.from_device((n, n), nnz, ip, ix, dv, adopt=True), n, nnz, rhs


def cfg2(torch, sa, dev):
    from sprsolve_amd import gen_torch
    ip, ix, dv, rhs, _ = gen_torch.grid_laplacian_dirichlet(1000, 1000, device=dev)
    dv = _perturb_x(torch, ip, ix, dv)
    n, nnz = 1000 * 1000, int(ip[-1].item())
    return sa.HipCsr.from_device((n, n), nnz, ip, ix, dv, adopt=True), n, nnz, rhs


def kernel_stats(path):
    """TB/s of the streaming kernels from rocprofv3's kernel stats (TotalDurationNs per kernel name), cfg 5's n."""
    n = GRID[0] * GRID[1] * GRID[2]
    want = {k: v[1] for k, v in _gmres_passes(KERNEL_STEPS).items()}
    want["BicgK5<"] = None                                               # 8 passes a launch (cg_bench.py)
    out = {}
    for row in csv.DictReader(open(path)):
        for key, passes in want.items():
            if key in row["Name"] and "fused_kernel" in row["Name"]:
                calls, total = int(row["Calls"]), float(row["TotalDurationNs"])
                rec = out.setdefault(key.rstrip("<"), dict(calls=0, total_us=0.0, passes=0))
                rec["calls"] += calls; rec["total_us"] += total / 1e3
                if passes is None:
                    rec["passes"] += 8 * calls                           # every instantiation of K5 in the trace counts
                else:
                    rec["passes"] = passes                               # the Gm* totals are over all their instantiations already
    for rec in out.values():
        rec["TBs"] = rec["passes"] * 8.0 * n / (rec["total_us"] * 1e3) / 1e3
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--kernel-stats":
        print(json.dumps(kernel_stats(sys.argv[2])))
        return
    import torch
    import sprsolve_amd as sa
    dev = torch.device("cuda", 0)
    sa.default_ctx(0)
    solvers = (("gmres30", lambda A, n: sa.GMRES.new(A, n, RESTART)), ("bicgstab", lambda A, n: sa.BiCGStab.new(A, n)))
    if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        A, n, nnz, rhs = cfg5(torch, sa, dev)
        for _, make in solvers:
            x = torch.zeros(n, dtype=torch.float64, device=dev)
            fixed(sa, make(A, n), rhs, x, KERNEL_STEPS)
        torch.cuda.synchronize()
        print(json.dumps(dict(kernels_run=True, steps=KERNEL_STEPS, route=A.spmv_route())))
        return
    out = dict(what="GMRES(%d) / BiCGStab, f64, no preconditioner, one GPU, one process; ms_per_step = (T(%d) - T(%d)) / %d at tol 0"
                    % (RESTART, K_HI, K_LO, K_HI - K_LO))
    for name, make_A, cap in (("cfg5_poisson3d_500x500x200_x_perturbed", cfg5, 20000), ("cfg2_poisson2d_1M_x_perturbed", cfg2, 20000)):
        A, n, nnz, rhs = make_A(torch, sa, dev)
        rec = dict(n=n, nnz=nnz, route=A.spmv_route())
        for label, make in solvers:
            rec[label] = measure(torch, sa, make, A, n, rhs, cap)
        out[name] = rec
        del A
    print(json.dumps(out))


if __name__ == "__main__":
    main()
