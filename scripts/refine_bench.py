"""Mixed-precision refinement (inner CG in f32, inner_tol 1e-2 and 1e-4) beside f64 CG: milliseconds to a TRUE relative residual of
1e-10, one GPU, one process, one build, on cfg 3 (symmetric banded, hbw 4, 1 M rows), cfg 5's operator with values="random"
and cfg 5's operator with constant coefficients (7-point 3-D Poisson, 500x500x200).  Refinement's own residual is the true one
(formed in f64 from x every outer step); CG's is its recurrence's, so the true one is formed afterwards and reported beside it.
Every solve is run once to warm up and once timed.  One JSON line to stdout.

cfg 5's values="random" operator is NOT symmetric (its generator keys an entry on row and slot): conjugate gradients, inner or
alone, do not apply to it, and the record says so (status) instead of a time.

usage: python scripts/refine_bench.py                      the measurement (run on the GPU box)
       python scripts/refine_bench.py --kernels            a short Refine and a short f64 CG solve on cfg 5, to be run under
                                                           `rocprofv3 --kernel-trace --stats -d DIR -- python scripts/refine_bench.py --kernels`
       python scripts/refine_bench.py --kernel-stats CSV   TB/s of RfResid / RfDemote / RfUpdate beside CgKB from that run's
                                                           *_kernel_stats.csv (no GPU needed)
Each GPU step of a job belongs under its own `timeout`, the steps chained with `&&`."""
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRID = (500, 500, 200)
TOL = 1e-10
# bytes per row the streaming kernels read or write at cfg 5 (no preconditioner): RfResid reads b, q and writes r in f64;
# RfDemote reads r (8) and writes rl, e (4 + 4); RfUpdate reads e (4), x (8) and writes x (8); CgKB: 6 passes of the element
BYTES = {"RfResid<": 24, "RfDemote<": 16, "RfUpdate<": 20, "CgKB<double": 48, "CgKB<float": 24}


def true_res(torch, A, rhs, x):
    y = torch.empty_like(x)
    A.mul_vec(x, y)
    return float(torch.linalg.norm(rhs - y) / torch.linalg.norm(rhs))


def timed(torch, fn, x):
    """fn() once to warm up, once timed, x zeroed before each -> (result, ms)."""
    out = None
    for _ in range(2):
        x.zero_(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return out, dt * 1e3


def measure(torch, sa, A, n, rhs, cap, max_outer):
    rec = {}
    x = torch.zeros(n, dtype=torch.float64, device=rhs.device)
    cg = sa.CG.new(A, n)

    def run_cg():
        try:
            its, res = cg.solve(rhs, x, cap, TOL)
            return dict(status="ok", iterations=its, reported_res=res)
        except sa.error.SolverError as e:
            return dict(status=type(e).__name__)
    r, ms = timed(torch, run_cg, x)
    r.update(ms_to_tol=ms, true_res=true_res(torch, A, rhs, x))
    rec["cg_f64"] = r
    del cg
    for inner_tol in (1e-2, 1e-4):
        R = sa.Refine.new(A, n)

        def run_refine():
            try:
                outer, inner, res = R.solve(rhs, x, max_outer, TOL, cap, inner_tol)
                return dict(status="ok", outer=outer, inner_iterations=inner, reported_res=res)
            except sa.error.SolverError as e:
                return dict(status=type(e).__name__, outer=R.last[0], inner_iterations=R.last[1])
        r, ms = timed(torch, run_refine, x)
        r.update(ms_to_tol=ms, true_res=true_res(torch, A, rhs, x), low_route=R.low.spmv_route())
        if r["status"] == "ok" and rec["cg_f64"]["status"] == "ok":
            r["ms_over_cg_f64"] = ms / rec["cg_f64"]["ms_to_tol"]
        rec["refine_inner_tol_%g" % inner_tol] = r
        R.close()
    return rec


def cfg5(torch, sa, dev, values="poisson"):
    from sprsolve_amd import gen_torch
    nx, ny, nz = GRID
    ip, ix, dv, rhs = gen_torch.poisson3d(nx, ny, nz, device=dev, values=values)
    n, nnz = nx * ny * nz, int(ip[-1].item())
    A = sa.HipCsr.from_device((n, n), nnz, ip, ix, dv, adopt=True)
    return A, n, nnz, rhs


def cfg5_random(torch, sa, dev):
    return cfg5(torch, sa, dev, values="random")


def cfg3(torch, sa, dev):
    from sprsolve_amd import gen
    ip, ix, d, rhs = gen.symmetric_banded(1_000_000)
    n = rhs.size
    return sa.HipCsr.new((n, n), ip, ix, d), n, int(ip[-1]), torch.from_numpy(rhs).to(dev)


def kernel_stats(path):
    """TB/s of the streaming kernels from rocprofv3's kernel stats (total time over calls per functor, all its instantiations),
    cfg 5's n."""
    n = GRID[0] * GRID[1] * GRID[2]
    acc = {}
    for row in csv.DictReader(open(path)):
        for key in BYTES:
            if key in row["Name"] and "fused_kernel" in row["Name"]:
                a = acc.setdefault(key, [0, 0.0])
                a[0] += int(row["Calls"]); a[1] += float(row["AverageNs"]) * int(row["Calls"])
    out = {}
    for key, (calls, ns) in acc.items():
        avg = ns / calls
        out[key.rstrip("<")] = dict(calls=calls, average_us=avg / 1e3, bytes_per_row=BYTES[key], TBs=BYTES[key] * n / avg / 1e3)
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
        x = torch.zeros(n, dtype=torch.float64, device=dev)
        R = sa.Refine.new(A, n)
        try:
            R.solve(rhs, x, 8, 0.0, 5, 1e-2)              # 8 outer steps of 5 inner iterations
        except sa.error.InsufficientIterNum:
            pass
        x.zero_()
        try:
            sa.CG.new(A, n).solve(rhs, x, 40, 0.0)
        except sa.error.InsufficientIterNum:
            pass
        torch.cuda.synchronize()
        print(json.dumps(dict(kernels_run=True, route=A.spmv_route(), low_route=R.low.spmv_route())))
        return
    out = dict(what="Refine (inner CG in f32) beside f64 CG, no preconditioner, one GPU, one process: ms to a true relative residual of %g "
                    "(second of two identical solves)" % TOL)
    # (iteration cap of CG and of every inner solve, max_outer): the non-symmetric operator only has to show that CG does not apply
    for name, make, cap, max_outer in (("cfg3_symmetric_banded_1M", cfg3, 2000, 60), ("cfg5_random_500x500x200", cfg5_random, 200, 3),
                                       ("cfg5_poisson3d_500x500x200", cfg5, 20000, 60)):
        A, n, nnz, rhs = make(torch, sa, dev)
        rec = dict(n=n, nnz=nnz, route=A.spmv_route())
        rec.update(measure(torch, sa, A, n, rhs, cap, max_outer))
        out[name] = rec
        del A
    print(json.dumps(out))


if __name__ == "__main__":
    main()
