"""Batched CG (sprs_cgmany_solve_dev) beside k sequential sprs_cg_solve_dev calls, f64, no preconditioner, one GPU, one process,
one build: marginal ms per iteration per right-hand side, (T(K_HI) - T(K_LO)) / (K_HI - K_LO) / k at tol 0 after a warm-up, for
k in {1, 2, 4, 8}.  The sequential side is the single-solve code, which this feature leaves untouched.

Operators: cfg 2's (1000 x 1000 5-point grid, Dirichlet rows) and cfg 5's (500 x 500 x 200 7-point Poisson; skipped when 5 blocks of
n x 8 doubles do not fit) with the plain CSR stream forced ("spmv_dict" 0) for the sequential side — the SpMM always reads the plain
arrays, and a plain stream moves the same bytes whatever the values are, so the operators keep their own (positive definite) values
where the issue's random ones would end CG in BreakDown; and cfg 3's (symmetric banded, n = 1e6) on the route it takes by itself.
One JSON line to stdout (kept as profiles/cg_many_bench.json).

usage: python scripts/cg_many_bench.py                      the measurement
       python scripts/cg_many_bench.py --kernels            40 iterations of both at k = 8 on cfg 3, to be run under
                                                            `rocprofv3 --kernel-trace --stats -d DIR -- python scripts/cg_many_bench.py --kernels`
       python scripts/cg_many_bench.py --kernel-stats CSV   TB/s of spmm_kernel / CgManyKB / CgManyKC beside CgKB from that run's stats
Each GPU step of a job belongs under its own `timeout`, the steps chained with `&&`."""
import csv
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (1, 2, 4, 8)
K_LO, K_HI, WARMUP = 20, 80, 10
KERNEL_STEPS = 40
N3 = 1000000


def _cfg2(torch, sa, dev):
    from sprsolve_amd import gen_torch
    ip, ix, dv, rhs, _ = gen_torch.grid_laplacian_dirichlet(1000, 1000, device=dev)
    n = 1000 * 1000
    return sa.HipCsr.from_device((n, n), int(ip[-1].item()), ip, ix, dv, adopt=True), n, 0


def _cfg3(torch, sa, dev):
    from sprsolve_amd import gen
    ip, ix, d, _ = gen.symmetric_banded(N3)
    return sa.HipCsr.new((N3, N3), ip, ix, d), N3, -1


def _cfg5(torch, sa, dev):
    from sprsolve_amd import gen_torch
    nx, ny, nz = 500, 500, 200
    n = nx * ny * nz
    free, _ = torch.cuda.mem_get_info()
    if free < 5 * n * 8 * 8 + n * 100 + (4 << 30):
        return None, n, 0
    ip, ix, dv, rhs = gen_torch.poisson3d(nx, ny, nz, device=dev)
    return sa.HipCsr.from_device((n, n), int(ip[-1].item()), ip, ix, dv, adopt=True), n, 0


def _columns(torch, n, k, dev):
    g = torch.Generator(device="cpu"); g.manual_seed(1234)
    return (torch.rand((n, k), generator=g, dtype=torch.float64) * 2 - 1).to(dev)


def _run_many(s, B, X, its):
    X.zero_()
    _, _, st = s.solve(B.reshape(-1), X.reshape(-1), its, 0.0)
    assert all(int(v) == 3 for v in st), st                      # every column still running: the timing is of `its` iterations


def _run_seq(sa, s, cols, xs, its):
    for b, x in zip(cols, xs):
        x.zero_()
        try:
            s.solve(b, x, its, 0.0)
        except sa.error.InsufficientIterNum:
            continue
        raise RuntimeError("the fixed-step solve returned early: timing would be invalid")


def _marginal(torch, run):
    run(WARMUP)
    t = {}
    for its in (K_LO, K_HI):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(its)
        torch.cuda.synchronize()
        t[its] = time.perf_counter() - t0
    return (t[K_HI] - t[K_LO]) / (K_HI - K_LO) * 1e3


def kernel_stats(path):
    """TB/s from rocprofv3's kernel stats; passes of n x 8 f64 blocks per launch: CgManyKB 6, CgManyKC 3, CgKB 6 vectors, and the
    SpMM's algorithmic bytes (12 B per entry, 4 per row, two blocks)."""
    from sprsolve_amd import gen
    nnz = int(gen.symmetric_banded(1000)[0][-1]) * (N3 // 1000)          # 9 entries a row but for the band's ends
    per = {"CgManyKB": 6 * 8 * 8.0 * N3, "CgManyKC": 3 * 8 * 8.0 * N3, "CgKB": 6 * 8.0 * N3, "spmm_kernel": 12.0 * nnz + 4.0 * N3 + 2 * 8 * 8.0 * N3}
    out = {}
    for row in csv.DictReader(open(path)):
        for key, b in per.items():
            if key + "I" in row["Name"] or key + "<" in row["Name"]:
                rec = out.setdefault(key, dict(calls=0, total_us=0.0))
                rec["calls"] += int(row["Calls"]); rec["total_us"] += float(row["TotalDurationNs"]) / 1e3
    for key, rec in out.items():
        rec["TBs"] = per[key] * rec["calls"] / (rec["total_us"] * 1e-6) / 1e12
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--kernel-stats":
        print(json.dumps(kernel_stats(sys.argv[2])))
        return
    import torch
    import sprsolve_amd as sa
    dev = torch.device("cuda", 0)
    ctx = sa.default_ctx(0)
    if len(sys.argv) > 1 and sys.argv[1] == "--kernels":
        A, n, _ = _cfg3(torch, sa, dev)
        B = _columns(torch, n, 8, dev); X = torch.zeros_like(B)
        _run_many(sa.CGMany.new(A, n, 8), B, X, KERNEL_STEPS)
        cols = [B[:, j].contiguous() for j in range(8)]
        _run_seq(sa, sa.CG.new(A, n), cols, [torch.zeros_like(c) for c in cols], KERNEL_STEPS)
        torch.cuda.synchronize()
        print(json.dumps(dict(kernels_run=True, steps=KERNEL_STEPS, route=A.spmv_route())))
        return
    out = dict(what="batched CG vs k sequential CG solves, f64, no preconditioner; ms per iteration per right-hand side = "
                    "(T(%d) - T(%d)) / %d / k at tol 0" % (K_HI, K_LO, K_HI - K_LO))
    for name, make in (("cfg2_plain_stream", _cfg2), ("cfg3", _cfg3), ("cfg5_plain_stream", _cfg5)):
        A, n, dict_knob = make(torch, sa, dev)
        if A is None:
            out[name] = dict(skipped="not enough device memory for 5 blocks of n x 8 doubles")
            continue
        ctx.set("spmv_dict", dict_knob)
        rec = dict(n=n, nnz=A.nnz(), route_sequential=A.spmv_route())
        seq = sa.CG.new(A, n)
        for k in KS:
            B = _columns(torch, n, k, dev); X = torch.zeros_like(B)
            cols = [B[:, j].contiguous() for j in range(k)]; xs = [torch.zeros_like(c) for c in cols]
            many = sa.CGMany.new(A, n, k)
            m = _marginal(torch, lambda its: _run_many(many, B, X, its)) / k
            q = _marginal(torch, lambda its: _run_seq(sa, seq, cols, xs, its)) / k
            rec["k%d" % k] = dict(batched_ms_per_it_per_rhs=m, sequential_ms_per_it_per_rhs=q, ratio=q / m)
            many.close(); del B, X, cols, xs
        ctx.set("spmv_dict", -1)
        out[name] = rec
        seq.close(); del A
    print(json.dumps(out))


if __name__ == "__main__":
    main()
