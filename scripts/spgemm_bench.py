"""The device CSR x CSR product (sprs_csr_matmul) and the AMG creation that runs on it, one GPU, one process, f64, on the 7-point
3-D Poisson matrix (gen.poisson3d, 128^3 by default).  After one warm-up creation (the first call of a process pays the
code-object load): the median and the spread (max - min) of three runs of AMG.new and of each level-0 product through
HipCsr.matmul — A P, and R (A P) with P and R read from the handle — and the rows each product sent to the short / table / dense
kernel.  The clock is read after a context synchronisation on both sides.  The creation time of the commit before the device
products is measured by that commit's scripts/amg_bench.py on the same machine and passed in with --parent-ms.  No speed threshold
is set.  One JSON line to stdout (and to --out PATH).

usage: python scripts/spgemm_bench.py [--p3 N] [--parent-ms MS] [--out PATH]      (run on the GPU box, under a `timeout`)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RUNS = 3


def timed(ctx, make):
    ctx.sync()
    t0 = time.perf_counter()
    h = make()
    ctx.sync()
    return h, (time.perf_counter() - t0) * 1e3


def three(ctx, make):
    ms = []
    for _ in range(RUNS):
        h, t = timed(ctx, make)
        ms.append(t)
        last = h
    return last, dict(median_ms=statistics.median(ms), spread_ms=max(ms) - min(ms), runs_ms=ms)


def main():
    args = sys.argv[1:]
    p3 = int(args[args.index("--p3") + 1]) if "--p3" in args else 128
    path = args[args.index("--out") + 1] if "--out" in args else None
    parent = float(args[args.index("--parent-ms") + 1]) if "--parent-ms" in args else None
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    ip, ix, d, _ = gen.poisson3d(p3, p3, p3)
    n = ip.size - 1
    A = sa.HipCsr.new((n, n), ip, ix, d)
    rec = dict(what="poisson3d(%d^3), f64: AMG.new and the level-0 products A P and R (A P) through HipCsr.matmul, median and spread "
                    "(max - min) of %d runs after one warm-up creation; info = rows on the short / table / dense kernel and the two limits"
                    % (p3, RUNS), n=int(n), nnz=int(ip[-1]))
    _, rec["amg_create_first_ms"] = timed(ctx, lambda: sa.AMG.new(A))
    M, rec["amg_create"] = three(ctx, lambda: sa.AMG.new(A))
    inf = M.info
    rec["amg_info"] = inf
    nc = inf["rows"][1]
    P = sa.HipCsr.new((n, nc), *M.level(0, "P"))
    R = sa.HipCsr.new((nc, n), *M.level(0, "R"))
    (AP, ap_info), rec["a_times_p"] = three(ctx, lambda: A.matmul(P, info=True))
    (AC, ac_info), rec["r_times_ap"] = three(ctx, lambda: R.matmul(AP, info=True))
    rec["a_times_p"].update(info=ap_info, nnz=AP.nnz())
    rec["r_times_ap"].update(info=ac_info, nnz=AC.nnz())
    assert AC.nnz() == inf["nnz"][1]
    if parent is not None:
        rec["parent_amg_create_ms"] = parent
        rec["create_over_parent"] = rec["amg_create"]["median_ms"] / parent
    line = json.dumps(rec)
    print(line)
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
