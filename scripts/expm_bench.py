"""The Krylov propagator w = exp(tA) v (sprs_expm_*) on one GPU: the heat equation u' = -L u on gen.poisson3d(128, 126, 124), f64,
ncv = 30, the default tolerance, the start vector gen.uniform(7, n).  t starts at ten times the first sub-step's size, which a probe
with max_steps = 1 reports, and is doubled until the solve takes ten sub-steps or more (the heat equation smooths its state, so the
steps lengthen on the way).  Reported for the last of these solves: wall ms (the earlier ones are the warm-up, a context
synchronise before every clock read), sub-steps, rejections, products, ms per sub-step, the error estimate.  Then the same
work once more in a child process under `rocprofv3 --kernel-trace --stats`, from which come the mean microseconds of
ex_step_kernel and, for ExCombine and for GmUpdate (the fused vector kernel beside it in the same run), calls, mean microseconds,
the bytes each must move and bytes / time.  Every sub-step of the process counts, the probe's and the shorter solves' too.
ExCombine moves (m + 3) n 8 bytes a call (v_0 .. v_m read, one vector written); GmUpdate at step j moves (j + 3) n 8 (v_0 .. v_j
and p read, one vector written).  Every figure is from a single run.  No speed threshold is set.  One JSON line to stdout and to
--out PATH (default profiles/expm_bench.json).

    python scripts/expm_bench.py [--no-profile] [--out PATH]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = (128, 126, 124)
NCV = 30


def child(out):
    """The probe and the solves in this process; the record of the last solve goes to `out`."""
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    ip, ix, d = gen.poisson3d(*GRID)[:3]
    n = ip.size - 1
    A = sa.HipCsr.new((n, n), ip, ix, -d)
    E = sa.Expm.new(A, n, NCV)
    v = sa.DevVec.from_numpy(gen.uniform(7, n))
    w = sa.DevVec(n, "float64", ctx)
    try:
        E.apply(1e6, v, max_steps=1, out=w)
        raise SystemExit("the probe finished in one sub-step")
    except sa.error.InsufficientIterNum as e:
        tau1 = e.info["t_done"]
    t, all_steps = 5.0 * tau1, 1
    for _ in range(12):
        t = 2.0 * t
        ctx.sync()
        t0 = time.perf_counter()
        _, info = E.apply(t, v, out=w)
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3
        all_steps += info["steps"]
        if info["steps"] >= 10:
            break
    rec = dict(grid=list(GRID), n=int(n), nnz=int(ip[-1]), dtype="float64", ncv=NCV, tau1=tau1, t=t, spmv_kernel=A.spmv_route()["kernel"],
               stream_format=A.stream_format(), wall_ms=round(ms, 2), ms_per_step=round(ms / max(1, info["steps"]), 3), steps=info["steps"],
               rejects=info["rejects"], products=info["matvecs"], err=info["err"], hump=info["hump"], all_steps=all_steps, single_run=True)
    E.close()
    with open(out, "w") as f:
        f.write(json.dumps(rec) + "\n")


def kernel_stats(path, rec):
    """ex_step_kernel's mean time and the rates of ExCombine and GmUpdate from a rocprofv3 kernel-stats table of child()."""
    n, m = rec["n"], rec["ncv"]
    steps = rec["all_steps"]                                  # the probe's sub-step and the shorter solves' included
    rows = list(csv.DictReader(open(path)))
    out = {}
    for key in ("ex_step_kernel", "ExCombine", "GmUpdate"):
        sel = [r for r in rows if key in r["Name"]]
        if not sel:
            continue
        calls = sum(int(r["Calls"]) for r in sel)
        ns = sum(float(r["TotalDurationNs"]) for r in sel)
        o = dict(calls=calls, mean_us=round(ns / calls / 1e3, 2))
        if key == "ExCombine":
            nbytes = steps * (m + 3) * n * 8
        elif key == "GmUpdate":
            nbytes = 2 * steps * sum(j + 3 for j in range(m)) * n * 8         # two launches a step
        else:
            nbytes = 0
        if nbytes:
            o.update(gbytes=round(nbytes / 1e9, 3), tb_per_s=round(nbytes / ns / 1e3, 3))
        out[key] = o
    return out


def main(args):
    me = os.path.abspath(__file__)
    with tempfile.TemporaryDirectory() as tmp:
        run = os.path.join(tmp, "run.json")
        subprocess.run([sys.executable, me, "--child", run], check=True, timeout=600)
        rec = json.load(open(run))
        if not args.no_profile:
            prof = os.path.join(tmp, "prof.json")
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(tmp, "rp"), "--",
                            sys.executable, me, "--child", prof], check=True, timeout=900, stdout=subprocess.DEVNULL)
            tables = glob.glob(os.path.join(tmp, "rp", "**", "*_kernel_stats.csv"), recursive=True)
            assert len(tables) == 1, tables
            prec = json.load(open(prof))
            assert (prec["steps"], prec["products"]) == (rec["steps"], rec["products"]), (prec, rec)
            rec["profiled"] = kernel_stats(tables[0], prec)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-profile", action="store_true", help="skip the run under rocprofv3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expm_bench.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    child(a.child) if a.child else main(a)
