"""ILU(0) with Jacobi-sweep triangular solves on the GPU (sprs_ilu0_create_sweeps, csrc/ilu0.hip) against the loops of
tests/_ilu_sweeps_ref.py: the three solves BIT FOR BIT (host arrays, device vectors, in place, repeated), the fixed point against
the library's own exact handle, and CG / GMRES preconditioned by k = 3 sweeps with the comparisons, tolerances and margins of
tests/test_gpu_ilu.py.  The checker's counts (tests/test_ilu_sweeps_cpu.py) stand behind every max_iter: twice the count."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ilu_ref as ref  # noqa: E402
from _ilu_sweeps_ref import Sweeps  # noqa: E402
from test_gmres_cpu import trace_close as gm_trace_close  # noqa: E402
from test_gpu_ilu import _cg_trace_array, _cg_trace_close, _margin, _run, _true_res  # noqa: E402
from test_ilu_cpu import ALL, C32, C64, CG_COUNTS, F32, F64, GMRES_COUNTS, GMRES_RESTART, GMRES_TRACE_ROWS, bits, factors_of, is_single, tol_of  # noqa: E402
from test_ilu_sweeps_cpu import SWEEP_CG_COUNTS, SWEEP_GMRES_COUNTS, SWEEPS  # noqa: E402

pytestmark = pytest.mark.gpu

_ids = lambda v: v if isinstance(v, str) else np.dtype(v).name


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


def _system(sa, name, dt):
    ip, ix, d, rhs, f = factors_of(name, np.dtype(dt).name)
    n = rhs.size
    return ip, ix, d, rhs, f, sa.HipCsr.new((n, n), ip, ix, d)


def _applies(P):
    return {0: P.mul_vec, 1: P.solve_lower, 2: P.solve_upper}


# 1000 rows are no multiple of 64 and rows of 1 .. 12 entries share a slice; cg f64 has 1320 rows: six workgroups, a part-filled last slice
CASES = [("cd24x20", F64), ("cd24x20", F32), ("herm300", C64), ("herm300", C32), ("ragged1000", F64), ("cg", F64), ("cg", C64)]


# ------------------------------------------------------------------------------------------------ 1. the stated loops
@pytest.mark.parametrize("name,dt", CASES, ids=_ids)
def test_solves_have_the_bits_of_the_stated_sweeps(sa, name, dt):
    ip, ix, d, rhs, f, A = _system(sa, name, dt)
    n = rhs.size
    for k in (1, 2, 3):
        P = sa.ILU0.new(A, sweeps=k)
        assert P.sweeps == k
        ck = Sweeps(ip, ix, f, k)
        apply = _applies(P)
        for which in (1, 2, 0):
            want = ck.solve(which, rhs)
            for rep in range(2):                                                  # twice in a row: the same bytes
                out = np.zeros(n, dt)
                apply[which](rhs, out)                                            # host entry point
                assert np.array_equal(bits(out), bits(want)), (k, which, "host", rep)
                d_in = sa.DevVec.from_numpy(rhs); d_out = sa.DevVec.from_numpy(np.zeros(n, dt))
                apply[which](d_in, d_out)                                         # device entry point
                assert np.array_equal(bits(d_out.to_numpy()), bits(want)), (k, which, "device", rep)
                assert np.array_equal(bits(d_in.to_numpy()), bits(rhs)), (k, which, "the input was written")
                apply[which](d_in, d_in)                                          # in == out
                assert np.array_equal(bits(d_in.to_numpy()), bits(want)), (k, which, "in place", rep)
            h = rhs.copy()
            apply[which](h, h)                                                    # in == out on host arrays
            assert np.array_equal(bits(h), bits(want)), (k, which, "host in place")
        P.close()


# ------------------------------------------------------------------------------------------------ 2. the fixed point
@pytest.mark.parametrize("name,dt", CASES, ids=_ids)
def test_as_many_sweeps_as_levels_is_the_exact_handle(sa, name, dt):
    ip, ix, d, rhs, f, A = _system(sa, name, dt)
    n = rhs.size
    E = sa.ILU0.new(A)
    le = E.levels
    k = max(le["lower_levels"], le["upper_levels"])
    P = sa.ILU0.new(A, sweeps=k)
    lp = P.levels
    print("%s %s: exact %s, sweeps %s" % (name, np.dtype(dt).name, le, lp))
    assert (E.sweeps, P.sweeps) == (0, k)
    assert (lp["lower_levels"], lp["upper_levels"]) == (le["lower_levels"], le["upper_levels"]) == ref.level_counts(ip, ix)
    assert (lp["lower_launches"], lp["upper_launches"]) == (k - 1, k)
    assert np.array_equal(bits(P.factors()), bits(E.factors())) and np.array_equal(bits(P.factors()), bits(f))
    for which in (1, 2, 0):
        a = np.zeros(n, dt); b = np.zeros(n, dt)
        _applies(E)[which](rhs, a); _applies(P)[which](rhs, b)
        assert np.array_equal(bits(a), bits(b)), which


# ------------------------------------------------------------------------------------------------ 3. one larger grid
def test_larger_grid_128_workgroups(sa):
    ip, ix, d, rhs, f, A = _system(sa, "p3_64x64x8", F64)
    n = rhs.size
    assert n == 32768
    P = sa.ILU0.new(A, sweeps=SWEEPS)
    want = Sweeps(ip, ix, f, SWEEPS).solve(0, rhs)
    out = np.zeros(n)
    P.mul_vec(rhs, out)
    assert np.array_equal(bits(out), bits(want))


# ------------------------------------------------------------------------------------------------ 3b. padded slots are skipped
PROBE_N = 130                                                # two full slices of 64 rows and two rows
PROBE_SEED = 20


@functools.lru_cache(maxsize=None)
def padding_probe(dtname):
    """A 130-row system whose rows have 0 .. 9 off-diagonal entries (so every slice is padded) under a dominant diagonal, columns
    ascending, and column 0 stored by rows 0, 5 and 70 only; a vector that is finite except for inf in entry 0; and the
    checkers' solves of it.  Rows take their columns from their own residue class modulo 5, so the inf reaches rows of the
    class of 0, 5 and 70 alone and four rows in five stay finite whatever PROBE_SEED draws.  A padded slot (column 0, value
    zero) that were multiplied would read entry 0 and turn such a row into NaN.
    -> ip, ix, data, v, the checker's factors, {(sweeps, which): checker's result}"""
    dt = np.dtype(dtname)
    rng = np.random.default_rng(PROBE_SEED)
    n = PROBE_N
    rows = []
    for i in range(n):
        cand = [j for j in range(1, n) if j % 5 == i % 5 and j != i]
        cols = set(rng.choice(cand, size=(i + i // 10) % 10, replace=False).tolist()) | {i}
        if i in (5, 70):
            cols.add(0)
        rows.append(sorted(cols))
    assert sorted({len(r) - 1 - (i in (5, 70)) for i, r in enumerate(rows)}) == list(range(10))
    ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ix = np.concatenate(rows).astype(np.int32)
    assert [i for i in range(n) if 0 in rows[i]] == [0, 5, 70]
    data = rng.uniform(-1, 1, ix.size) + (1j * rng.uniform(-1, 1, ix.size) if dt.kind == "c" else 0)
    data[ix == np.repeat(np.arange(n), np.diff(ip))] = 16.0
    data = data.astype(dt)
    v = (rng.uniform(-1, 1, n) + (1j * rng.uniform(-1, 1, n) if dt.kind == "c" else 0)).astype(dt)
    v[0] = np.inf
    f = ref.ilu0(ip, ix, data)
    assert f.status == ref.OK
    with np.errstate(all="ignore"):
        want = {(k, which): (Sweeps(ip, ix, f.val, k) if k else ref.Applier(ip, ix, f.val)).solve(which, v) for k in (0, 2) for which in (1, 2)}
    return ip, ix, data, v, f.val, want


@pytest.mark.parametrize("dt", [F64, C32], ids=_ids)
def test_padded_slots_are_skipped_not_multiplied(sa, dt):
    ip, ix, data, v, f, want = padding_probe(np.dtype(dt).name)
    n = PROBE_N
    A = sa.HipCsr.new((n, n), ip, ix, data)
    for k in (0, 2):                                                              # the exact solves, then two sweeps
        P = sa.ILU0.new(A, sweeps=k)
        assert np.array_equal(bits(P.factors()), bits(f))
        for which in (1, 2):
            w = want[k, which]
            finite = np.isfinite(w)
            print("%s sweeps %d which %d: the checker leaves %d of %d entries finite" % (np.dtype(dt).name, k, which, finite.sum(), n))
            assert 2 * finite.sum() >= n                                          # (else the comparison below would say little)
            out = np.zeros(n, dt)
            _applies(P)[which](v, out)                                            # host entry point
            d_v = sa.DevVec.from_numpy(v)
            _applies(P)[which](d_v, d_v)                                          # in place on the device: entry 0 of `out` is inf from the start
            for got, how in ((out, "host"), (d_v.to_numpy(), "in place")):
                assert np.array_equal(bits(got[finite]), bits(w[finite])), (k, which, how)
                assert not np.any(np.isfinite(got[~finite])), (k, which, how)
        P.close()


# ------------------------------------------------------------------------------------------------ 4. CG + sweeps
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_cg_literal_follows_the_checker_and_fused_follows_literal(sa, dt):
    ip, ix, d, rhs, f, A = _system(sa, "cg", dt)
    P = sa.ILU0.new(A, sweeps=SWEEPS)
    n = rhs.size
    tol = tol_of(dt)
    max_iter = 2 * SWEEP_CG_COUNTS[np.dtype(dt).name]
    o = ref.cg(ip, ix, d, rhs, np.zeros(n, dt), max_iter, tol, prec=Sweeps(ip, ix, f, SWEEPS))
    assert o.status == ref.OK and 2 * o.its <= max_iter
    out = {}
    for mode in ("literal", "fused"):
        s = sa.CG.new(A, n); s.set_mode(mode); s.set_trace(max_iter)
        x = np.zeros(n, dt)
        st, its, res = _run(sa, s, P, rhs, x, max_iter, tol)
        out[mode] = (st, its, res, x, s.trace())
    (sl, il, rl, xl, tl), (sf, itf, rf, xf, tf) = out["literal"], out["fused"]
    want = _cg_trace_array(o.trace)
    err = np.max(np.abs(xl - o.x))
    true_res = _true_res(ip, ix, d, rhs, xf)
    print("cg+sweeps %s: literal its %d (checker %d) res %.3e (checker %.3e) max|x - checker| %.3e; fused its %d res %.3e true %.3e max|dx| %.3e"
          % (np.dtype(dt).name, il, o.its, rl, o.res, err, itf, rf, true_res, np.max(np.abs(xf - xl))))
    # literal against the checker
    assert (sl, il) == (o.status, o.its)
    assert tl.shape == want.shape == (o.its - 1, 8)
    if is_single(dt):
        assert _cg_trace_close(tl[0], want[0], rtol=1e-5)
        assert err < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
        assert rl <= tol
    else:
        assert _cg_trace_close(tl, want, rtol=1e-9, atol=1e-12)
        assert err <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
        assert np.isclose(rl, o.res, rtol=1e-9, atol=1e-12)
    # fused against literal
    assert sf == sl == ref.OK
    assert abs(itf - il) <= _margin(il)
    assert true_res <= 10 * tol
    if is_single(dt):
        assert np.max(np.abs(xf - xl)) < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
        assert _cg_trace_close(tf[0], tl[0], rtol=1e-5)
    else:
        assert np.max(np.abs(xf - xl)) <= 1e-7 * np.max(np.abs(xl))
        k = min(tf.shape[0], tl.shape[0])
        assert k >= il - 2 and _cg_trace_close(tf[:k], tl[:k], rtol=1e-9, atol=1e-12)
    # without a trace buffer (lazy polling) and on device vectors the fused solve returns the same bits
    s = sa.CG.new(A, n)
    x2 = np.zeros(n, dt)
    assert _run(sa, s, P, rhs, x2, max_iter, tol)[:2] == (sf, itf) and np.array_equal(x2, xf)
    d_rhs = sa.DevVec.from_numpy(rhs); d_x = sa.DevVec.from_numpy(np.zeros(n, dt))
    assert _run(sa, s, P, d_rhs, d_x, max_iter, tol)[:2] == (sf, itf) and np.array_equal(d_x.to_numpy(), xf)
    # strictly fewer iterations than Jacobi, and no fewer than the exact handle's (less the margin)
    rows = np.repeat(np.arange(n), np.diff(ip))
    J = sa.DiagPrecond.new(d[rows == ix].real.astype(np.float32 if is_single(dt) else np.float64).copy(), t_dtype=d.dtype)
    stj, itj, _ = _run(sa, s, J, rhs, np.zeros(n, dt), 2 * CG_COUNTS[np.dtype(dt).name][0], tol)
    ste, ite, _ = _run(sa, s, sa.ILU0.new(A), rhs, np.zeros(n, dt), 2 * CG_COUNTS[np.dtype(dt).name][1], tol)
    print("    iterations: Jacobi %d, %d sweeps %d, exact %d" % (itj, SWEEPS, itf, ite))
    assert stj == ste == ref.OK
    assert itf < itj and il < itj
    assert itf >= ite - _margin(ite) and il >= ite - _margin(ite)


# ------------------------------------------------------------------------------------------------ 5. GMRES + sweeps
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_gmres_literal_follows_the_checker_and_fused_follows_literal(sa, dt):
    ip, ix, d, rhs, f, A = _system(sa, "cd24x20", dt)
    P = sa.ILU0.new(A, sweeps=SWEEPS)
    n = rhs.size
    tol = tol_of(dt)
    m = GMRES_RESTART
    max_iter = 2 * SWEEP_GMRES_COUNTS[np.dtype(dt).name]
    o = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), max_iter, tol, restart=m, prec=Sweeps(ip, ix, f, SWEEPS))
    assert o.status == ref.OK and 2 * o.its <= max_iter and o.its > m            # at least two cycles
    out = {}
    for mode in ("literal", "fused"):
        s = sa.GMRES.new(A, n, m); s.set_mode(mode); s.set_trace(max_iter)
        x = np.zeros(n, dt)
        st, its, res = _run(sa, s, P, rhs, x, max_iter, tol)
        out[mode] = (st, its, res, x, s.trace(), _true_res(ip, ix, d, rhs, x))
    (sl, il, rl, xl, tl, true_l), (sf, itf, rf, xf, tf, true_f) = out["literal"], out["fused"]
    want = np.array([[t[0], t[1], t[2], t[3].real, t[3].imag, t[4], t[5].real, t[5].imag] for t in o.trace]).reshape(-1, 8)
    err = np.max(np.abs(xl - o.x))
    print("gmres+sweeps %s: literal its %d (checker %d) res %.3e (checker %.3e) true %.3e max|x - checker| %.3e; fused its %d res %.3e true %.3e max|dx| %.3e"
          % (np.dtype(dt).name, il, o.its, rl, o.res, true_l, err, itf, rf, true_f, np.max(np.abs(xf - xl))))
    # literal against the checker
    assert sl == o.status == ref.OK
    assert abs(il - o.its) <= _margin(o.its)
    assert tl.shape == (il, 8) and np.array_equal(tl[:, 0], np.arange(1, il + 1))
    assert rl <= tol and true_l <= 10 * tol
    k = min(GMRES_TRACE_ROWS, il, o.its)
    if is_single(dt):
        assert gm_trace_close(tl[:1], want[:1], rtol=1e-5, atol=1e-8)
        assert err < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
    else:
        assert gm_trace_close(tl[:k], want[:k], rtol=1e-9, atol=1e-12)
        assert err <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
        assert il == o.its and np.isclose(rl, o.res, rtol=1e-9, atol=1e-12)
    # fused against literal
    assert sf == sl == ref.OK
    assert abs(itf - il) <= _margin(il)
    assert rf <= tol and true_f <= 10 * tol
    assert tf.shape == (itf, 8) and np.array_equal(tf[:, 0], np.arange(1, itf + 1))
    k = min(GMRES_TRACE_ROWS, itf, il)
    if is_single(dt):
        assert np.max(np.abs(xf - xl)) < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
        assert gm_trace_close(tf[:1], tl[:1], rtol=1e-5, atol=1e-8)
    else:
        assert np.max(np.abs(xf - xl)) <= 1e-7 * np.max(np.abs(xl))
        assert gm_trace_close(tf[:k], tl[:k], rtol=1e-9, atol=1e-12)
        assert itf == il and np.isclose(rf, rl, rtol=1e-9, atol=1e-12)
    # lazy polling and device vectors: the same bits
    s = sa.GMRES.new(A, n, m)
    x2 = np.zeros(n, dt)
    assert _run(sa, s, P, rhs, x2, max_iter, tol)[:2] == (sf, itf) and np.array_equal(x2, xf)
    d_rhs = sa.DevVec.from_numpy(rhs); d_x = sa.DevVec.from_numpy(np.zeros(n, dt))
    assert _run(sa, s, P, d_rhs, d_x, max_iter, tol)[:2] == (sf, itf) and np.array_equal(d_x.to_numpy(), xf)
    # strictly fewer steps than Jacobi, and no fewer than the exact handle's (less the margin)
    rows = np.repeat(np.arange(n), np.diff(ip))
    J = sa.DiagPrecond.new(d[rows == ix].real.astype(np.float32 if is_single(dt) else np.float64).copy(), t_dtype=d.dtype)
    stj, itj, _ = _run(sa, s, J, rhs, np.zeros(n, dt), 2 * GMRES_COUNTS[np.dtype(dt).name][0], tol)
    ste, ite, _ = _run(sa, s, sa.ILU0.new(A), rhs, np.zeros(n, dt), 2 * GMRES_COUNTS[np.dtype(dt).name][1], tol)
    print("    steps: Jacobi %d, %d sweeps %d, exact %d" % (itj, SWEEPS, itf, ite))
    assert stj == ste == ref.OK
    assert itf < itj and il < itj
    assert itf >= ite - _margin(ite) and il >= ite - _margin(ite)


# ------------------------------------------------------------------------------------------------ 6. arguments
def test_sweep_count_and_handle_arguments(sa):
    from sprsolve_amd import _lib
    L = _lib.lib()
    ip, ix, d, rhs, f, A = _system(sa, "cd24x20", F64)
    n = rhs.size
    for bad in (-1, 4097):
        with pytest.raises(ValueError, match="sweeps"):
            sa.ILU0.new(A, sweeps=bad)
        h = C.c_void_p(1); row = C.c_int64(-7)
        assert L.sprs_ilu0_create_sweeps(A.h, bad, C.byref(h), C.byref(row)) == _lib.INVALID_ARGUMENT
        assert not h.value and row.value == -1 and b"sweeps" in L.sprs_last_error(A.ctx.h)
    assert L.sprs_ilu0_sweeps(None) == -1
    # sweeps = 0 is sprs_ilu0_create
    h = C.c_void_p()
    assert L.sprs_ilu0_create_sweeps(A.h, 0, C.byref(h), None) == 0 and L.sprs_ilu0_sweeps(h) == 0
    Z = sa.ILU0(h, A.ctx, A.dtype, n, A.nnz())
    E = sa.ILU0.new(A)
    assert Z.levels == E.levels and E.sweeps == 0
    for which in (1, 2, 0):
        a = np.zeros(n); b = np.zeros(n)
        _applies(Z)[which](rhs, a); _applies(E)[which](rhs, b)
        assert np.array_equal(bits(a), bits(b)), which
    # the other creation errors are as for an exact handle
    with pytest.raises(sa.error.IncompatibleMatrixFormat, match="Not a square"):
        sa.ILU0.new(sa.HipCsr.new((2, 3), np.array([0, 2, 4], np.int32), np.array([0, 1, 0, 1], np.int32), np.ones(4)), sweeps=2)
    with pytest.raises(sa.error.ZeorDiagonalElem) as ei:
        sa.ILU0.new(sa.HipCsr.new((2, 2), np.array([0, 2, 4], np.int32), np.array([0, 1, 0, 1], np.int32), np.ones(4)), sweeps=2)
    assert ei.value.row == 1


def test_wrong_sweeps_handle_is_refused_by_the_solvers(sa):
    ip, ix, d, rhs, f, A = _system(sa, "cd24x20", F64)
    n = rhs.size
    P32 = sa.ILU0.new(_system(sa, "cd24x20", F32)[5], sweeps=SWEEPS)
    Psmall = sa.ILU0.new(_system(sa, "tri300", F64)[5], sweeps=SWEEPS)
    for mk in (lambda: sa.CG.new(A, n), lambda: sa.GMRES.new(A, n, 5)):
        x = np.zeros(n)
        with pytest.raises(ValueError):
            mk().precond_solve(P32, rhs, x, 10, 1e-10)                            # another scalar type
        with pytest.raises(sa.error.DimensionMismatch):
            mk().precond_solve(Psmall, rhs, x, 10, 1e-10)                         # another size
        assert not np.any(x)


def test_distributed_operator_is_refused(sa):
    import torch
    from sprsolve_amd import dist as sdist, gen
    from test_gpu_dist import _self_halo_plan
    ctx = sa.default_ctx(0)
    dev = torch.device("cuda", 0)
    comm = sdist.Comm(ctx, 0, 1)
    try:
        n = 96 * 96
        ip, ix, d, rhs = gen.symmetric_banded(n)
        plan = _self_halo_plan(torch, dev, n, ix, lambda c: np.zeros(c.shape, bool))
        A = sdist.DistCsr.from_plan(comm, plan, int(ip[-1]), torch.from_numpy(ip).to(dev), torch.from_numpy(d).to(dev), adopt=True,
                                    to_device=lambda a: torch.from_numpy(a).to(dev))
        with pytest.raises(ValueError, match="distributed"):
            sa.ILU0.new(A, sweeps=SWEEPS)
    finally:
        comm.close()
