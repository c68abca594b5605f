"""The AMG hierarchy built on the device (sprs_amg_create_dev, csrc/amg_setup.hpp) against tests/_amg_par_ref.py: aggregates,
rounds, patterns and omega exactly and the values of A_l, P_l, R_l BIT FOR BIT, read back through sprs_amg_level_read (which
unpacks the sliced-row layout on a device-built handle); one application of the cycle bit for bit against the checker's
Applier, which covers the dense LU's effect; seeds; the refusals with their rows; and the solvers on a device-built handle —
CG and GMRES in literal mode against the checker with the comparisons of tests/test_gpu_amg.py, BiCGStab, MINRES, IDR(s) and
LOBPCG to tolerance.

Not run here: the refusal of a distributed A needs several ranks and that of more than 2^31 - 1 entries 13 GB; both are the
host creation's own code path (amg_create_args in csrc/amg.hip), taken before either set-up starts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _amg_par_ref as par  # noqa: E402
import _amg_ref as amg  # noqa: E402
import _ilu_ref as ref  # noqa: E402
from test_amg_cpu import ALL, C32, C64, F32, F64, GMRES_RESTART, GMRES_TRACE_ROWS, MAX_LEVELS, THETA, bits, system_of  # noqa: E402
from test_amg_par_cpu import (CG_PAR_COUNTS, GMRES_PAR_COUNTS, ROUNDS, ROWS, WIDE_HUBS, WIDE_ROUNDS, WIDE_SEED, par_hierarchy_of,  # noqa: E402
                              par_system_of)
from test_gmres_cpu import trace_close as gm_trace_close  # noqa: E402
from test_gpu_ilu import _cg_trace_array, _cg_trace_close, _run, _true_res  # noqa: E402

pytestmark = pytest.mark.gpu

_ids = lambda v: v if isinstance(v, str) else (np.dtype(v).name if isinstance(v, type) else str(v))


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


_made = {}


def _handles(sa, name, dt, seed=0):
    """(ip, ix, d, rhs, checker's hierarchy, A, device-built AMG), made once per case."""
    key = (name, np.dtype(dt).name, seed)
    if key not in _made:
        ip, ix, d, rhs = par_system_of(name, key[1])
        n = rhs.size
        A = sa.HipCsr.new((n, n), ip, ix, d)
        _made[key] = (ip, ix, d, rhs, par_hierarchy_of(name, key[1], seed), A, sa.AMG.new(A, setup="device", seed=seed))
    return _made[key]


CASES = ([(name, dt, 0) for name in ("p3_12x11x10", "cd24x20", "tri300", "ragged1000", "hub600") for dt in ALL] +
         [("p3_12x11x10", F64, 1), ("p3_24x22x20", F64, 0), ("p3_8x7x6", F64, 0), ("isolated400", F64, 0), ("isolated400", C64, 1),
          ("onesided400", F64, 1), ("onesided400", F32, 0)] +
         # the whole-wavefront walk where a helping lane's own vertex would change the round count (tests/test_amg_par_cpu.py)
         [(name, dt, WIDE_SEED) for name in sorted(WIDE_HUBS) for dt in (F64, F32)])


# ------------------------------------------------------------------------------------------------ 1. the hierarchy
@pytest.mark.parametrize("name,dt,seed", CASES, ids=_ids)
def test_hierarchy_equals_the_checkers(sa, name, dt, seed):
    ip, ix, d, rhs, H, A, P = _handles(sa, name, dt, seed)
    inf = P.info
    print(name, np.dtype(dt).name, seed, inf)
    assert inf["setup"] == "device"
    assert inf["levels"] == len(H.levels) and inf["rows"] == [L.n for L in H.levels]
    assert inf["rounds"] == H.rounds
    if np.dtype(dt) == np.dtype(F64) and name in ROWS:
        assert inf["rows"] == ROWS[name][seed] and inf["rounds"] == ROUNDS[name][seed]
    if name in WIDE_HUBS:
        assert inf["rounds"] == WIDE_ROUNDS[name]
    assert inf["nnz"] == [int(L.ip[-1]) for L in H.levels]
    assert inf["p_nnz"] == [int(L.P[0][-1]) if L.P is not None else 0 for L in H.levels]
    assert inf["lu_rows"] == (H.levels[-1].n if H.lu is not None else 0)
    for l, L in enumerate(H.levels):
        assert bits(np.array([inf["omega"][l]], amg.Ops(dt).R)).tolist() == bits(np.array([L.omega])).tolist()
        for which, want in (("A", (L.ip, L.ix, L.val)), ("P", L.P), ("R", L.R)):
            if want is None:
                continue
            gp, gx, gv = P.level(l, which)
            assert np.array_equal(gp, want[0]) and np.array_equal(gx, want[1]), (l, which)
            assert np.array_equal(bits(gv), bits(want[2])), (l, which)
        if L.agg is not None:
            assert np.array_equal(P.aggregates(l), L.agg), l
    last = len(H.levels) - 1                                                      # the coarsest level has no P, R or aggregates
    for bad in (lambda: P.level(last, "P"), lambda: P.level(last, "R"), lambda: P.aggregates(last), lambda: P.level(last + 1), lambda: P.level(-1)):
        with pytest.raises(ValueError):
            bad()


def test_level_sizes_that_exercise_the_kernels(sa):
    """What the cases above are chosen for: 10 560 rows are 42 workgroups and 1007 = 15 * 64 + 47 rows a partial last slice;
    p3_8x7x6 runs entirely inside the tail kernel; the hub's list of 302 neighbours is walked by a whole wavefront."""
    assert _handles(sa, "p3_24x22x20", F64)[6].info["rows"] == [10560, 1007, 98]
    inf = _handles(sa, "p3_8x7x6", F64)[6].info
    assert inf["tail_level"] == 0 and inf["launches"] == 1 and inf["levels"] == 2
    agg = _handles(sa, "hub600", F64)[6].aggregates(0)
    assert np.count_nonzero(agg == agg[17]) >= 200


# ------------------------------------------------------------------------------------------------ 2. one application
@pytest.mark.parametrize("name,dt,seed", CASES, ids=_ids)
def test_cycle_bits(sa, name, dt, seed):
    ip, ix, d, rhs, H, A, P = _handles(sa, name, dt, seed)
    want = amg.Applier(H)(rhs)
    out = np.zeros_like(rhs)
    P.mul_vec(rhs, out)                                                           # host arrays, out of place
    assert np.array_equal(bits(out), bits(want))
    buf = rhs.copy()
    P.mul_vec(buf, buf)                                                           # host arrays, in place
    assert np.array_equal(bits(buf), bits(want))
    v = sa.DevVec.from_numpy(rhs)
    P.mul_vec(v, v)                                                               # device vectors, in place
    assert np.array_equal(bits(v.to_numpy()), bits(want))
    a, b = sa.DevVec.from_numpy(rhs), sa.DevVec.from_numpy(np.zeros_like(rhs))
    P.mul_vec(a, b)                                                               # device vectors, out of place
    assert np.array_equal(bits(b.to_numpy()), bits(want)) and np.array_equal(bits(a.to_numpy()), bits(rhs))


# ------------------------------------------------------------------------------------------------ 3. seeds, host handles
def _level_bytes(P):
    inf = P.info
    out = []
    for l in range(inf["levels"]):
        for which in ("A", "P", "R")[:3 if l + 1 < inf["levels"] else 1]:
            out += [a.tobytes() for a in P.level(l, which)]
        if l + 1 < inf["levels"]:
            out.append(P.aggregates(l).tobytes())
    return out


def test_seeds_differ_and_one_seed_gives_the_same_bytes(sa):
    ip, ix, d, rhs, H, A, P0 = _handles(sa, "p3_12x11x10", F64, 0)
    P1 = _handles(sa, "p3_12x11x10", F64, 1)[6]
    assert not np.array_equal(P0.aggregates(0), P1.aggregates(0))
    again = sa.AMG.new(A, setup="device", seed=0)
    assert again.info == P0.info and _level_bytes(again) == _level_bytes(P0)
    again.close()
    hub_a = _handles(sa, "hub600", F64, 0)
    again = sa.AMG.new(hub_a[5], setup="device", seed=0)                          # the atomically filled half of G does not reach a result
    assert _level_bytes(again) == _level_bytes(hub_a[6])
    again.close()


def test_host_built_handle_reports_host_and_zero_rounds(sa):
    A = _handles(sa, "p3_24x22x20", F64)[5]
    P = sa.AMG.new(A)
    inf = P.info
    assert inf["setup"] == "host" and inf["rounds"] == [0, 0] and inf["rows"] == [10560, 1293, 138]
    assert not any(P.setup_ms.values())
    assert sa.AMG.new(A, setup="host", seed=5).info == inf                        # the host rule has no seed
    dev = _handles(sa, "p3_24x22x20", F64)[6]
    assert set(dev.setup_ms) == set(sa.AMG.STAGES) and not any(dev.setup_ms.values())   # the stage clock is a diagnostic: off
    os.environ["SPRS_CREATE_TRACE"] = "1"
    try:
        timed = sa.AMG.new(A, setup="device")
    finally:
        del os.environ["SPRS_CREATE_TRACE"]
    ms = timed.setup_ms
    assert all(v >= 0 for v in ms.values()) and sum(ms.values()) > 0
    assert timed.info == dev.info and _level_bytes(timed) == _level_bytes(dev)          # ... and changes nothing it times
    timed.close()
    with pytest.raises(ValueError, match="setup"):
        sa.AMG.new(A, setup="gpu")
    P.close()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_creation_errors(sa):
    E = sa.error
    new = lambda A, **kw: sa.AMG.new(A, setup="device", **kw)
    ip = np.array([0, 2, 4], np.int32); ix = np.array([0, 1, 0, 1], np.int32)
    for dt in ALL:
        with pytest.raises(E.ZeorDiagonalElem) as ei:                             # the coarse LU: u_11 = 1 - 1*1
            new(sa.HipCsr.new((2, 2), ip, ix, np.ones(4, dt)))
        assert "1" in str(ei.value)
    ip3 = np.array([0, 2, 3, 5, 6], np.int32); ix3 = np.array([0, 1, 0, 1, 2, 2], np.int32)
    with pytest.raises(E.ZeorDiagonalElem) as ei:                                 # a missing diagonal: row 1
        new(sa.HipCsr.new((4, 4), ip3, ix3, np.ones(6)))
    assert "1" in str(ei.value)
    with pytest.raises(E.ZeorDiagonalElem) as ei:                                 # a zero diagonal: row 1
        new(sa.HipCsr.new((2, 2), ip, ix, np.array([1.0, 1.0, 1.0, 0.0])))
    assert "1" in str(ei.value)
    with pytest.raises(E.ZeorDiagonalElem) as ei:                                 # a diagonal that is not finite: row 0
        new(sa.HipCsr.new((2, 2), ip, ix, np.array([np.inf, 1.0, 1.0, 1.0])))
    assert "0" in str(ei.value)
    # the smallest of several offending rows, on a matrix of more than one workgroup
    ipc, ixc, dc, _ = system_of("cd24x20", "float64")
    rows = np.repeat(np.arange(480), np.diff(ipc))
    dz = dc.copy(); dz[(rows == ixc) & np.isin(rows, (301, 77, 402))] = 0.0
    with pytest.raises(E.ZeorDiagonalElem) as ei:
        new(sa.HipCsr.new((480, 480), ipc, ixc, dz))
    assert "77" in str(ei.value)
    with pytest.raises(E.IncompatibleMatrixFormat):                               # not square
        new(sa.HipCsr.new((2, 3), ip, np.array([0, 2, 0, 1], np.int32), np.ones(4)))
    for bad, row in ((np.array([1, 0, 0, 1], np.int32), 0), (np.array([0, 1, 1, 1], np.int32), 1)):   # unsorted; duplicate
        with pytest.raises(ValueError, match="row %d are not strictly ascending" % row):
            new(sa.HipCsr.new((2, 2), ip, bad, np.array([2.0, 1.0, 1.0, 2.0])))
    A = sa.HipCsr.new((2, 2), ip, ix, np.array([2.0, 1.0, 1.0, 2.0]))
    for kw in (dict(theta=-1.0), dict(theta=float("nan")), dict(coarse_max=0), dict(coarse_max=amg.COARSE_LIMIT + 1), dict(max_levels=0),
               dict(max_levels=amg.LEVELS_LIMIT + 1)):
        with pytest.raises(ValueError):
            new(A, **kw)
    P = new(A)
    assert P.info["levels"] == 1 and P.info["lu_rows"] == 2 and P.info["rounds"] == []
    with pytest.raises(sa.error.DimensionMismatch):
        P.mul_vec(np.ones(3), np.zeros(3))


def test_stop_rules(sa):
    """max_levels ends the coarsening above coarse_max (Jacobi sweeps for the coarse solve, no LU and no download), and
    theta = 10 leaves singletons only, so the half-rows stop makes level 0 the coarsest."""
    ip, ix, d, rhs = system_of("p3_24x22x20", "float64")
    n = rhs.size
    A = _handles(sa, "p3_24x22x20", F64)[5]
    H = par.build(ip, ix, d, THETA, 64, 2, 0)
    P = sa.AMG.new(A, coarse_max=64, max_levels=2, setup="device")
    inf = P.info
    assert len(H.levels) == 2 and H.lu is None and inf["rows"] == [10560, 1007] and inf["lu_rows"] == 0 and inf["rounds"] == H.rounds
    out = np.zeros(n)
    P.mul_vec(rhs, out)
    assert np.array_equal(bits(out), bits(amg.Applier(H)(rhs)))
    P.close()
    ip, ix, d, rhs = system_of("tri300", "float64")
    H = par.build(ip, ix, d, 10.0, 16, MAX_LEVELS, 0)
    P = sa.AMG.new(sa.HipCsr.new((300, 300), ip, ix, d), theta=10.0, coarse_max=16, setup="device")
    assert len(H.levels) == 1 and H.lu is None and P.info["levels"] == 1 and P.info["rounds"] == []
    with pytest.raises(ValueError):
        P.aggregates(0)
    out = np.zeros(300)
    P.mul_vec(rhs, out)
    assert np.array_equal(bits(out), bits(amg.Applier(H)(rhs)))
    P.close()


# ------------------------------------------------------------------------------------------------ 5. CG and GMRES, literal mode
@pytest.mark.parametrize("seed", (0, 1))
def test_cg_literal_follows_the_checker(sa, seed):
    ip, ix, d, rhs = system_of("cg", "float64")
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    P = sa.AMG.new(A, setup="device", seed=seed)
    H = par.build(ip, ix, d, THETA, 256, MAX_LEVELS, seed)
    max_iter = 2 * CG_PAR_COUNTS[seed]
    o = ref.cg(ip, ix, d, rhs, np.zeros(n), max_iter, 1e-10, prec=amg.Applier(H))
    assert o.status == ref.OK and o.its == CG_PAR_COUNTS[seed]
    s = sa.CG.new(A, n); s.set_mode("literal"); s.set_trace(max_iter)
    x = np.zeros(n)
    st, its, res = _run(sa, s, P, rhs, x, max_iter, 1e-10)
    tl, want = s.trace(), _cg_trace_array(o.trace)
    err = np.max(np.abs(x - o.x))
    print("cg + device-built amg, seed %d: its %d (checker %d) res %.3e (checker %.3e) max|x - checker| %.3e" % (seed, its, o.its, res, o.res, err))
    assert (st, its) == (o.status, o.its)
    assert tl.shape == want.shape == (o.its - 1, 8)
    assert _cg_trace_close(tl, want, rtol=1e-9, atol=1e-12)
    assert err <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
    assert np.isclose(res, o.res, rtol=1e-9, atol=1e-12)
    s = sa.CG.new(A, n)                                                           # fused mode: to tolerance
    xf = np.zeros(n)
    stf, itf, _ = _run(sa, s, P, rhs, xf, max_iter, 1e-10)
    assert stf == ref.OK and _true_res(ip, ix, d, rhs, xf) <= 1e-9 and np.max(np.abs(xf - x)) <= 1e-7 * np.max(np.abs(x))


@pytest.mark.parametrize("dt,seed", [(F64, 0), (F64, 1), (C64, 0)], ids=_ids)
def test_gmres_literal_follows_the_checker(sa, dt, seed):
    ip, ix, d, rhs, H, A, P = _handles(sa, "cd24x20", dt, seed)
    n = rhs.size
    m = GMRES_RESTART
    max_iter = 60
    o = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), max_iter, 1e-10, restart=m, prec=amg.Applier(H))
    assert o.status == ref.OK and o.its > m and 2 * o.its <= max_iter
    if np.dtype(dt) == np.dtype(F64):
        assert o.its == GMRES_PAR_COUNTS[seed]
    s = sa.GMRES.new(A, n, m); s.set_mode("literal"); s.set_trace(max_iter)
    x = np.zeros(n, dt)
    st, its, res = _run(sa, s, P, rhs, x, max_iter, 1e-10)
    tl = s.trace()
    want = np.array([[t[0], t[1], t[2], t[3].real, t[3].imag, t[4], t[5].real, t[5].imag] for t in o.trace]).reshape(-1, 8)
    err = np.max(np.abs(x - o.x))
    true_res = _true_res(ip, ix, d, rhs, x)
    print("gmres + device-built amg %s seed %d: its %d (checker %d) res %.3e (checker %.3e) true %.3e max|x - checker| %.3e"
          % (np.dtype(dt).name, seed, its, o.its, res, o.res, true_res, err))
    assert st == o.status == ref.OK and its == o.its
    assert tl.shape == (its, 8) and np.array_equal(tl[:, 0], np.arange(1, its + 1))
    assert res <= 1e-10 and true_res <= 1e-9
    k = GMRES_TRACE_ROWS
    assert gm_trace_close(tl[:k], want[:k], rtol=1e-9, atol=1e-12)
    assert err <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
    assert np.isclose(res, o.res, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 6. the other solvers
@pytest.mark.parametrize("solver", ["bicgstab", "idrs", "minres"])
def test_solvers_converge_with_a_device_built_handle(sa, solver):
    name = "cg" if solver == "minres" else "cd24x20"                              # MINRES wants a Hermitian A
    if name == "cg":
        ip, ix, d, rhs = system_of("cg", "float64")
        A = sa.HipCsr.new((rhs.size, rhs.size), ip, ix, d)
        P = sa.AMG.new(A, setup="device")
    else:
        ip, ix, d, rhs, _, A, P = _handles(sa, name, F64)
    n = rhs.size
    S = {"bicgstab": lambda: sa.BiCGStab.new(A, n), "idrs": lambda: sa.IDRS.new(A, n, 4), "minres": lambda: sa.MinRes.new(A, n)}[solver]()
    x0 = np.zeros(n); x = np.zeros(n)
    plain = S.solve(rhs, x0, 2000, 1e-10)[0]
    its, res = S.precond_solve(P, rhs, x, 2000, 1e-10)
    true_res = _true_res(ip, ix, d, rhs, x)
    print("%s: %d iterations (%d without), res %.3e true %.3e" % (solver, its, plain, res, true_res))
    assert its < plain and res <= 1e-10 and true_res <= 1e-9
    dB, dX = sa.DevVec.from_numpy(rhs), sa.DevVec.from_numpy(np.zeros(n))
    dits, dres = S.precond_solve(P, dB, dX, 2000, 1e-10)
    assert (dits, dres) == (its, res) and dX.to_numpy().tobytes() == x.tobytes()


def test_lobpcg_converges_with_a_device_built_handle(sa):
    ip, ix, d, rhs, _, A, P = _handles(sa, "p3_12x11x10", F64)
    n = rhs.size
    import scipy.sparse as sp
    M = sp.csr_matrix((d, ix, ip), shape=(n, n))
    lam = np.linalg.eigvalsh(M.toarray())
    S = sa.Lobpcg.new(A, n, 8)
    plain = S.solve(4, "smallest")[2]["iters"]
    vals, X, info = S.solve(4, "smallest", precond=P)
    print("lobpcg: %d iterations (%d without)" % (info["iters"], plain), vals)
    assert info["nconv"] == 4 and info["iters"] < plain
    assert np.max(np.abs(vals - lam[:4])) <= 1e-8 * lam[-1]
    for c in range(4):
        assert np.linalg.norm(M @ X[c] - vals[c] * X[c]) <= 1e-8 * lam[-1] * np.linalg.norm(X[c])
