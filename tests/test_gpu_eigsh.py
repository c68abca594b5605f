"""The thick-restart Lanczos eigensolver on the GPU (sprs_eigsh_*, csrc/eigsh_fuse.hpp): its Ritz pairs against
numpy.linalg.eigvalsh of the dense matrix and against the numpy restatement of the recurrence (tests/_eigsh_ref.py), the edges
of the basis rotation kernel, every SpMV route, determinism, the invariant-subspace rule, the events and the argument checks.

The restatement's cycle and product counts (tests/test_eigsh_cpu.py::COUNTS holds and checks them; f64 / c64 at tol 1e-10,
f32 / c32 at 1e-4, the default start vector) range from 1 cycle of 64 products (chgrid9x8, ncv 64) to 494 cycles of two
products (hermband700, k = 1, ncv 3, largest, c64).  n = 1320 and 1500 leave a partial last tile in every scalar type (a tile is
64 rows of c64, 128 of f64 / c32, 256 of f32), n = 72 and n = 30 are less than one tile.  The Kronecker family of tests/_kron.py
gives sizes, computed from the device's CU count, at which every workgroup of the in-place rotation makes several trips and
the fused kernels walk several chunks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eigsh_ref as ref  # noqa: E402
import _kron  # noqa: E402
from test_eigsh_cpu import (CASES, KRON_COUNTS, KRON_K, KRON_N1, KRON_NCV, _id, checker, count, kron_checker, kron_n2, orth_defect,  # noqa: E402
                            spectrum, system, true_residual, wanted)

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = [F64, C64, F32, C32]
_KNOBS = ("spmv_dict", "stream_nt", "ew_chunk")


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


@pytest.fixture(autouse=True)
def _restore_knobs(sa):
    ctx = sa.default_ctx(0)
    grid = ctx.get("grid")
    yield
    for k in _KNOBS:
        ctx.set(k, -1)
    ctx.set("grid", grid)


def _eps(dt):
    return float(np.finfo(ref.real_dtype(dt)).eps)


def _handle(sa, name, dt):
    ip, ix, d = system(name, dt)
    n = ip.size - 1
    return sa.HipCsr.new((n, n), ip, ix, d), n


def _solve(sa, name, dt, k, m, which, **kw):
    A, n = _handle(sa, name, dt)
    E = sa.Eigsh.new(A, n, m)
    try:
        return E.solve(k, which, **kw)
    finally:
        E.close()


def _check_pairs(name, dt, k, which, vals, X, info, tol=None):
    """The issue's bounds: |theta_i - lambda_i| <= tol |A|_2 and the true residual, formed in double from X, <= 2 tol |A|_2."""
    A, lam, nrm = spectrum(name)
    tol = ref.default_tol(dt) if tol is None else tol
    assert info["nconv"] == k and vals.shape == (k,) and X.shape == (k, A.shape[0])
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(X)) and np.all(np.isfinite(info["res"]))
    err = float(np.max(np.abs(vals.astype(F64) - wanted(lam, k, which))))
    tr = true_residual(A, vals, X)
    print("%s %s k=%d %s: |theta - lambda| %.3e, true residual %.3e, tol |A| %.3e" % (name, np.dtype(dt).name, k, which, err, tr, tol * nrm))
    assert err <= tol * nrm
    assert tr <= 2 * tol * nrm


def _same_bits(a, b):
    (va, Xa, ia), (vb, Xb, ib) = a, b
    assert np.array_equal(va.view(np.uint8), vb.view(np.uint8))
    assert np.array_equal(ia["res"].view(np.uint8), ib["res"].view(np.uint8))
    assert (Xa is None) == (Xb is None)
    if Xa is not None:
        assert np.array_equal(Xa.view(np.uint8), Xb.view(np.uint8))
    assert (ia["nconv"], ia["restarts"], ia["matvecs"]) == (ib["nconv"], ib["restarts"], ib["matvecs"])


# ---------------------------------------------------------------------------------------------- parity with the mathematics
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_parity(sa, case):
    name, k, m, which, dt = case
    o = checker(name, k, m, which, np.dtype(dt).name)
    vals, X, info = _solve(sa, name, dt, k, m, which)
    _check_pairs(name, dt, k, which, vals, X, info)
    assert orth_defect(X) <= max(8 * orth_defect(o.X), 64 * _eps(dt))
    want = count(name, k, m, which, dt)
    one_cycle = m - ref.restart_size(k, m)
    # a residual estimate that sits on the threshold may fall either way under another summation order
    assert abs(info["matvecs"] - want[1]) <= one_cycle and abs(info["restarts"] - want[0]) <= 1, (info, want)
    assert info["matvecs"] == m + (info["restarts"] - 1) * one_cycle


# ---------------------------------------------------------------------------------------------- several tiles a workgroup
def _kron_solve(sa, n1, n2, dt, k, m, which, **kw):
    ip, ix, d, _, _ = _kron.kron_sum(n1, n2, dt)
    n = ip.size - 1
    E = sa.Eigsh.new(sa.HipCsr.new((n, n), ip, ix, d), n, m)
    try:
        return E.solve(k, which, **kw)
    finally:
        E.close()


def _check_big(n1, n2, dt, k, which, vals, X, info, label):
    """The bounds of _check_pairs on kron_sum(n1, n2): truth from the factors' spectra, the true residual in double."""
    ip, ix, d, lam, nrm = _kron.kron_sum(n1, n2, dt)
    tol = ref.default_tol(dt)
    assert info["nconv"] == k and vals.shape == (k,) and X.shape == (k, n1 * n2) and np.all(np.isfinite(vals)) and np.all(np.isfinite(X))
    err = float(np.max(np.abs(vals.astype(F64) - wanted(lam, k, which))))
    tr = _kron.true_residual(_kron.csr_double(ip, ix, d), vals, X)
    print("%s: |theta - lambda| %.3e (bound %.3e), true residual %.3e (bound %.3e), cycles %d, products %d"
          % (label, err, tol * nrm, tr, 2 * tol * nrm, info["restarts"], info["matvecs"]))
    assert err <= tol * nrm
    assert tr <= 2 * tol * nrm


@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_rotation_in_place_takes_several_trips(sa, dt):
    """LzRotate rotates the basis in place (out == V): safe because a tile's rows are read by one workgroup alone and a barrier
    stands before the LDS tile is overwritten by the next trip.  Up to 1500 rows there are at most 24 tiles and one trip.  Here
    ncv = 64: the tile and the 64 x 8 coefficient block take 66 to 68 KiB of LDS, per_cu = clamp(160 KiB / lds, 1, 8) = 2 and
    the grid is 2 num_cu; n = 40 n2 is the least with more than 3 grid tiles and a partial last one, so every workgroup makes three
    trips and one a fourth on the partial tile.  Both ends against the factors' spectra; the end recorded in
    test_eigsh_cpu.py::KRON_COUNTS also against the restatement's cycle count at this size."""
    num_cu = sa.default_ctx(0).get("num_cu")
    n2, grid = kron_n2(num_cu, dt, KRON_NCV, KRON_K)
    rows = _kron.TILE_ROWS[np.dtype(dt).name]
    n = KRON_N1 * n2
    ntile = (n + rows - 1) // rows
    assert grid == 2 * num_cu and ntile == 3 * grid + 1 and n % rows != 0
    print("n %d, %d tiles of %d rows, grid %d: 3 trips a workgroup, 4 for the first" % (n, ntile, rows, grid))
    one_cycle = KRON_NCV - ref.restart_size(KRON_K, KRON_NCV)
    recorded = KRON_COUNTS[np.dtype(dt).name][0]
    for which in ("smallest", "largest"):
        vals, X, info = _kron_solve(sa, KRON_N1, n2, dt, KRON_K, KRON_NCV, which)
        _check_big(KRON_N1, n2, dt, KRON_K, which, vals, X, info, "kron40x%d %s %s" % (n2, np.dtype(dt).name, which))
        assert info["matvecs"] == KRON_NCV + (info["restarts"] - 1) * one_cycle
        assert info["restarts"] >= 2                         # at least one restart: the in-place rotation of 64 vectors into 8 ran
        if which == recorded:
            o = kron_checker(n2, KRON_K, KRON_NCV, which, np.dtype(dt).name)
            print("cycles: GPU %d, restatement %d" % (info["restarts"], o.restarts))
            assert o.status == ref.OK and abs(info["restarts"] - o.restarts) <= 1 and abs(info["matvecs"] - o.matvecs) <= one_cycle
            assert orth_defect(X) <= max(8 * orth_defect(o.X), 64 * _eps(dt))


def test_wide_rotation_takes_several_trips(sa):
    """k = 9, ncv = 24: the restart keeps restart_size = min(k + max(k, 4), ncv - 2) = 18 columns of 24 vectors, the CB = 4 flavour
    of the rotation (q > 8); 24 KiB of tile and a 24 x 20 coefficient block make per_cu = 5, the final rotation into nine columns
    (24 x 12) 6.  In c64 (64 rows a tile, the least n for these caps) n is the least with three trips a workgroup of the larger
    grid, so more for the other, and a partial tile.  Nine pairs at the lower end: the four
    isolated ones and five from the cluster above them."""
    dt, k, m = C64, 9, 24
    p = ref.restart_size(k, m)
    assert p == 18
    num_cu = sa.default_ctx(0).get("num_cu")
    grids = [_kron.rotate_grid(num_cu, m, q, 8) for q in (p, k)]
    grid = max(g[0] for g in grids)
    n2 = _kron.n2_for_tiles(KRON_N1, 64, 3 * grid)
    n = KRON_N1 * n2
    assert [g[1] for g in grids] == [5, 6] and (n + 63) // 64 == 3 * grid + 1 and n % 64 != 0
    print("n %d, %d tiles, grids %s: at least 3 trips a workgroup" % (n, (n + 63) // 64, [g[0] for g in grids]))
    vals, X, info = _kron_solve(sa, KRON_N1, n2, dt, k, m, "smallest", max_restarts=20000)
    _check_big(KRON_N1, n2, dt, k, "smallest", vals, X, info, "kron40x%d complex128 k=9 ncv=24" % n2)
    assert info["matvecs"] == m + (m - p) * (info["restarts"] - 1) and info["restarts"] >= 2


@pytest.mark.parametrize("dt,nt", [(F64, 1), (F32, -1), (C64, -1), (C32, -1)], ids=["float64-nt", "float32", "complex128", "complex64"])
def test_fused_walk_takes_several_trips(sa, dt, nt):
    """The fused kernels of the Lanczos step (GmDots, GmUpdate, GmScale, LzNrm through launch_fused) with the "grid" knob at 8 and
    ew_chunk at 1: one workgroup an XCD walks its eighth of the packs in trips of 256.  n = 41 * 979 = 40139 is odd and 3 mod 4 (a
    scalar tail in f64, f32 and c32) and makes ceil(ceil(n / PK / 8) / 256) >= 5 trips, the last XCD's last trip partial.
    Against truth, and against the default-knob run of the same case: another summation order, so the values agree to tol |A|
    and the counts within one cycle (test_parity's allowance)."""
    n1, n2, k, m = 41, 979, 4, 30
    n = n1 * n2
    ctx = sa.default_ctx(0)
    packs = n // (16 // np.dtype(dt).itemsize)
    trips = -(-(-(-packs // 8)) // 256)                      # fused_kernel: chunk = trips * 256 packs an XCD, one workgroup each
    assert n % 2 == 1 and n % 4 == 3 and trips >= 5 and 0 < packs - 7 * trips * 256 and (packs - 7 * trips * 256) % 256 != 0
    nrm = _kron.kron_sum(n1, n2, dt)[4]
    one_cycle = m - ref.restart_size(k, m)
    g0 = ctx.get("grid")
    for which in ("smallest", "largest"):
        v0, X0, i0 = _kron_solve(sa, n1, n2, dt, k, m, which)
        ctx.set("grid", 8); ctx.set("ew_chunk", 1); ctx.set("stream_nt", nt)
        try:
            v1, X1, i1 = _kron_solve(sa, n1, n2, dt, k, m, which)
        finally:
            ctx.set("grid", g0); ctx.set("ew_chunk", -1); ctx.set("stream_nt", -1)
        print("n %d, %d trips a workgroup, %s: cycles %d (default knobs %d)" % (n, trips, which, i1["restarts"], i0["restarts"]))
        _check_big(n1, n2, dt, k, which, v1, X1, i1, "kron41x979 %s %s grid 8" % (np.dtype(dt).name, which))
        _check_big(n1, n2, dt, k, which, v0, X0, i0, "kron41x979 %s %s default" % (np.dtype(dt).name, which))
        assert np.max(np.abs(v1.astype(F64) - v0.astype(F64))) <= ref.default_tol(dt) * nrm
        assert abs(i1["restarts"] - i0["restarts"]) <= 1 and abs(i1["matvecs"] - i0["matvecs"]) <= one_cycle
        assert i1["matvecs"] == m + (i1["restarts"] - 1) * one_cycle


# ---------------------------------------------------------------------------------------------- the rotation kernel's edges
@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("km", [(4, 24), (8, 20)], ids=str)
def test_fewer_rows_than_one_tile(sa, dt, km):
    k, m = km
    for which in ("smallest", "largest"):
        vals, X, info = _solve(sa, "symband30", dt, k, m, which)
        _check_pairs("symband30", dt, k, which, vals, X, info)


@pytest.mark.parametrize("name,dt", [("poisson12x11x10", F64), ("poisson12x11x10", F32), ("hermband700", C64), ("hermband700", C32)],
                         ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_restart_keeps_all_but_two(sa, name, dt):
    """k = 9, ncv = 20: p = min(k + max(k, 4), m - 2) = m - 2 = 18, the widest rotation a basis of 20 takes."""
    assert ref.restart_size(9, 20) == 18
    for which in ("smallest", "largest"):
        vals, X, info = _solve(sa, name, dt, 9, 20, which)
        _check_pairs(name, dt, 9, which, vals, X, info)
        assert info["matvecs"] == 20 + 2 * (info["restarts"] - 1)


@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_without_vectors_and_non_temporal_flavour(sa, dt):
    """vectors=False changes nothing but X; the non-temporal flavour of the vector kernels and of the rotation gives the same
    bits as the plain one."""
    name = "hermband700" if np.dtype(dt).kind == "c" else "poisson12x11x10"
    ctx = sa.default_ctx(0)
    A, n = _handle(sa, name, dt)
    E = sa.Eigsh.new(A, n, 24)
    ctx.set("stream_nt", 0)
    plain = E.solve(4, "smallest")
    vals, X, info = E.solve(4, "smallest", vectors=False)
    assert X is None
    _same_bits((plain[0], None, plain[2]), (vals, None, info))
    ctx.set("stream_nt", 1)
    nt = E.solve(4, "smallest")
    _same_bits(plain, nt)
    _check_pairs(name, dt, 4, "smallest", *nt)
    E.close()


# ---------------------------------------------------------------------------------------------- routes, determinism
def test_every_spmv_route_gives_the_same_bits(sa):
    ctx = sa.default_ctx(0)
    runs, formats = [], []
    for knob in (0, 1, 2):
        ctx.set("spmv_dict", knob)
        A, n = _handle(sa, "poisson12x11x10", F64)
        formats.append(A.stream_format()[0])
        E = sa.Eigsh.new(A, n, 24)
        runs.append(E.solve(4, "largest"))
        E.close()
    assert formats == [0, 1, 2], formats
    _same_bits(runs[0], runs[1]); _same_bits(runs[0], runs[2])
    _check_pairs("poisson12x11x10", F64, 4, "largest", *runs[0])


@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_two_solves_and_the_device_entry_give_the_same_bits(sa, dt):
    name = "chgrid9x8" if np.dtype(dt).kind == "c" else "symband1500"
    A, n = _handle(sa, name, dt)
    E = sa.Eigsh.new(A, n, 20)
    first = E.solve(8, "largest")
    second = E.solve(8, "largest")
    _same_bits(first, second)
    other = E.solve(3, "smallest")                           # another solve in between leaves nothing behind
    assert other[2]["nconv"] == 3
    _same_bits(first, E.solve(8, "largest"))
    v0 = sa.DevVec.from_numpy(E.default_v0())
    _same_bits(first, E.solve(8, "largest", v0=v0))
    _same_bits((first[0], None, first[2]), E.solve(8, "largest", v0=v0, vectors=False))
    E.close()


# ---------------------------------------------------------------------------------------------- invariant subspaces
@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_invariant_subspace(sa, dt):
    """diag(1 .. 40), zero-based: e5 carries the entry 6 and e17 the entry 18."""
    A, n = _handle(sa, "diag40", dt)
    E = sa.Eigsh.new(A, n)
    v0 = np.zeros(40, dt); v0[5] = v0[17] = 1
    for which, want in (("largest", [18.0, 6.0]), ("smallest", [6.0, 18.0])):
        vals, X, info = E.solve(2, which, v0=v0)
        assert info["matvecs"] == 2 and info["nconv"] == 2 and info["restarts"] == 1
        assert np.allclose(vals, want, rtol=8 * _eps(dt), atol=0)
        assert np.all(np.isfinite(vals)) and np.all(np.isfinite(X)) and np.all(np.isfinite(info["res"]))
        assert true_residual(spectrum("diag40")[0], vals, X) <= 2 * ref.default_tol(dt) * 40.0
    with pytest.raises(sa.error.BreakDown) as ei:
        E.solve(3, "largest", v0=v0)
    assert ei.value.info["matvecs"] == 2 and ei.value.X is None
    e5 = np.zeros(40, dt); e5[5] = 1
    vals, X, info = E.solve(1, "smallest", v0=e5)
    assert vals[0] == 6.0 and info["matvecs"] == 1 and info["nconv"] == 1
    assert np.array_equal(np.flatnonzero(X[0]), [5]) and abs(abs(X[0, 5]) - 1.0) <= 4 * _eps(dt)
    E.close()


def test_multiple_eigenvalues_return_true_pairs(sa):
    """poisson3d(8, 8, 8) has triple eigenvalues; a single start vector finds one copy of each.  Every returned pair is an
    eigenpair to the residual bound; which copies and how many is not asserted."""
    A, lam, nrm = spectrum("poisson8x8x8")
    tol = ref.default_tol(F64)
    for which in ("smallest", "largest"):
        vals, X, info = _solve(sa, "poisson8x8x8", F64, 4, 0, which)
        assert info["nconv"] == 4
        assert true_residual(A, vals, X) <= 2 * tol * nrm
        assert all(np.min(np.abs(lam - v)) <= tol * nrm for v in vals)


# ---------------------------------------------------------------------------------------------- events and arguments
def test_one_cycle_is_not_enough(sa):
    A, n = _handle(sa, "symband1500", F64)
    E = sa.Eigsh.new(A, n, 9)
    with pytest.raises(sa.error.InsufficientIterNum) as ei:
        E.solve(3, "smallest", max_restarts=1)
    e = ei.value
    assert e.info["nconv"] < 3 and e.info["restarts"] == 1 and e.info["matvecs"] == 9 and e.iters == 1
    assert np.all(np.isfinite(e.vals)) and np.all(np.isfinite(e.X)) and np.all(np.isfinite(e.info["res"])) and e.X.shape == (3, n)
    o = ref.eigsh(*system("symband1500", F64), 3, ref.SMALLEST, ref.default_v0(n, F64), 9, 1, 1e-10)
    assert np.allclose(e.vals, o.vals, rtol=1e-9)            # the same Krylov space of nine vectors
    E.close()


@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_breakdowns(sa, dt):
    name = "chgrid9x8" if np.dtype(dt).kind == "c" else "symband30"
    ip, ix, d = system(name, dt)
    n = ip.size - 1
    bad = d.copy(); bad[3] = np.nan
    E = sa.Eigsh.new(sa.HipCsr.new((n, n), ip, ix, bad), n, 12)
    with pytest.raises(sa.error.BreakDown):
        E.solve(2, "largest")
    E.close()
    A, n = _handle(sa, name, dt)
    E = sa.Eigsh.new(A, n, 12)
    with pytest.raises(sa.error.BreakDown) as ei:
        E.solve(2, "largest", v0=np.zeros(n, dt))
    assert ei.value.info["matvecs"] == 0 and ei.value.info["restarts"] == 0
    vals, X, info = E.solve(2, "largest")                    # the handle is as good as new
    _check_pairs(name, dt, 2, "largest", vals, X, info)
    E.close()


def test_argument_checks(sa):
    from sprsolve_amd import _lib
    Lb = _lib.lib()
    E_ = sa.error
    A, n = _handle(sa, "symband30", F64)
    h = C.c_void_p()
    for ncv in (1, 2, 65, 31):                               # below 3, above 64, above n = 30
        assert Lb.sprs_eigsh_create_d(A.h, n, ncv, C.byref(h)) == _lib.INVALID_ARGUMENT and not h.value
        with pytest.raises(ValueError, match="ncv"):
            sa.Eigsh.new(A, n, ncv)
    assert Lb.sprs_eigsh_create_d(A.h, n + 1, 8, C.byref(h)) == _lib.DIM_MISMATCH and not h.value
    with pytest.raises(E_.DimensionMismatch):
        sa.Eigsh.new(A, n + 1, 8)
    assert Lb.sprs_eigsh_create_s(A.h, n, 8, C.byref(h)) == _lib.INVALID_ARGUMENT and not h.value      # another scalar type
    ip = np.array([0, 1, 2, 3], np.int32); ix = np.array([0, 1, 2], np.int32)
    rect = sa.HipCsr.new((3, 5), ip, ix, np.ones(3))
    assert Lb.sprs_eigsh_create_d(rect.h, 3, 3, C.byref(h)) == _lib.NOT_SQUARE and not h.value
    with pytest.raises(E_.IncompatibleMatrixFormat):
        sa.Eigsh.new(rect, 3, 3)
    assert sa.Eigsh.new(A, n).ncv == 30 and sa.Eigsh.new(A, n, 3).ncv == 3        # ncv = 0: min(32, n)

    E = sa.Eigsh.new(A, n, 8)
    for k in (0, 7, 8):                                      # k = 0, k = ncv - 1, k = ncv
        with pytest.raises(ValueError):
            E.solve(k)
    with pytest.raises(ValueError):
        E.solve(2, which=2)
    with pytest.raises(ValueError):
        E.solve(2, which="both")
    with pytest.raises(ValueError):
        E.solve(2, max_restarts=0)
    with pytest.raises(E_.IncompatibleMatrixFormat, match="Input vec dimension"):
        E.solve(2, v0=np.ones(n + 1))
    vals = (C.c_double * 2)(); res = (C.c_double * 2)()
    v0 = np.ones(n); X = np.zeros(2 * n + 1)
    args = lambda vl, xl: (E.h, 2, 0, v0.ctypes.data_as(C.c_void_p), vl, 500, 1e-10, vals, X.ctypes.data_as(C.c_void_p), xl, res, None, None, None)
    assert Lb.sprs_eigsh_solve_d(*args(n - 1, 2 * n)) == _lib.INCOMPATIBLE_RHS_SIZE
    assert Lb.sprs_eigsh_solve_d(*args(n, 2 * n + 1)) == _lib.INCOMPATIBLE_X_SIZE
    assert Lb.sprs_eigsh_solve_d(*args(n, 2 * n)) == _lib.OK             # the three counters may be NULL
    assert Lb.sprs_eigsh_solve_z(*args(n, 2 * n)) == _lib.INVALID_ARGUMENT       # the handle holds another scalar type
    _check_pairs("symband30", F64, 2, "largest", np.array(vals[:]), X[: 2 * n].reshape(2, n), dict(nconv=2, res=np.array(res[:])))
    E.close()
    assert Lb.sprs_eigsh_destroy(None) == 0


def test_distributed_operator_is_refused(sa):
    import torch
    from sprsolve_amd import _lib, dist as sdist
    from test_gpu_dist import _self_halo_plan
    ctx = sa.default_ctx(0)
    dev = torch.device("cuda", 0)
    comm = sdist.Comm(ctx, 0, 1)
    try:
        ip, ix, d = system("symband1500", F64)
        n = ip.size - 1
        plan = _self_halo_plan(torch, dev, n, ix, lambda c: np.zeros(c.shape, bool))
        A = sdist.DistCsr.from_plan(comm, plan, int(ip[-1]), torch.from_numpy(ip.copy()).to(dev), torch.from_numpy(d.copy()).to(dev), adopt=True,
                                    to_device=lambda a: torch.from_numpy(a).to(dev))
        h = C.c_void_p()
        st = _lib.lib().sprs_eigsh_create_d(A.h, n, 0, C.byref(h))
        text = _lib.lib().sprs_last_error(ctx.h).decode()
        assert st == _lib.INVALID_ARGUMENT and not h.value and "distributed" in text, (st, text)
        with pytest.raises(ValueError, match="distributed"):
            sa.Eigsh.new(A, n)
    finally:
        comm.close()
