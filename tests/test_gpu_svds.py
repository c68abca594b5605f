"""The truncated SVD solver on the GPU (sprs_svds_*, csrc/svds_fuse.hpp): its triplets against numpy.linalg.svd of the dense
matrix and against the numpy restatement of the recurrence (tests/_svds_ref.py), the swap for wide matrices, the edges of the
basis rotation on both bases, every SpMV route, determinism, agreement with the Lanczos eigensolver, the invariant-subspace
rule, the events and the argument checks.

The restatement's cycle and product counts (tests/test_svds_cpu.py::COUNTS holds and checks them; f64 / c64 at tol 1e-10,
f32 / c32 at 1e-4, the default start vector) range from 1 cycle of 128 products (ncv 64 on the 130 x 67 matrices) to 215 cycles of
four products (lsmr600x400, k = 1, ncv 3, largest, c64).  1500 and 700 rows leave a partial last tile in every scalar type (a tile
is 64 rows of c64, 128 of f64 / c32, 256 of f32), 30 and 20 are less than one tile."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kron  # noqa: E402
import _svds_ref as ref  # noqa: E402
from test_svds_cpu import CASES, _id, checker, count, orth_defect, spectrum_of, system, true_residuals, wanted  # noqa: E402

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = [F64, C64, F32, C32]
_KNOBS = ("spmv_dict", "stream_nt", "ew_chunk")
_dtid = lambda d: np.dtype(d).name


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
    shape, ip, ix, d = system(name, dt)
    return sa.HipCsr.new(shape, ip, ix, d)


def _solve(sa, name, dt, k, m, which, **kw):
    S = sa.Svds.new(_handle(sa, name, dt), m)
    try:
        return S.solve(k, which, **kw)
    finally:
        S.close()


def _check_triplets(name, dt, k, which, s, U, V, info, tol=None):
    """The issue's bounds: |sigma_i - sigma_i(dense)| <= tol |A|_2 and both true residuals, formed in double, <= 2 tol |A|_2."""
    A, sv = spectrum_of(name, dt)
    nrm = float(sv[0])
    tol = ref.default_tol(dt) if tol is None else tol
    assert info["nconv"] == k and s.shape == (k,) and U.shape == (k, A.shape[0]) and V.shape == (k, A.shape[1])
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(U)) and np.all(np.isfinite(V)) and np.all(np.isfinite(info["res"]))
    err = float(np.max(np.abs(s.astype(F64) - wanted(sv, k, which))))
    r1, r2 = true_residuals(A, s, U, V)
    print("%s %s k=%d %s: |sigma - dense| %.3e, |A v - s u| %.3e, |A^H u - s v| %.3e, tol |A| %.3e" % (name, np.dtype(dt).name, k, which, err, r1, r2, tol * nrm))
    assert err <= tol * nrm
    assert r1 <= 2 * tol * nrm and r2 <= 2 * tol * nrm


def _same_bits(a, b):
    (sa_, Ua, Va, ia), (sb, Ub, Vb, ib) = a, b
    assert np.array_equal(sa_.view(np.uint8), sb.view(np.uint8))
    assert np.array_equal(ia["res"].view(np.uint8), ib["res"].view(np.uint8))
    for Xa, Xb in ((Ua, Ub), (Va, Vb)):
        assert (Xa is None) == (Xb is None)
        if Xa is not None:
            assert np.array_equal(Xa.view(np.uint8), Xb.view(np.uint8))
    assert (ia["nconv"], ia["restarts"], ia["matvecs"]) == (ib["nconv"], ib["restarts"], ib["matvecs"])


def _no_vectors(r):
    return (r[0], None, None, r[3])


# ---------------------------------------------------------------------------------------------- parity with the mathematics
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_parity(sa, case):
    name, k, m, which, dt = case
    o = checker(name, k, m, which, np.dtype(dt).name)
    s, U, V, info = _solve(sa, name, dt, k, m, which)
    _check_triplets(name, dt, k, which, s, U, V, info)
    assert orth_defect(U) <= max(8 * orth_defect(o.U), 64 * _eps(dt))
    assert orth_defect(V) <= max(8 * orth_defect(o.V), 64 * _eps(dt))
    want = count(name, k, m, which, dt)
    one_cycle = 2 * (m - ref.restart_size(k, m))
    # a residual estimate that sits on the threshold may fall either way under another summation order
    assert abs(info["matvecs"] - want[1]) <= one_cycle and abs(info["restarts"] - want[0]) <= 1, (info, want)
    assert info["matvecs"] == 2 * m + (info["restarts"] - 1) * one_cycle


@pytest.mark.parametrize("dt", ALL, ids=_dtid)
def test_a_wide_matrix_swaps_the_operators(sa, dt):
    """67 x 130: Op = A^H, the start vector has 67 entries, U comes from the small basis and V from the large one."""
    S = sa.Svds.new(_handle(sa, "lsmr67x130", dt), 24)
    assert S.default_v0().shape == (67,)
    for which in ("largest", "smallest"):
        s, U, V, info = S.solve(4, which)
        assert U.shape == (4, 67) and V.shape == (4, 130)
        _check_triplets("lsmr67x130", dt, 4, which, s, U, V, info)
    S.close()


# ---------------------------------------------------------------------------------------------- several tiles a workgroup
def _kron_solve(sa, dims, dt, k, m, **kw):
    ip, ix, d, _, shape = _kron.kron_product(*dims, dt)
    S = sa.Svds.new(sa.HipCsr.new(shape, ip, ix, d), m)
    try:
        return S.solve(k, "largest", **kw)
    finally:
        S.close()


def _check_big(dims, dt, k, s, U, V, info, label):
    """The bounds of _check_triplets on kron_product(*dims): truth is the products of the factors' singular values, both true
    residuals are formed in double."""
    ip, ix, d, sv, shape = _kron.kron_product(*dims, dt)
    A = _kron.csr_double(ip, ix, d, shape)
    nrm, tol = float(sv[0]), ref.default_tol(dt)
    assert info["nconv"] == k and s.shape == (k,) and U.shape == (k, shape[0]) and V.shape == (k, shape[1])
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(U)) and np.all(np.isfinite(V))
    wd = C64 if np.dtype(dt).kind == "c" else F64
    Uw, Vw = U.astype(wd), V.astype(wd)
    AH = A.conj().T.tocsr()
    err = float(np.max(np.abs(s.astype(F64) - sv[:k])))
    r1 = max(float(np.linalg.norm(A @ Vw[i] - float(s[i]) * Uw[i])) for i in range(k))
    r2 = max(float(np.linalg.norm(AH @ Uw[i] - float(s[i]) * Vw[i])) for i in range(k))
    print("%s: |sigma - truth| %.3e (bound %.3e), |A v - s u| %.3e, |A^H u - s v| %.3e (bound %.3e), cycles %d, products %d"
          % (label, err, tol * nrm, r1, r2, 2 * tol * nrm, info["restarts"], info["matvecs"]))
    assert err <= tol * nrm
    assert r1 <= 2 * tol * nrm and r2 <= 2 * tol * nrm


def _past_the_cap(num_cu, dt, wide):
    """kron_product dims whose short side has 3 grid + 1 tiles, the last partial, for the rotation's grid at ncv = 64, k = 6
    (launch_lz_rotate: 2 num_cu, as in tests/test_gpu_eigsh.py) and whose long side has more, also with a partial tile."""
    rows = _kron.TILE_ROWS[np.dtype(dt).name]
    grid = max(_kron.rotate_grid(num_cu, 64, q, ref.real_dtype(dt).itemsize)[0] for q in (ref.restart_size(6, 64), 6))
    short = _kron.n2_for_tiles(37, rows, 3 * grid)
    long_ = short + 5
    while (40 * long_) % rows == 0:
        long_ += 1
    dims = (37, 40, short, long_) if wide else (40, 37, long_, short)
    return dims, grid, rows


@pytest.mark.parametrize("dt,wide", [(C64, False), (F64, True), (F32, False), (C32, True)],
                         ids=["complex128-tall", "float64-wide", "float32-tall", "complex64-wide"])
def test_rotations_in_place_take_several_trips(sa, dt, wide):
    """Both bases are rotated in place by LzRotate: at every restart (64 vectors into restart_size = 12 columns, CB = 4) and at
    the end of every solve (m_eff vectors into k columns).  With ncv = 64 its grid is 2 num_cu; M and N are both past 3 grid tiles
    with partial last tiles, so every workgroup makes at least three trips on either basis.  A wide matrix swaps the operators:
    the long basis is then the other one.  The six largest triplets (6, 4.5, 4.4, 3.3, 3.2, 2.4 before the off-diagonals, over a
    cluster that ends at 2) against the products of the factors' singular values; the cycle count is printed — with one cycle only
    the final rotation ran."""
    num_cu = sa.default_ctx(0).get("num_cu")
    dims, grid, rows = _past_the_cap(num_cu, dt, wide)
    M, N = dims[0] * dims[2], dims[1] * dims[3]
    tM, tN = (M + rows - 1) // rows, (N + rows - 1) // rows
    assert grid == 2 * num_cu and min(tM, tN) == 3 * grid + 1 and M % rows != 0 and N % rows != 0 and (M < N) == wide
    print("%d x %d, tiles of %d rows: %d and %d, grid %d: at least 3 trips a workgroup on both bases" % (M, N, rows, tM, tN, grid))
    s, U, V, info = _kron_solve(sa, dims, dt, 6, 64)
    _check_big(dims, dt, 6, s, U, V, info, "kron %dx%d %s" % (M, N, np.dtype(dt).name))
    one_cycle = 2 * (64 - ref.restart_size(6, 64))
    assert info["matvecs"] == 2 * 64 + (info["restarts"] - 1) * one_cycle and info["restarts"] >= 1
    assert orth_defect(U) <= 4 * 64 * (info["restarts"] + 1) * _eps(dt) and orth_defect(V) <= 4 * 64 * (info["restarts"] + 1) * _eps(dt)


@pytest.mark.parametrize("dt,nt", [(F64, -1), (F32, -1), (C64, 1), (C32, -1)], ids=["float64", "float32", "complex128-nt", "complex64"])
def test_fused_walk_takes_several_trips(sa, dt, nt):
    """The fused kernels of the bidiagonalisation step with the "grid" knob at 8 and ew_chunk at 1: one workgroup an XCD walks its
    eighth of the packs in trips of 256.  40139 x 36149 (41 * 979 and 37 * 977: both odd, M = 3 mod 4, scalar tails on both sides)
    makes at least five trips on either side, the last XCD's last trip partial.  Against truth, and against the default-knob run:
    another summation order, so the values agree to tol |A| and the counts within one cycle (test_parity's allowance)."""
    dims, k, m = (41, 37, 979, 977), 4, 12                   # a short basis: several cycles, so restarts run under the walk too
    M, N = dims[0] * dims[2], dims[1] * dims[3]
    ctx = sa.default_ctx(0)
    for n in (M, N):
        packs = n // (16 // np.dtype(dt).itemsize)
        trips = -(-(-(-packs // 8)) // 256)
        assert n % 2 == 1 and trips >= 5 and 0 < packs - 7 * trips * 256 and (packs - 7 * trips * 256) % 256 != 0
    assert M % 4 == 3
    nrm = float(_kron.kron_product(*dims, dt)[3][0])
    one_cycle = 2 * (m - ref.restart_size(k, m))
    g0 = ctx.get("grid")
    r0 = _kron_solve(sa, dims, dt, k, m)
    ctx.set("grid", 8); ctx.set("ew_chunk", 1); ctx.set("stream_nt", nt)
    try:
        r1 = _kron_solve(sa, dims, dt, k, m)
    finally:
        ctx.set("grid", g0); ctx.set("ew_chunk", -1); ctx.set("stream_nt", -1)
    print("%d x %d, %d trips a workgroup on the short side: cycles %d (default knobs %d)" % (M, N, trips, r1[3]["restarts"], r0[3]["restarts"]))
    _check_big(dims, dt, k, *r1, "kron %dx%d %s grid 8" % (M, N, np.dtype(dt).name))
    _check_big(dims, dt, k, *r0, "kron %dx%d %s default" % (M, N, np.dtype(dt).name))
    assert np.max(np.abs(r1[0].astype(F64) - r0[0].astype(F64))) <= ref.default_tol(dt) * nrm
    assert abs(r1[3]["restarts"] - r0[3]["restarts"]) <= 1 and abs(r1[3]["matvecs"] - r0[3]["matvecs"]) <= one_cycle
    assert r1[3]["matvecs"] == 2 * m + (r1[3]["restarts"] - 1) * one_cycle


# ---------------------------------------------------------------------------------------------- the rotation kernel's edges
@pytest.mark.parametrize("dt", ALL, ids=_dtid)
@pytest.mark.parametrize("km", [(4, 12), (6, 20)], ids=str)
def test_fewer_rows_than_one_tile_on_either_side(sa, dt, km):
    """30 x 20; ncv = 20 spans the whole small space, so the last step meets the invariant subspace."""
    k, m = km
    for which in ("smallest", "largest"):
        s, U, V, info = _solve(sa, "lsmr30x20", dt, k, m, which)
        _check_triplets("lsmr30x20", dt, k, which, s, U, V, info)


@pytest.mark.parametrize("dt", ALL, ids=_dtid)
def test_partial_last_tiles_on_both_sides(sa, dt):
    s, U, V, info = _solve(sa, "graded1500x700", dt, 4, 24, "largest")
    _check_triplets("graded1500x700", dt, 4, "largest", s, U, V, info)


@pytest.mark.parametrize("name,dt,ends", [("lsmr600x400", F64, ("largest",)), ("lsmr600x400", F32, ("largest",)),
                                          ("lsmr130x67", C64, ("largest", "smallest")), ("lsmr130x67", C32, ("largest", "smallest"))],
                         ids=lambda v: v if isinstance(v, str) else (np.dtype(v).name if not isinstance(v, tuple) else "-".join(v)))
def test_restart_keeps_all_but_two(sa, name, dt, ends):
    """k = 9, ncv = 20: p = min(k + max(k, 4), l - 2) = l - 2 = 18, the widest rotation a basis of 20 takes."""
    assert ref.restart_size(9, 20) == 18
    for which in ends:
        s, U, V, info = _solve(sa, name, dt, 9, 20, which)
        _check_triplets(name, dt, 9, which, s, U, V, info)
        assert info["matvecs"] == 40 + 4 * (info["restarts"] - 1)


# ---------------------------------------------------------------------------------------------- routes, determinism
@pytest.mark.parametrize("dt", ALL, ids=_dtid)
def test_without_vectors_and_non_temporal_flavour(sa, dt):
    """vectors=False changes nothing but U and V; the non-temporal flavour of the vector kernels and of the rotation gives the
    same bits as the plain one."""
    ctx = sa.default_ctx(0)
    S = sa.Svds.new(_handle(sa, "lsmr600x400", dt), 24)
    ctx.set("stream_nt", 0)
    plain = S.solve(4, "smallest")
    r = S.solve(4, "smallest", vectors=False)
    assert r[1] is None and r[2] is None
    _same_bits(_no_vectors(plain), r)
    ctx.set("stream_nt", 1)
    nt = S.solve(4, "smallest")
    _same_bits(plain, nt)
    _check_triplets("lsmr600x400", dt, 4, "smallest", *nt)
    S.close()


def test_every_spmv_route_gives_the_same_bits(sa):
    ctx = sa.default_ctx(0)
    runs, formats = [], []
    for knob in (0, 1, 2):
        ctx.set("spmv_dict", knob)
        A = _handle(sa, "poisson12x11x10", F64)
        formats.append(A.stream_format()[0])
        S = sa.Svds.new(A, 24)
        runs.append(S.solve(4, "largest"))
        S.close()
    assert formats == [0, 1, 2], formats
    _same_bits(runs[0], runs[1]); _same_bits(runs[0], runs[2])
    _check_triplets("poisson12x11x10", F64, 4, "largest", *runs[0])


@pytest.mark.parametrize("dt", ALL, ids=_dtid)
def test_two_solves_the_adjoint_handle_and_the_device_entry_give_the_same_bits(sa, dt):
    A = _handle(sa, "lsmr130x67", dt)
    S = sa.Svds.new(A, 20)
    first = S.solve(8, "largest")
    _same_bits(first, S.solve(8, "largest"))
    other = S.solve(3, "smallest")                           # another solve in between leaves nothing behind
    assert other[3]["nconv"] == 3
    _same_bits(first, S.solve(8, "largest"))
    v0 = sa.DevVec.from_numpy(S.default_v0())
    _same_bits(first, S.solve(8, "largest", v0=v0))
    _same_bits(_no_vectors(first), S.solve(8, "largest", v0=v0, vectors=False))
    S.close()
    AH = A.adjoint()
    S2 = sa.Svds.new(A, 20, adjoint=AH)                      # the caller's adjoint handle, borrowed
    _same_bits(first, S2.solve(8, "largest"))
    S2.close()
    x = sa.DevVec.from_numpy(np.ones(130, dt)); y = sa.DevVec.from_numpy(np.zeros(67, dt))
    AH.mul_vec_unchecked(x, y)                               # the borrowed handle outlives the solver
    yh = y.to_numpy()
    assert AH.shape == (67, 130) and np.all(np.isfinite(yh)) and np.any(yh != 0)


def test_agreement_with_the_lanczos_eigensolver(sa):
    """A Hermitian positive-definite matrix: its singular values are its eigenvalues."""
    A = _handle(sa, "poisson12x11x10", F64)
    n = A.shape[0]
    s, U, V, info = sa.Svds.new(A, 24).solve(4, "largest")
    E = sa.Eigsh.new(A, n, 24)
    theta, X, einfo = E.solve(4, "largest")
    E.close()
    nrm = float(spectrum_of("poisson12x11x10", F64)[1][0])
    print("sigma", s, "theta", theta)
    assert np.max(np.abs(s - theta)) <= 2 * ref.default_tol(F64) * nrm
    _check_triplets("poisson12x11x10", F64, 4, "largest", s, U, V, info)


# ---------------------------------------------------------------------------------------------- invariant subspaces, events
@pytest.mark.parametrize("dt", ALL, ids=_dtid)
def test_invariant_subspace(sa, dt):
    """50 x 40, A[i, i] = i + 1, zero-based: e5 carries the entry 6 and e17 the entry 18."""
    S = sa.Svds.new(_handle(sa, "diag50x40", dt))
    v0 = np.zeros(40, dt); v0[5] = v0[17] = 1
    for which, want in (("largest", [18.0, 6.0]), ("smallest", [6.0, 18.0])):
        s, U, V, info = S.solve(2, which, v0=v0)
        assert info["matvecs"] == 4 and info["nconv"] == 2 and info["restarts"] == 1
        assert np.allclose(s, want, rtol=8 * _eps(dt), atol=0)
        assert np.all(info["res"] == 0)
        assert U.shape == (2, 50) and V.shape == (2, 40) and np.all(np.isfinite(U)) and np.all(np.isfinite(V))
        r1, r2 = true_residuals(spectrum_of("diag50x40", dt)[0], s, U, V)
        assert r1 <= 2 * ref.default_tol(dt) * 40.0 and r2 <= 2 * ref.default_tol(dt) * 40.0
    with pytest.raises(sa.error.BreakDown) as ei:
        S.solve(3, "largest", v0=v0)
    assert ei.value.info["matvecs"] == 4 and ei.value.U is None and ei.value.V is None
    S.close()


def test_one_cycle_is_not_enough(sa):
    S = sa.Svds.new(_handle(sa, "lsmr600x400", F64), 9)
    with pytest.raises(sa.error.InsufficientIterNum) as ei:
        S.solve(3, "smallest", max_restarts=1)
    e = ei.value
    assert e.info["nconv"] < 3 and e.info["restarts"] == 1 and e.info["matvecs"] == 18 and e.iters == 1
    assert np.all(np.isfinite(e.s)) and np.all(np.isfinite(e.U)) and np.all(np.isfinite(e.V)) and np.all(np.isfinite(e.info["res"]))
    assert e.U.shape == (3, 600) and e.V.shape == (3, 400)
    shape, ip, ix, d = system("lsmr600x400", F64)
    o = ref.svds(shape, ip, ix, d, 3, ref.SMALLEST, ref.default_v0(shape, F64), 9, 1, 1e-10)
    assert np.allclose(e.s, o.s, rtol=1e-9)                  # the same Krylov spaces of nine vectors
    S.close()


@pytest.mark.parametrize("dt", ALL, ids=_dtid)
def test_breakdowns(sa, dt):
    """A NaN in A ends in BreakDown, not a hang: `skip` stops the blind launches.  A zero start vector is a breakdown before any
    product, and the handle is as good as new after either."""
    shape, ip, ix, d = system("lsmr30x20", dt)
    bad = d.copy(); bad[3] = np.nan
    S = sa.Svds.new(sa.HipCsr.new(shape, ip, ix, bad), 12)
    with pytest.raises(sa.error.BreakDown) as ei:
        S.solve(2, "largest")
    assert ei.value.U is None and ei.value.info["restarts"] <= 1 and ei.value.info["matvecs"] <= 2
    S.close()
    S = sa.Svds.new(_handle(sa, "lsmr30x20", dt), 12)
    with pytest.raises(sa.error.BreakDown) as ei:
        S.solve(2, "largest", v0=np.zeros(20, dt))
    assert ei.value.info["matvecs"] == 0 and ei.value.info["restarts"] == 0
    s, U, V, info = S.solve(2, "largest")
    _check_triplets("lsmr30x20", dt, 2, "largest", s, U, V, info)
    S.close()


def test_argument_checks(sa):
    from sprsolve_amd import _lib
    Lb = _lib.lib()
    E_ = sa.error
    ctx = sa.default_ctx(0)
    A = _handle(sa, "lsmr30x20", F64)
    rows, cols = 30, 20
    h = C.c_void_p()
    for ncv in (1, 2, 65, 21):                               # below 3, above 64, above min(rows, cols) = 20
        assert Lb.sprs_svds_create_d(A.h, None, ncv, C.byref(h)) == _lib.INVALID_ARGUMENT and not h.value
        assert b"ncv" in Lb.sprs_last_error(ctx.h)
        with pytest.raises(ValueError, match="ncv"):
            sa.Svds.new(A, ncv)
    assert Lb.sprs_svds_create_s(A.h, None, 8, C.byref(h)) == _lib.INVALID_ARGUMENT and not h.value      # another scalar type
    assert Lb.sprs_svds_create_d(A.h, A.h, 8, C.byref(h)) == _lib.INVALID_ARGUMENT and not h.value       # an "adjoint" of 30 x 20
    assert b"adjoint" in Lb.sprs_last_error(ctx.h)
    with pytest.raises(ValueError, match="adjoint"):
        sa.Svds.new(A, 8, adjoint=A)
    AHs = _handle(sa, "lsmr30x20", F32).adjoint()
    assert Lb.sprs_svds_create_d(A.h, AHs.h, 8, C.byref(h)) == _lib.INVALID_ARGUMENT and not h.value     # an adjoint of another type
    assert b"adjoint" in Lb.sprs_last_error(ctx.h)
    assert sa.Svds.new(A).ncv == 20 and sa.Svds.new(A, 3).ncv == 3               # ncv = 0: min(32, rows, cols)

    S = sa.Svds.new(A, 8)
    for k in (0, 7, 8):                                      # k = 0, k = ncv - 1, k = ncv
        with pytest.raises(ValueError):
            S.solve(k)
    with pytest.raises(ValueError):
        S.solve(2, which=2)
    with pytest.raises(ValueError):
        S.solve(2, which="both")
    with pytest.raises(ValueError):
        S.solve(2, max_restarts=0)
    with pytest.raises(E_.IncompatibleMatrixFormat, match="Input vec dimension"):
        S.solve(2, v0=np.ones(rows))                         # the start vector lives in the small space
    vals = (C.c_double * 2)(); res = (C.c_double * 2)()
    v0 = np.ones(cols); U = np.zeros(2 * rows + 1); V = np.zeros(2 * cols + 1)
    up, vp = U.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p)
    args = lambda vl, u, ul, v, vvl: (S.h, 2, 0, v0.ctypes.data_as(C.c_void_p), vl, 500, 1e-10, vals, u, ul, v, vvl, res, None, None, None)
    assert Lb.sprs_svds_solve_d(*args(cols - 1, up, 2 * rows, vp, 2 * cols)) == _lib.INCOMPATIBLE_RHS_SIZE
    assert Lb.sprs_svds_solve_d(*args(cols, up, 2 * rows + 1, vp, 2 * cols)) == _lib.INCOMPATIBLE_X_SIZE
    assert Lb.sprs_svds_solve_d(*args(cols, up, 2 * rows, vp, 2 * cols + 1)) == _lib.INCOMPATIBLE_X_SIZE
    assert Lb.sprs_svds_solve_d(*args(cols, up, 2 * rows, None, 2 * cols)) == _lib.INVALID_ARGUMENT          # one vector block without the other
    assert Lb.sprs_svds_solve_d(*args(cols, None, 2 * rows, vp, 2 * cols)) == _lib.INVALID_ARGUMENT
    assert Lb.sprs_svds_solve_z(*args(cols, up, 2 * rows, vp, 2 * cols)) == _lib.INVALID_ARGUMENT            # the handle holds another scalar type
    assert Lb.sprs_svds_solve_d(*args(cols, up, 2 * rows, vp, 2 * cols)) == _lib.OK                          # the three counters may be NULL
    _check_triplets("lsmr30x20", F64, 2, "largest", np.array(vals[:]), U[: 2 * rows].reshape(2, rows), V[: 2 * cols].reshape(2, cols),
                    dict(nconv=2, res=np.array(res[:])))
    assert Lb.sprs_svds_solve_d(*args(cols, None, 0, None, 0)) == _lib.OK                                    # no vectors at all
    S.close()
    assert Lb.sprs_svds_destroy(None) == 0


def test_distributed_operator_is_refused(sa):
    import torch
    from sprsolve_amd import _lib, dist as sdist
    from test_gpu_dist import _self_halo_plan
    from test_eigsh_cpu import system as esystem
    ctx = sa.default_ctx(0)
    dev = torch.device("cuda", 0)
    comm = sdist.Comm(ctx, 0, 1)
    try:
        ip, ix, d = esystem("symband1500", F64)
        n = ip.size - 1
        plan = _self_halo_plan(torch, dev, n, ix, lambda c: np.zeros(c.shape, bool))
        A = sdist.DistCsr.from_plan(comm, plan, int(ip[-1]), torch.from_numpy(ip.copy()).to(dev), torch.from_numpy(d.copy()).to(dev), adopt=True,
                                    to_device=lambda a: torch.from_numpy(a).to(dev))
        h = C.c_void_p()
        st = _lib.lib().sprs_svds_create_d(A.h, None, 0, C.byref(h))
        text = _lib.lib().sprs_last_error(ctx.h).decode()
        assert st == _lib.INVALID_ARGUMENT and not h.value and "distributed" in text, (st, text)
        with pytest.raises(ValueError, match="distributed"):
            sa.Svds.new(A)
    finally:
        comm.close()
