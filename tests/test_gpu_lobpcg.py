"""The LOBPCG eigensolver on the GPU (sprs_lobpcg_*, csrc/lobpcg_fuse.hpp): its pairs against numpy.linalg.eigvalsh of the dense
matrix, its iteration counts capped by the numpy restatement of the recurrence (tests/_lobpcg_ref.py), every preconditioner, the
edges of the Gram and rotation kernels, multiple eigenvalues, determinism over routes and flavours, the events and the argument
checks.

The restatement's counts (tests/test_lobpcg_cpu.py::COUNTS holds and checks them; f64 / c64 at tol 1e-10, f32 / c32 at 1e-4, the
default start block) range from 11 iterations (chgrid9x8, (4, 8), largest, c32) to 167 (poisson12x11x10, (1, 1), smallest, f64).
A GPU run may take up to 4 times the restatement's count: a cap, not a parity claim — summation order alone moved the
restatement's own single-precision counts by a factor of 2.  n = 1320 and 1500 leave a partial last tile in every scalar type (a
tile is 64 rows of c64, 128 of f64 / c32, 256 of f32), n = 72 and n = 30 are less than one tile.

The Kronecker family of tests/_kron.py (isolated extreme eigenvalues over a cluster, truth from the factors' spectra) carries the
cases the small matrices cannot: early convergence of the leading columns (soft locking, anorm), and sizes computed from the
device's CU count at which every walker of the Gram kernel takes several tiles and the fused residual kernel several trips."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kron  # noqa: E402
import _lobpcg_ref as ref  # noqa: E402
from test_eigsh_cpu import orth_defect, spectrum, system, true_residual, wanted  # noqa: E402
from test_lobpcg_cpu import (CASES, EDGE_CASES, KRON_CASES, KRON_N1, _id, _kron_id, check_kron_pairs, checker, count, is_single, kron_checker,  # noqa: E402
                             kron_X0)

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = [F64, C64, F32, C32]
_KNOBS = ("spmv_dict", "stream_nt", "ew_chunk")
_ids = lambda v: v if isinstance(v, str) else np.dtype(v).name


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


def _solve(sa, name, dt, k, b, which, **kw):
    A, n = _handle(sa, name, dt)
    S = sa.Lobpcg.new(A, n, b)
    try:
        return S.solve(k, which, **kw)
    finally:
        S.close()


def _check_pairs(name, dt, k, which, vals, X, info, tol=None):
    """The issue's bounds: |theta_i - lambda_i| <= tol |A|_2 and the true residual, formed in double from X, <= 2 tol |A|_2."""
    A, lam, nrm = spectrum(name)
    tol = ref.default_tol(dt) if tol is None else tol
    assert info["nconv"] == k and vals.shape == (k,) and X.shape == (k, A.shape[0])
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(X)) and np.all(np.isfinite(info["res"]))
    err = float(np.max(np.abs(vals.astype(F64) - wanted(lam, k, which))))
    tr = true_residual(A, vals, X)
    print("%s %s k=%d %s: |theta - lambda| %.3e, true residual %.3e, tol |A| %.3e, iters %d, restarts %d"
          % (name, np.dtype(dt).name, k, which, err, tr, tol * nrm, info.get("iters", -1), info.get("restarts", -1)))
    assert err <= tol * nrm
    assert tr <= 2 * tol * nrm


def _same_bits(a, b):
    (va, Xa, ia), (vb, Xb, ib) = a, b
    assert np.array_equal(va.view(np.uint8), vb.view(np.uint8))
    assert np.array_equal(ia["res"].view(np.uint8), ib["res"].view(np.uint8))
    assert (Xa is None) == (Xb is None)
    if Xa is not None:
        assert np.array_equal(Xa.view(np.uint8), Xb.view(np.uint8))
    assert all(ia[f] == ib[f] for f in ("nconv", "iters", "restarts", "matvecs"))


def _parity(sa, case):
    name, k, b, which, dt = case
    o = checker(name, k, b, which, np.dtype(dt).name)
    want = count(name, k, b, which, dt)
    vals, X, info = _solve(sa, name, dt, k, b, which, max_iter=4 * want[0])      # more than that: InsufficientIterNum
    print("iterations: GPU %d (fallbacks %d), restatement %d (fallbacks %d)" % (info["iters"], info["restarts"], want[0], want[1]))
    _check_pairs(name, dt, k, which, vals, X, info)
    assert orth_defect(X) <= max(8 * orth_defect(o.X), 64 * _eps(dt))
    assert info["matvecs"] == b * (info["iters"] + 1)


# ---------------------------------------------------------------------------------------------- parity with the mathematics
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_parity(sa, case):
    """b = 8 in c64 is the widest Gram (48 KiB of tile, the two triangles split over two workgroups); b = 1 gives m = 3, an odd
    Jacobi size."""
    _parity(sa, case)


# ---------------------------------------------------------------------------------------------- the kernels' edges
@pytest.mark.parametrize("case", EDGE_CASES, ids=_id)
def test_fewer_rows_than_one_tile(sa, case):
    _parity(sa, case)


# ---------------------------------------------------------------------------------------------- isolated extreme eigenvalues
_STATUS = {"InsufficientIterNum": ref.INSUFFICIENT_ITER, "BreakDown": ref.BREAKDOWN}


def _kron_solve(sa, n1, n2, dt, k, b, which, **kw):
    """-> (status, vals, X, info) of one solve on kron_sum(n1, n2): an event comes back as its status, not as an exception."""
    ip, ix, d, _, _ = _kron.kron_sum(n1, n2, dt)
    n = ip.size - 1
    S = sa.Lobpcg.new(sa.HipCsr.new((n, n), ip, ix, d), n, b)
    try:
        return (ref.OK,) + tuple(S.solve(k, which, **kw))
    except (sa.error.InsufficientIterNum, sa.error.BreakDown) as e:
        return _STATUS[type(e).__name__], e.vals, e.X, e.info
    finally:
        S.close()


@pytest.mark.parametrize("case", KRON_CASES, ids=_kron_id)
def test_isolated_extreme_eigenvalues(sa, case):
    """kron_sum(40, n2) (tests/test_lobpcg_cpu.py): the leading columns converge long before the others and are soft-locked.  A
    solve that says OK holds the bounds of _check_pairs against the factors' spectra; where the restatement converges the GPU run
    must, within 4 times its iterations (test_parity's cap)."""
    n2, which, dt, x0 = case
    o = kron_checker(n2, which, np.dtype(dt).name, x0)
    n = KRON_N1 * n2
    max_iter = 4 * o.iters if o.status == ref.OK else 400
    status, vals, X, info = _kron_solve(sa, KRON_N1, n2, dt, 4, 8, which, max_iter=max_iter, X0=None if x0 == "default" else kron_X0(n, 8, dt, x0))
    print("iterations: GPU %d (fallbacks %d, status %d), restatement %d (fallbacks %d, status %d)"
          % (info["iters"], info["restarts"], status, o.iters, o.restarts, o.status))
    ok = check_kron_pairs(n2, dt, 4, which, status, vals, X, _kron_id(case))
    assert ok or o.status != ref.OK
    if ok:
        assert info["nconv"] == 4 and info["matvecs"] == 8 * (info["iters"] + 1)
        assert orth_defect(X) <= 64 * _eps(dt)


# ---------------------------------------------------------------------------------------------- more than one tile a workgroup
def gram_walkers(num_cu, dt, m):
    """Lobpcg::gram's launch rule (csrc/lobpcg.hip): entry blocks of R x R (R = 4; 2 in c64), MB = ceil(m / R) block rows,
    nb1 = MB (MB + 1) / 2 blocks a triangle, 8 wavefronts; one workgroup holds both triangles when ceil(2 nb1 / 8) <= NBL (6; c64:
    10; c32: 3), else two share them (nsplit = 2); the small flavour (blocks a wavefront <= NBS = 2; c64: 3) runs two workgroups a
    CU.  -> (the cap on the walkers GW = min(num_cu per_cu / nsplit, 512), nsplit, per_cu)."""
    dt = np.dtype(dt)
    R = 2 if dt == np.dtype(C64) else 4
    NBL = {np.dtype(F64): 6, np.dtype(F32): 6, np.dtype(C32): 3, np.dtype(C64): 10}[dt]
    NBS = 3 if dt == np.dtype(C64) else 2
    MB = (m + R - 1) // R
    nb1 = MB * (MB + 1) // 2
    nsplit = 1 if (2 * nb1 + 7) // 8 <= NBL else 2
    need = ((2 * nb1 if nsplit == 1 else nb1) + 7) // 8
    per_cu = 2 if need <= NBS else 1
    return min(num_cu * per_cu // nsplit, 512), nsplit, per_cu


def _check_big(n1, n2, dt, k, which, vals, X, label):
    """The bounds of _check_pairs on kron_sum(n1, n2): truth from the factors' spectra, the true residual in double."""
    ip, ix, d, lam, nrm = _kron.kron_sum(n1, n2, dt)
    tol = ref.default_tol(dt)
    assert vals.shape == (k,) and X.shape == (k, n1 * n2) and np.all(np.isfinite(vals)) and np.all(np.isfinite(X))
    err = float(np.max(np.abs(vals.astype(F64) - wanted(lam, k, which))))
    tr = _kron.true_residual(_kron.csr_double(ip, ix, d), vals, X)
    print("%s: |theta - lambda| %.3e (bound %.3e), true residual %.3e (bound %.3e)" % (label, err, tol * nrm, tr, 2 * tol * nrm))
    assert err <= tol * nrm
    assert tr <= 2 * tol * nrm


@pytest.mark.parametrize("block", [8, 2])
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_gram_walk_takes_several_tiles(sa, dt, block):
    """LobGram's walkers fold tile t while tile t + GW lands in the other LDS buffer.  With at most 24 tiles (n <= 1500) every
    walker has one tile and the prefetch, the buffer flip and the whole / partial switch inside a walk never run.  Here
    n = 40 n2 is the least with ntile > 3.5 GW for the widest pass (m = 3 b; m = 2 b at the first iteration has the same or a
    larger cap, so it is asserted too) and n no multiple of the tile: every walker takes 3 or 4 tiles, both buffers are
    prefetched into, and the last tile is partial.  Block 8 is the wide register flavour (nsplit = 2 in c64 and c32), block 2
    the small one with two workgroups a CU.  The numpy restatement is not run at this size: truth is the factors' spectra."""
    num_cu = sa.default_ctx(0).get("num_cu")
    rows = _kron.TILE_ROWS[np.dtype(dt).name]
    caps = [gram_walkers(num_cu, dt, mm * block) for mm in (3, 2)]
    GW = max(c[0] for c in caps)
    n2 = _kron.n2_for_tiles(KRON_N1, rows, (7 * GW + 1) // 2)
    n = KRON_N1 * n2
    ntile = (n + rows - 1) // rows
    assert n % rows != 0 and all(ntile >= 3 * c[0] + 1 for c in caps) and ntile > 24
    if block == 8:
        assert caps[0][1] == (2 if np.dtype(dt).kind == "c" else 1) and caps[0][2] == 1
    else:
        assert caps[0][1] == 1 and caps[0][2] == 2
    k = 4 if block == 8 else 1
    print("n %d, %d tiles of %d rows, walkers (m = 3 b, 2 b) %s: %d to %d tiles a walker"
          % (n, ntile, rows, [c[0] for c in caps], ntile // GW, -(-ntile // min(c[0] for c in caps))))
    ip, ix, d, _, _ = _kron.kron_sum(KRON_N1, n2, dt)
    S = sa.Lobpcg.new(sa.HipCsr.new((n, n), ip, ix, d), n, block)
    for which in ("smallest", "largest"):
        first = S.solve(k, which, max_iter=1000)
        print("%s: iters %d, fallbacks %d" % (which, first[2]["iters"], first[2]["restarts"]))
        _check_big(KRON_N1, n2, dt, k, which, first[0], first[1], "kron40x%d %s b=%d %s" % (n2, np.dtype(dt).name, block, which))
        assert first[2]["nconv"] == k and first[2]["matvecs"] == block * (first[2]["iters"] + 1)
        assert orth_defect(first[1]) <= 64 * _eps(dt)
        _same_bits(first, S.solve(k, which, max_iter=1000))
    S.close()


@pytest.mark.parametrize("dt,nt", [(F64, -1), (F32, 1), (C64, -1), (C32, -1)], ids=["float64", "float32-nt", "complex128", "complex64"])
def test_fused_walk_takes_several_trips(sa, dt, nt):
    """The fused residual kernel (LobResid through launch_fused) with the "grid" knob at 8 and ew_chunk at 1: one workgroup an
    XCD walks its eighth of the packs in trips of 256, n = 41 * 979 = 40139 (odd, and 3 mod 4: a scalar tail in f64, f32 and c32)
    makes ceil(ceil(n / PK / 8) / 256) >= 5 trips, the last XCD's last trip partial.  Against truth, and against the default-knob
    run of the same case: another summation order of the residual norms, so the values agree to tol |A| and the iteration counts
    within this file's cap between summation orders (LOBPCG has no cycle to count in)."""
    n1, n2 = 41, 979
    n = n1 * n2
    ctx = sa.default_ctx(0)
    pk = 16 // np.dtype(dt).itemsize
    packs = n // pk
    trips = -(-(-(-packs // 8)) // 256)                      # fused_kernel: chunk = trips * 256 packs an XCD, one workgroup each
    assert n % 2 == 1 and n % 4 == 3 and trips >= 5 and 0 < packs - 7 * trips * 256 and (packs - 7 * trips * 256) % 256 != 0
    g0 = ctx.get("grid")
    _, _, _, _, nrm = _kron.kron_sum(n1, n2, dt)
    tol = ref.default_tol(dt)
    for which in ("smallest", "largest"):
        st0, v0, X0_, i0 = _kron_solve(sa, n1, n2, dt, 4, 8, which, max_iter=1000)
        ctx.set("grid", 8); ctx.set("ew_chunk", 1); ctx.set("stream_nt", nt)
        try:
            st1, v1, X1, i1 = _kron_solve(sa, n1, n2, dt, 4, 8, which, max_iter=1000)
        finally:
            ctx.set("grid", g0); ctx.set("ew_chunk", -1); ctx.set("stream_nt", -1)
        assert st0 == ref.OK and st1 == ref.OK
        print("n %d, %d trips a workgroup, %s: iters %d (default knobs %d)" % (n, trips, which, i1["iters"], i0["iters"]))
        _check_big(n1, n2, dt, 4, which, v1, X1, "kron41x979 %s %s grid 8" % (np.dtype(dt).name, which))
        _check_big(n1, n2, dt, 4, which, v0, X0_, "kron41x979 %s %s default" % (np.dtype(dt).name, which))
        assert np.max(np.abs(v1.astype(F64) - v0.astype(F64))) <= tol * nrm
        assert i1["iters"] <= 4 * i0["iters"] and i0["iters"] <= 4 * i1["iters"]
        if i1["iters"] == i0["iters"]:                       # the iterates do not depend on the walk, the residual norms' sums do: n eps each
            assert np.all(np.abs(i1["res"].astype(F64) - i0["res"].astype(F64)) <= 2 * n * _eps(dt) * i0["res"].astype(F64))


# ---------------------------------------------------------------------------------------------- preconditioners
def _precond(sa, A, kind, name, dt):
    if kind == "jacobi":
        ip, ix, d = system(name, dt)
        rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
        return sa.DiagPrecond.new(d[rows == ix].real.astype(np.float32 if is_single(dt) else np.float64).copy(), t_dtype=np.dtype(dt))
    if kind == "fsai":
        return sa.FSAI.new(A, 1)
    if kind == "amg":
        return sa.AMG.new(A)
    return sa.ILU0.new(A, sweeps=3) if kind == "ilu_s3" else sa.ILU0.new(A)


_plain = {}


def _plain_iters(sa, name, dt):
    """The unpreconditioned GPU run of the same case (shared)."""
    key = (name, np.dtype(dt).name)
    if key not in _plain:
        _plain[key] = _solve(sa, name, dt, 4, 8, "smallest")[2]["iters"]
    return _plain[key]


@pytest.mark.parametrize("kind", ["jacobi", "fsai", "amg", "ilu", "ilu_s3"])
@pytest.mark.parametrize("name,dt", [("poisson12x11x10", F64), ("poisson12x11x10", F32), ("symband1500", F64), ("symband1500", F32),
                                     ("hermband700", C64), ("hermband700", C32)], ids=_ids)
def test_preconditioners(sa, name, dt, kind):
    A, n = _handle(sa, name, dt)
    M = _precond(sa, A, kind, name, dt)
    S = sa.Lobpcg.new(A, n, 8)
    vals, X, info = S.solve(4, "smallest", precond=M)
    plain = _plain_iters(sa, name, dt)
    print("%s %s %s: %d iterations, %d without a preconditioner" % (name, np.dtype(dt).name, kind, info["iters"], plain))
    _check_pairs(name, dt, 4, "smallest", vals, X, info)
    assert info["matvecs"] == 8 * (info["iters"] + 1)
    if kind in ("fsai", "amg") and not is_single(dt):
        assert info["iters"] < plain
    Xd = sa.DevVec.from_numpy(S.default_X0().reshape(-1))                # the device entry gives the same bits
    _same_bits((vals, X, info), S.solve(4, "smallest", precond=M, X0=Xd))
    S.close(); M.close()


# ---------------------------------------------------------------------------------------------- multiple eigenvalues
def test_multiple_eigenvalues_are_found_with_multiplicity(sa):
    """poisson3d(8, 8, 8) has triple eigenvalues: the block finds every copy, which a single Lanczos vector cannot."""
    A, lam, nrm = spectrum("poisson8x8x8")
    tol = ref.default_tol(F64)
    for which in ("smallest", "largest"):
        vals, X, info = _solve(sa, "poisson8x8x8", F64, 4, 8, which)
        _check_pairs("poisson8x8x8", F64, 4, which, vals, X, info)
        assert np.max(np.abs(vals - wanted(lam, 4, which))) <= tol * nrm       # with multiplicity: lam_1 = lam_2 = lam_3
        assert orth_defect(X) <= 64 * _eps(F64)


# ---------------------------------------------------------------------------------------------- the same bits
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_two_solves_the_device_entry_and_the_flavours_give_the_same_bits(sa, dt):
    name = "hermband700" if np.dtype(dt).kind == "c" else "symband1500"
    ctx = sa.default_ctx(0)
    A, n = _handle(sa, name, dt)
    S = sa.Lobpcg.new(A, n, 8)
    ctx.set("stream_nt", 0)
    first = S.solve(4, "largest")
    _same_bits(first, S.solve(4, "largest"))
    other = S.solve(3, "smallest")                           # another solve in between leaves nothing behind
    assert other[2]["nconv"] == 3
    _same_bits(first, S.solve(4, "largest"))
    _same_bits(first, S.solve(4, "largest", X0=S.default_X0()))          # the library's default block is default_X0()
    X0 = sa.DevVec.from_numpy(S.default_X0().reshape(-1))
    _same_bits(first, S.solve(4, "largest", X0=X0))
    vals, X, info = S.solve(4, "largest", vectors=False)
    assert X is None
    _same_bits((first[0], None, first[2]), (vals, None, info))
    _same_bits((first[0], None, first[2]), S.solve(4, "largest", X0=X0, vectors=False))
    ctx.set("stream_nt", 1)
    nt = S.solve(4, "largest")
    _same_bits(first, nt)
    _check_pairs(name, dt, 4, "largest", *nt)
    S.close()


def test_every_spmv_route_gives_the_same_bits(sa):
    ctx = sa.default_ctx(0)
    runs, formats = [], []
    for knob in (0, 1, 2):
        ctx.set("spmv_dict", knob)
        A, n = _handle(sa, "poisson12x11x10", F64)
        formats.append(A.stream_format()[0])
        S = sa.Lobpcg.new(A, n, 8)
        runs.append(S.solve(4, "smallest"))
        S.close()
    assert formats == [0, 1, 2], formats
    _same_bits(runs[0], runs[1]); _same_bits(runs[0], runs[2])
    _check_pairs("poisson12x11x10", F64, 4, "smallest", *runs[0])


# ---------------------------------------------------------------------------------------------- events and arguments
def test_one_iteration_is_not_enough(sa):
    A, n = _handle(sa, "symband1500", F64)
    S = sa.Lobpcg.new(A, n, 8)
    with pytest.raises(sa.error.InsufficientIterNum) as ei:
        S.solve(4, "smallest", max_iter=1)
    e = ei.value
    assert e.info["nconv"] < 4 and e.info["iters"] == 1 and e.info["matvecs"] == 16 and e.iters == 1
    assert np.all(np.isfinite(e.vals)) and np.all(np.isfinite(e.X)) and np.all(np.isfinite(e.info["res"])) and e.X.shape == (4, n)
    S.close()


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_breakdowns(sa, dt):
    name = "chgrid9x8" if np.dtype(dt).kind == "c" else "symband30"
    ip, ix, d = system(name, dt)
    n = ip.size - 1
    bad = d.copy(); bad[3] = np.nan
    S = sa.Lobpcg.new(sa.HipCsr.new((n, n), ip, ix, bad), n, 3)
    with pytest.raises(sa.error.BreakDown):
        S.solve(2, "largest")
    S.close()
    A, n = _handle(sa, name, dt)
    S = sa.Lobpcg.new(A, n, 3)
    X0 = S.default_X0(); X0[1] = 0                            # a zero column: G_ii = 0 at the start
    with pytest.raises(sa.error.BreakDown) as ei:
        S.solve(2, "largest", X0=X0)
    assert ei.value.info["matvecs"] <= 3 and ei.value.info["iters"] == 0 and ei.value.X is None
    vals, X, info = S.solve(2, "largest")                     # the handle is as good as new
    _check_pairs(name, dt, 2, "largest", vals, X, info)
    S.close()
    S = sa.Lobpcg.new(A, n, 2)
    X0 = S.default_X0(); X0[1] = X0[0]                        # two equal columns: the Cholesky rule at the start step
    with pytest.raises(sa.error.BreakDown) as ei:
        S.solve(1, "smallest", X0=X0)
    assert ei.value.info["iters"] == 0 and ei.value.info["matvecs"] <= 2
    S.close()


def test_argument_checks(sa):
    from sprsolve_amd import _lib
    Lb = _lib.lib()
    E_ = sa.error
    ctx = sa.default_ctx(0)
    A, n = _handle(sa, "symband30", F64)
    h = C.c_void_p()
    for block in (9, 6):                                     # above 8, 6 block above n = 30
        assert Lb.sprs_lobpcg_create_d(A.h, n, block, C.byref(h)) == _lib.INVALID_ARGUMENT and not h.value
        assert b"block" in Lb.sprs_last_error(ctx.h)
        with pytest.raises(ValueError, match="block"):
            sa.Lobpcg.new(A, n, block)
    assert Lb.sprs_lobpcg_create_d(A.h, n + 1, 2, C.byref(h)) == _lib.DIM_MISMATCH and not h.value
    with pytest.raises(E_.DimensionMismatch):
        sa.Lobpcg.new(A, n + 1, 2)
    assert Lb.sprs_lobpcg_create_s(A.h, n, 2, C.byref(h)) == _lib.INVALID_ARGUMENT and not h.value     # another scalar type
    assert b"scalar type" in Lb.sprs_last_error(ctx.h)
    ip = np.array([0, 1, 2, 3], np.int32); ix = np.array([0, 1, 2], np.int32)
    rect = sa.HipCsr.new((3, 5), ip, ix, np.ones(3))
    assert Lb.sprs_lobpcg_create_d(rect.h, 3, 1, C.byref(h)) == _lib.NOT_SQUARE and not h.value
    with pytest.raises(E_.IncompatibleMatrixFormat):
        sa.Lobpcg.new(rect, 3, 1)
    assert sa.Lobpcg.new(A, n).block == 5 and sa.Lobpcg.new(A, n, 1).block == 1          # block = 0: min(8, n // 6)

    S = sa.Lobpcg.new(A, n, 3)
    for k in (0, 4):                                         # k = 0, k > block
        with pytest.raises(ValueError):
            S.solve(k)
    with pytest.raises(ValueError):
        S.solve(2, which=2)
    with pytest.raises(ValueError):
        S.solve(2, which="both")
    with pytest.raises(ValueError):
        S.solve(2, max_iter=0)
    with pytest.raises(E_.IncompatibleMatrixFormat, match="Input block dimension"):
        S.solve(2, X0=np.ones((3, n + 1)))
    # a preconditioner of another size or scalar type
    with pytest.raises(E_.DimensionMismatch):
        S.solve(2, precond=sa.DiagPrecond.new(np.ones(n + 1)))
    with pytest.raises(ValueError):
        S.solve(2, precond=sa.DiagPrecond.new(np.ones(n, np.float32)))
    A32, _ = _handle(sa, "symband30", F32)
    with pytest.raises(ValueError):
        S.solve(2, precond=sa.FSAI.new(A32, 1))
    B, nb = _handle(sa, "chgrid9x8", C64)
    with pytest.raises((ValueError, E_.DimensionMismatch)):
        S.solve(2, precond=sa.ILU0.new(B))
    vals = (C.c_double * 2)(); res = (C.c_double * 2)()
    X0 = S.default_X0(); X = np.zeros(2 * n + 1)
    args = lambda vl, xl: (S.h, None, 2, 0, X0.ctypes.data_as(C.c_void_p), vl, 500, 1e-10, vals, X.ctypes.data_as(C.c_void_p), xl, res, None, None,
                           None, None)
    assert Lb.sprs_lobpcg_solve_d(*args(3 * n - 1, 2 * n)) == _lib.INCOMPATIBLE_RHS_SIZE
    assert Lb.sprs_lobpcg_solve_d(*args(3 * n, 2 * n + 1)) == _lib.INCOMPATIBLE_X_SIZE
    assert Lb.sprs_lobpcg_solve_d(*args(3 * n, 2 * n)) == _lib.OK             # the four counters may be NULL
    assert Lb.sprs_lobpcg_solve_z(*args(3 * n, 2 * n)) == _lib.INVALID_ARGUMENT       # the handle holds another scalar type
    _check_pairs("symband30", F64, 2, "largest", np.array(vals[:]), X[: 2 * n].reshape(2, n), dict(nconv=2, res=np.array(res[:])))
    S.close()
    assert Lb.sprs_lobpcg_destroy(None) == 0


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
        st = _lib.lib().sprs_lobpcg_create_d(A.h, n, 0, C.byref(h))
        text = _lib.lib().sprs_last_error(ctx.h).decode()
        assert st == _lib.INVALID_ARGUMENT and not h.value and "distributed" in text, (st, text)
        with pytest.raises(ValueError, match="distributed"):
            sa.Lobpcg.new(A, n)
    finally:
        comm.close()
