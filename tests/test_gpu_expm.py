"""The Krylov propagator w = exp(tA) v on the GPU (sprs_expm_*, csrc/expm_fuse.hpp): its result against scipy.linalg.expm of the
dense matrix and against the numpy restatement of the recurrence (tests/_expm_ref.py), the invariants of a unitary evolution,
the happy breakdown, the events, determinism across routes and entry points, the ends of ncv and the argument checks.

The restatement's sub-step, rejection and product counts (tests/test_expm_cpu.py::COUNTS holds and checks them) range from one
sub-step of five products (diag5) to 47 sub-steps of four (cd9x8, ncv 3).  n = 1320 leaves a partial last tile in every scalar
type (a tile is 64 rows of c64, 128 of f64 / c32, 256 of f32), n = 72 is less than one tile; ncv = 48 is the full footprint of
the small exponential in local memory (three 50 x 51 matrices: 122 400 B in the complex types)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _expm_ref as ref  # noqa: E402
import _kron  # noqa: E402
from test_expm_cpu import CASES, COUNTS, TENTH_REJECTION, _id, checker, propagator, system, tol_of, true_error, wide  # noqa: E402

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = [F64, C64, F32, C32]
_KNOBS = ("spmv_dict", "stream_nt")
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
    for k in _KNOBS + ("ew_chunk",):
        ctx.set(k, -1)
    ctx.set("grid", grid)


def _eps(dt):
    return float(np.finfo(ref.real_dtype(dt)).eps)


def _handle(sa, name, dt):
    ip, ix, d = system(name, dt)
    n = ip.size - 1
    return sa.HipCsr.new((n, n), ip, ix, d), n


def _apply(sa, name, dt, t, ncv, v=None, **kw):
    A, n = _handle(sa, name, dt)
    E = sa.Expm.new(A, n, ncv)
    try:
        return E.apply(t, ref.start_vector(n, dt) if v is None else v, **kw)
    finally:
        E.close()


def _norm(x):
    return float(np.linalg.norm(np.asarray(x).astype(wide(x.dtype))))


def _same_bits(a, b):
    (wa, ia), (wb, ib) = a, b
    wa = wa.to_numpy() if hasattr(wa, "to_numpy") else wa
    wb = wb.to_numpy() if hasattr(wb, "to_numpy") else wb
    assert np.array_equal(wa.view(np.uint8), wb.view(np.uint8))
    assert ia == ib


# ---------------------------------------------------------------------------------------------- parity with the mathematics
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_parity(sa, case):
    name, dtname, t, ncv, tau0, tol = case
    dt = np.dtype(dtname).type
    o, p = checker(case), checker(case, "pairwise")
    w, info = _apply(sa, name, dt, t, ncv, tol=tol, tau0=tau0)
    bound = 1.2 * abs(t) * tol_of(case)
    err, ref_err, pw_err = true_error(name, dt, t, w), true_error(name, dt, t, o.w), true_error(name, dt, t, p.w)
    print("%s: true error %.3e (the restatement's %.3e, with pairwise sums %.3e), estimate %.3e, bound %.3e, %r"
          % (_id(case), err, ref_err, pw_err, info["err"], bound, info))
    assert np.all(np.isfinite(w))
    assert err <= bound
    assert err <= max(4 * ref_err, pw_err)
    steps, rejects, matvecs = COUNTS[case]
    assert abs(info["steps"] - steps) <= 1 and abs(info["rejects"] - rejects) <= 1, (info, COUNTS[case])
    if name == "diag5":
        assert (info["steps"], info["matvecs"]) == (1, 5)
    else:
        assert info["matvecs"] == info["steps"] * (ncv + 1)
    assert 0.0 <= info["err"] <= bound
    assert info["hump"] >= _norm(ref.start_vector(w.size, dt)) * (1 - w.size * _eps(dt))     # (any order of a sum of n squares)
    assert info["t_done"] == float(np.dtype(ref.real_dtype(dt)).type(t))


# ---------------------------------------------------------------------------------------------- several trips a workgroup
@pytest.mark.parametrize("dt,nt", [(F64, -1), (F32, -1), (C64, -1), (C32, 1)], ids=["float64", "float32", "complex128", "complex64-nt"])
def test_fused_walk_takes_several_trips(sa, dt, nt):
    """The fused kernels of the Arnoldi step and of the state update with the "grid" knob at 8 and ew_chunk at 1: one workgroup an
    XCD walks its eighth of the packs in trips of 256.  kron_sum(41, 979) (tests/_kron.py), n = 40139: odd and 3 mod 4 (a scalar
    tail in f64, f32 and c32), at least five trips, the last XCD's last trip partial.  ncv = 30, t = 0.25 (|exp(tA)|_2 = e^(4 t)
    = 2.7), a start vector of norm one.  Truth is vec(E2 V E1^T) from the dense exponentials of the two factors: |w - w_exact|
    against the bound test_parity applies to the error estimate, for this run and the default-knob run of the same case, which
    agree to twice that bound and in their counts within one sub-step."""
    n1, n2, ncv, t = 41, 979, 30, 0.25
    n = n1 * n2
    ctx = sa.default_ctx(0)
    packs = n // (16 // np.dtype(dt).itemsize)
    trips = -(-(-(-packs // 8)) // 256)                      # fused_kernel: chunk = trips * 256 packs an XCD, one workgroup each
    assert n % 2 == 1 and n % 4 == 3 and trips >= 5 and 0 < packs - 7 * trips * 256 and (packs - 7 * trips * 256) % 256 != 0
    ip, ix, d, _, nrm = _kron.kron_sum(n1, n2, dt)
    v = ref.start_vector(n, dt).astype(wide(dt))
    v = (v / np.linalg.norm(v)).astype(dt)
    exact = _kron.expm_exact(n1, n2, t, v, np.dtype(dt).kind == "c")
    bound = 1.2 * abs(t) * ref.default_tol(dt)
    A = sa.HipCsr.new((n, n), ip, ix, d)
    E = sa.Expm.new(A, n, ncv)
    g0 = ctx.get("grid")
    w0, i0 = E.apply(t, v)
    ctx.set("grid", 8); ctx.set("ew_chunk", 1); ctx.set("stream_nt", nt)
    try:
        w1, i1 = E.apply(t, v)
    finally:
        ctx.set("grid", g0); ctx.set("ew_chunk", -1); ctx.set("stream_nt", -1)
    E.close()
    e0, e1 = _norm(w0.astype(wide(dt)) - exact), _norm(w1.astype(wide(dt)) - exact)
    print("n %d, %d trips a workgroup, |exp(tA)| %.2f: |w - w_exact| %.3e (default knobs %.3e), estimates %.3e and %.3e, bound %.3e, %r / %r"
          % (n, trips, np.exp(t * nrm), e1, e0, i1["err"], i0["err"], bound, i1, i0))
    assert np.all(np.isfinite(w1)) and e1 <= bound and e0 <= bound
    assert 0.0 <= i1["err"] <= bound and i1["t_done"] == float(np.dtype(ref.real_dtype(dt)).type(t))
    assert _norm(w1.astype(wide(dt)) - w0.astype(wide(dt))) <= 2 * bound
    assert abs(i1["steps"] - i0["steps"]) <= 1 and abs(i1["rejects"] - i0["rejects"]) <= 1
    assert i1["matvecs"] == i1["steps"] * (ncv + 1)


# ---------------------------------------------------------------------------------------------- a unitary evolution
@pytest.mark.parametrize("dt", [C64, C32], ids=_dtid)
def test_schroedinger_keeps_the_norm_and_runs_backwards(sa, dt):
    A, n = _handle(sa, "schro700", dt)
    E = sa.Expm.new(A, n, 12)
    v = ref.start_vector(n, dt)
    t = 0.5
    bound = 1.2 * t * ref.default_tol(dt)
    w, info = E.apply(t, v)
    assert abs(_norm(w) - _norm(v)) <= bound
    back, info2 = E.apply(-t, w)
    d = _norm(back.astype(wide(dt)) - v.astype(wide(dt)))
    print("schro700 %s: | |w| - |v| | %.3e, |exp(-tA) exp(tA) v - v| %.3e, bound %.3e" % (np.dtype(dt).name, abs(_norm(w) - _norm(v)), d, bound))
    assert d <= 2 * bound
    assert info2["t_done"] == -t and info2["steps"] >= 1
    E.close()


# ---------------------------------------------------------------------------------------------- events
@pytest.mark.parametrize("dt", ALL, ids=_dtid)
def test_happy_breakdown(sa, dt):
    w, info = _apply(sa, "diag5", dt, 1.5, 12)
    assert (info["steps"], info["rejects"], info["matvecs"], info["err"]) == (1, 0, 5, 0.0)
    ip, ix, d = system("diag5", F64)
    exact = np.exp(1.5 * d) * ref.start_vector(300, dt).astype(wide(dt))
    assert np.linalg.norm(w.astype(wide(dt)) - exact) <= 64 * _eps(dt) * np.linalg.norm(exact)


@pytest.mark.parametrize("dt", ALL, ids=_dtid)
def test_zero_time_zero_vector_and_nan(sa, dt):
    name = "schro700" if np.dtype(dt).kind == "c" else "cd40x33"
    A, n = _handle(sa, name, dt)
    E = sa.Expm.new(A, n, 10)
    v = ref.start_vector(n, dt)
    zero = dict(err=0.0, hump=0.0, t_done=0.0, steps=0, rejects=0, matvecs=0)
    w, info = E.apply(0.0, v)                                # t = 0: v bit for bit, no product
    assert np.array_equal(w.view(np.uint8), v.view(np.uint8)) and info == zero
    vd = sa.DevVec.from_numpy(v)
    wd, info = E.apply(0.0, vd)
    assert np.array_equal(wd.to_numpy().view(np.uint8), v.view(np.uint8)) and info == zero
    w, info = E.apply(-0.5, np.zeros(n, dt), out=np.ones(n, dt))      # v = 0: zeros, SPRS_OK
    assert not np.any(w) and info["matvecs"] == 0 and info["steps"] == 0
    bad = v.copy(); bad[n // 2] = np.nan
    for dev in (False, True):                                # a NaN in v: SPRS_BREAKDOWN, w is not written
        out = np.full(n, 7, dt)
        outd = sa.DevVec.from_numpy(out) if dev else out
        with pytest.raises(sa.error.BreakDown) as ei:
            E.apply(0.5, sa.DevVec.from_numpy(bad) if dev else bad, out=outd)
        assert ei.value.w is None and ei.value.info["matvecs"] == 0 and ei.value.info["steps"] == 0
        assert np.array_equal(outd.to_numpy() if dev else outd, np.full(n, 7, dt))
    w, info = E.apply(0.25, v)                               # the handle is as good as new
    assert true_error(name, dt, 0.25, w) <= 1.2 * 0.25 * ref.default_tol(dt)
    E.close()


def test_one_sub_step_is_not_enough(sa):
    case = ("heat12x11x10", "float64", 0.5, 10, 0.0, 0.0)
    assert COUNTS[case][0] > 1
    A, n = _handle(sa, "heat12x11x10", F64)
    E = sa.Expm.new(A, n, 10)
    v = ref.start_vector(n, F64)
    with pytest.raises(sa.error.InsufficientIterNum) as ei:
        E.apply(0.5, v, max_steps=1)
    e = ei.value
    assert e.info["steps"] == 1 and e.info["matvecs"] == 11 and e.iters == 1 and 0.0 < abs(e.info["t_done"]) < 0.5
    # w is the state at t_done
    assert np.linalg.norm(e.w - propagator("heat12x11x10", e.info["t_done"]) @ v) <= 1.2 * 0.5 * ref.default_tol(F64)
    with pytest.raises(sa.error.InsufficientIterNum) as ei:
        E.apply(-0.5, v, max_steps=1)
    assert -0.5 < ei.value.info["t_done"] < 0.0
    E.close()


def test_the_tenth_rejection_is_a_breakdown(sa):
    name, dtname, t, ncv, tau0, tol = TENTH_REJECTION
    o = checker(TENTH_REJECTION)
    assert o.status == ref.BREAKDOWN
    with pytest.raises(sa.error.BreakDown) as ei:
        _apply(sa, name, np.dtype(dtname).type, t, ncv, tau0=tau0)
    assert ei.value.info["rejects"] == ref.MAX_REJECTS - 1 and ei.value.info["steps"] == 0 and ei.value.info["matvecs"] == ncv + 1


# ---------------------------------------------------------------------------------------------- routes, determinism
@pytest.mark.parametrize("dt", ALL, ids=_dtid)
def test_same_bits_twice_aliased_and_through_the_device_entry(sa, dt):
    name = "schro700" if np.dtype(dt).kind == "c" else "cd40x33"
    A, n = _handle(sa, name, dt)
    E = sa.Expm.new(A, n, 10)
    v = ref.start_vector(n, dt)
    first = E.apply(1.0, v, tau0=1.0)
    assert first[1]["rejects"] >= 1
    _same_bits(first, E.apply(1.0, v, tau0=1.0))
    other = E.apply(-0.1, v)                                 # another application in between leaves nothing behind
    assert other[1]["steps"] >= 1
    _same_bits(first, E.apply(1.0, v, tau0=1.0))
    alias = v.copy()
    _same_bits(first, E.apply(1.0, alias, tau0=1.0, out=alias))          # w may be v
    vd = sa.DevVec.from_numpy(v)
    _same_bits(first, E.apply(1.0, vd, tau0=1.0))
    _same_bits(first, E.apply(1.0, vd, tau0=1.0, out=vd))
    E.close()


@pytest.mark.parametrize("knob", _KNOBS)
def test_knobs_give_the_same_bits(sa, knob):
    ctx = sa.default_ctx(0)
    runs = []
    for value in (0, 1):
        ctx.set(knob, value)
        runs.append(_apply(sa, "heat12x11x10", F64, 1.0, 12, tau0=1.0))
    _same_bits(runs[0], runs[1])
    assert true_error("heat12x11x10", F64, 1.0, runs[0][0]) <= 1.2 * ref.default_tol(F64)


def test_one_call(sa):
    A, n = _handle(sa, "cd9x8", F64)
    v = ref.start_vector(n, F64)
    w, info = sa.expm_multiply(A, v, t=0.5, ncv=10)
    _same_bits((w, info), _apply(sa, "cd9x8", F64, 0.5, 10))
    w, info = sa.expm_multiply(A, v)                          # t = 1, ncv = min(30, n)
    assert np.linalg.norm(w - propagator("cd9x8", 1.0) @ v) <= 1.2 * ref.default_tol(F64)


# ---------------------------------------------------------------------------------------------- arguments
def test_argument_checks(sa):
    from sprsolve_amd import _lib
    Lb = _lib.lib()
    E_ = sa.error
    A, n = _handle(sa, "cd9x8", F64)
    h = C.c_void_p()
    for ncv in (1, 2, 49, 73):                               # below 3, above 48, above n = 72
        assert Lb.sprs_expm_create_d(A.h, n, ncv, C.byref(h)) == _lib.INVALID_ARGUMENT and not h.value
        with pytest.raises(ValueError, match="ncv"):
            sa.Expm.new(A, n, ncv)
    assert Lb.sprs_expm_create_d(A.h, n + 1, 8, C.byref(h)) == _lib.DIM_MISMATCH and not h.value
    with pytest.raises(E_.DimensionMismatch):
        sa.Expm.new(A, n + 1, 8)
    assert Lb.sprs_expm_create_s(A.h, n, 8, C.byref(h)) == _lib.INVALID_ARGUMENT and not h.value       # another scalar type
    ip = np.array([0, 1, 2, 3], np.int32); ix = np.array([0, 1, 2], np.int32)
    rect = sa.HipCsr.new((3, 5), ip, ix, np.ones(3))
    assert Lb.sprs_expm_create_d(rect.h, 3, 3, C.byref(h)) == _lib.NOT_SQUARE and not h.value
    with pytest.raises(E_.IncompatibleMatrixFormat):
        sa.Expm.new(rect, 3, 3)
    assert sa.Expm.new(A, n).ncv == 30 and sa.Expm.new(A, n, 3).ncv == 3 and sa.Expm.new(A, n, 48).ncv == 48      # ncv = 0: min(30, n)

    E = sa.Expm.new(A, n, 8)
    v = ref.start_vector(n, F64)
    for t in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError):
            E.apply(t, v)
    for kw in (dict(tol=-1.0), dict(tol=np.nan), dict(tau0=-1.0), dict(tau0=np.inf), dict(max_steps=0)):
        with pytest.raises(ValueError):
            E.apply(0.5, v, **kw)
    with pytest.raises(E_.IncompatibleMatrixFormat, match="Input vec dimension"):
        E.apply(0.5, np.ones(n + 1))
    with pytest.raises(E_.IncompatibleMatrixFormat, match="output vec dimension"):
        E.apply(0.5, v, out=np.ones(n + 1))
    w = np.zeros(n)
    args = lambda vl, wl: (E.h, 0.5, v.ctypes.data_as(C.c_void_p), vl, 0.0, 100, 0.0, w.ctypes.data_as(C.c_void_p), wl, None, None, None, None, None, None)
    assert Lb.sprs_expm_apply_d(*args(n - 1, n)) == _lib.INCOMPATIBLE_RHS_SIZE
    assert Lb.sprs_expm_apply_d(*args(n, n - 1)) == _lib.INCOMPATIBLE_X_SIZE
    assert Lb.sprs_expm_apply_d(*args(n, n)) == _lib.OK                  # the six outputs may be NULL
    assert Lb.sprs_expm_apply_z(*args(n, n)) == _lib.INVALID_ARGUMENT    # the handle holds another scalar type
    assert np.linalg.norm(w - propagator("cd9x8", 0.5) @ v) <= 1.2 * 0.5 * ref.default_tol(F64)
    E.close()
    assert Lb.sprs_expm_destroy(None) == 0


def test_distributed_operator_is_refused(sa):
    import torch
    from sprsolve_amd import _lib, dist as sdist
    from test_gpu_dist import _self_halo_plan
    ctx = sa.default_ctx(0)
    dev = torch.device("cuda", 0)
    comm = sdist.Comm(ctx, 0, 1)
    try:
        ip, ix, d = system("cd40x33", F64)
        n = ip.size - 1
        plan = _self_halo_plan(torch, dev, n, ix, lambda c: np.zeros(c.shape, bool))
        A = sdist.DistCsr.from_plan(comm, plan, int(ip[-1]), torch.from_numpy(ip.copy()).to(dev), torch.from_numpy(d.copy()).to(dev), adopt=True,
                                    to_device=lambda a: torch.from_numpy(a).to(dev))
        h = C.c_void_p()
        st = _lib.lib().sprs_expm_create_d(A.h, n, 0, C.byref(h))
        text = _lib.lib().sprs_last_error(ctx.h).decode()
        assert st == _lib.INVALID_ARGUMENT and not h.value and "distributed" in text, (st, text)
        with pytest.raises(ValueError, match="distributed"):
            sa.Expm.new(A, n)
    finally:
        comm.close()
