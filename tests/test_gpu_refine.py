"""Mixed-precision iterative refinement on the GPU (sprs_refine_*, csrc/refine.hip, refine_fuse.hpp) against the numpy restatement
of its recurrence (tests/_refine_ref.py): the element-wise kernels bit for bit, the demoted operator bit for bit, the solves
against the checker, what the feature is for, the events of the recurrence, and one larger shape.

The checker's counts (x0 = 0, tol 1e-12; measured on the CPU, tests/test_refine_cpu.py asserts them): 3 outer steps at
inner_tol 1e-4 (inner CG 11/12/11 on symmetric_banded(2000), 11/11/11 on hermitian_banded(1500, 3)), 6 at inner_tol 1e-2."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _refine_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
TOL, MAX_OUTER, INNER_MAX = 1e-12, 20, 200
_KNOBS = ("spmv_dict", "spmv_tile", "spmv_chain", "spmv_wide", "halo_overlap")      # tests/test_gpu_cg.py::_KNOBS


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
    poll = ctx.get("poll")
    halo = ctx.get("halo_overlap")
    yield
    for k in _KNOBS[:4]:
        ctx.set(k, -1)
    ctx.set("halo_overlap", halo); ctx.set("poll", poll)


_SYS = {}


def _system(dt):
    """The banded generators (their diagonal varies, so Jacobi is not a constant scaling), computed once."""
    key = np.dtype(dt).kind
    if key not in _SYS:
        from sprsolve_amd import gen
        _SYS[key] = gen.hermitian_banded(1500, 3) if key == "c" else gen.symmetric_banded(2000)
    return _SYS[key]


_CHECKER = {}


def _checker(dt, **kw):
    """tests/_refine_ref.py on _system(dt) from x0 = 0, computed once per setting and never modified."""
    key = (np.dtype(dt).kind,) + tuple(sorted(kw.items()))
    if key not in _CHECKER:
        ip, ix, d, rhs = _system(dt)
        args = dict(max_outer=MAX_OUTER, tol=TOL, inner_max_iter=INNER_MAX, inner_tol=1e-4, inner="cg", restart=10, jacobi=False,
                    keep_iterates=False)
        args.update(kw)
        dg = _diag(ip, ix, d) if args.pop("jacobi") else None
        _CHECKER[key] = ref.refine(ip, ix, d, rhs, np.zeros(rhs.size, d.dtype), precond_diag=dg, **args)
    return _CHECKER[key]


def _diag(ip, ix, d):
    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    return d[rows == ix].real.copy()


def _csr(ip, ix, d):
    import scipy.sparse as sp
    n = ip.size - 1
    return sp.csr_matrix((d, ix, ip), shape=(n, n))


def _true_res(ip, ix, d, rhs, x):
    return np.linalg.norm(rhs - _csr(ip, ix, d) @ x) / np.linalg.norm(rhs)


_EXACT = {}


def _exact(dt):
    key = np.dtype(dt).kind
    if key not in _EXACT:
        import scipy.sparse.linalg as spla
        ip, ix, d, rhs = _system(dt)
        _EXACT[key] = spla.spsolve(_csr(ip, ix, d).tocsc(), rhs)
    return _EXACT[key]


def _run(sa, R, rhs, x, max_outer=MAX_OUTER, tol=TOL, inner_max_iter=INNER_MAX, inner_tol=1e-4):
    """-> (status, outer, inner_its, res) with the checker's status codes; x is updated in place."""
    E = sa.error
    try:
        return (ref.OK,) + tuple(R.solve(rhs, x, max_outer, tol, inner_max_iter, inner_tol))
    except E.InsufficientIterNum:
        st = ref.INSUFFICIENT_ITER
    except E.BreakDown:
        st = ref.BREAKDOWN
    except E.InvalidPreconditioner:
        st = ref.INVALID_PRECOND
    return (st,) + R.last


# ------------------------------------------------------------------------------------------------ 1. element-wise kernels
LENGTHS = [1, 3, 4, 5, 255, 1027]


def _same_bits(got, want):
    """Bit for bit, a NaN answering a NaN (its payload is the converter's business); complex: per component."""
    R = {np.dtype(F32): F32, np.dtype(C32): F32, np.dtype(F64): F64, np.dtype(C64): F64}[got.dtype]
    U = np.uint32 if R is F32 else np.uint64
    g, w = np.ascontiguousarray(got).view(R), np.ascontiguousarray(want).view(R)
    nan = np.isnan(w)
    return g.shape == w.shape and np.array_equal(np.isnan(g), nan) and np.array_equal(g[~nan].view(U), w[~nan].view(U))


def _specials(v, vals):
    """Put the special values in front, as many as fit (complex: into the components, re and im alternately).  Writes into v."""
    R = v.view(F32 if v.dtype in (np.dtype(F32), np.dtype(C32)) else F64)
    k = min(R.size, len(vals))
    R[:k] = vals[:k]
    return v


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset-by-one"])
@pytest.mark.parametrize("dt", [F64, C64], ids=lambda d: np.dtype(d).name)
def test_demote_scaled_bit_for_bit(sa, dt, offset):
    """out_i = fl_L(in_i * scale), against numpy's (v * scale).astype(L) with the real scale applied per component."""
    import torch
    from sprsolve_amd import vecalg
    L = ref.LOW[np.dtype(dt)]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    scale = 0.37
    for n in LENGTHS:
        m = n + offset
        v = rng.standard_normal(m) * 10.0 ** rng.integers(-30, 30, m)          # |v * scale| stays in L's normal range
        if np.dtype(dt).kind == "c":
            v = v + 1j * (rng.standard_normal(m) * 10.0 ** rng.integers(-30, 30, m))
        v = v.astype(dt)
        # +-0, a product beyond L's largest finite value on either side (3.7e38 > 3.4e38), NaN
        _specials(v[offset:], [0.0, -0.0, 1e39, -1e39, np.nan, 1e300, -0.0, 0.0])
        t_in = torch.from_numpy(v).to(dev)
        t_out = torch.full((m,), 7.0, dtype=torch.from_numpy(np.zeros(1, L)).dtype, device=dev)
        vecalg.demote_scaled(t_in[offset:], scale, t_out[offset:])
        got = t_out.cpu().numpy()
        want = ref.demote_scaled(v[offset:], scale, L)
        assert _same_bits(got[offset:], want), (np.dtype(dt).name, n, offset)
        assert np.all(got[:offset] == 7.0)                                      # nothing in front of the view was written
        if n >= 5 and np.dtype(dt).kind != "c":
            assert np.isposinf(got[offset + 2]) and np.isneginf(got[offset + 3]) and np.isnan(got[offset + 4])
            assert not np.signbit(got[offset]) and np.signbit(got[offset + 1]) and got[offset] == 0 == got[offset + 1]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset-by-one"])
@pytest.mark.parametrize("dt", [F64, C64], ids=lambda d: np.dtype(d).name)
def test_axpy_promoted_bit_for_bit(sa, dt, offset):
    """x_i = x_i + fl_H(in_i) * alpha, against numpy's x + e.astype(H) * alpha with the real alpha applied per component."""
    import torch
    from sprsolve_amd import vecalg
    L = ref.LOW[np.dtype(dt)]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    alpha = 3.1e-5
    for n in LENGTHS:
        m = n + offset
        e = rng.standard_normal(m) * 10.0 ** rng.integers(-20, 20, m)
        x = rng.standard_normal(m)
        if np.dtype(dt).kind == "c":
            e = e + 1j * (rng.standard_normal(m) * 10.0 ** rng.integers(-20, 20, m))
            x = x + 1j * rng.standard_normal(m)
        e = e.astype(L); x = x.astype(dt)
        _specials(e[offset:], [0.0, -0.0, np.inf, -np.inf, np.nan, 3e38, -0.0, 0.0])
        t_e = torch.from_numpy(e).to(dev); t_x = torch.from_numpy(x).to(dev)
        vecalg.axpy_promoted(alpha, t_e[offset:], t_x[offset:])
        got = t_x.cpu().numpy()
        want = ref.axpy_promoted(x[offset:], e[offset:], alpha)
        assert _same_bits(got[offset:], want), (np.dtype(dt).name, n, offset)
        assert np.array_equal(got[:offset], x[:offset])


def test_elementwise_host_arrays_and_type_checks(sa):
    from sprsolve_amd import vecalg
    v = np.linspace(-2.0, 2.0, 1027)
    out = np.zeros(1027, F32)
    vecalg.demote_scaled(v, 1.0 / 3.0, out)
    assert _same_bits(out, ref.demote_scaled(v, 1.0 / 3.0, F32))
    x = np.ones(1027)
    vecalg.axpy_promoted(0.1, out, x)
    assert _same_bits(x, ref.axpy_promoted(np.ones(1027), out, 0.1))
    with pytest.raises(TypeError):
        vecalg.demote_scaled(v, 1.0, np.zeros(1027))                            # f64 -> f64 is no demotion
    with pytest.raises(TypeError):
        vecalg.axpy_promoted(1.0, np.zeros(4, C32), np.zeros(4))


# ------------------------------------------------------------------------------------------------ 2. the demoted operator
@pytest.mark.parametrize("dt", [F64, C64], ids=lambda d: np.dtype(d).name)
def test_low_operator_is_the_rounded_matrix(sa, dt):
    ip, ix, d, rhs = _system(dt)
    n = rhs.size
    L = ref.LOW[np.dtype(dt)]
    A = sa.HipCsr.new((n, n), ip, ix, d)
    dg = _diag(ip, ix, d)
    for P in (None, sa.DiagPrecond.new(dg, t_dtype=dt)):
        R = sa.Refine.new(A, n, precond=P)
        direct = sa.HipCsr.new((n, n), ip, ix, d.astype(L))
        assert R.low.dtype == np.dtype(L) and R.low.shape == (n, n) and R.low.nnz() == d.size
        assert R.low.stream_format() == direct.stream_format()
        v = rhs.astype(L)
        y0 = np.zeros(n, L); y1 = np.zeros(n, L)
        R.low.mul_vec(v, y0); direct.mul_vec(v, y1)
        assert _same_bits(y0, y1) and np.any(y0)
        R.close()
        y2 = np.zeros(n, dt)
        A.mul_vec(rhs, y2)                                                      # the f64 handle lives on, untouched
        assert np.allclose(y2, _csr(ip, ix, d) @ rhs, rtol=1e-12)


def test_creation_refusals(sa):
    from sprsolve_amd import _lib
    Lb = _lib.lib()
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = _system(F64)
    n = rhs.size
    big = d.copy(); big[3] = 1e300
    A = sa.HipCsr.new((n, n), ip, ix, big)
    h = C.c_void_p()
    st = Lb.sprs_refine_create_d(A.h, n, None, _lib.INNER_CG, 0, C.byref(h))
    assert st == _lib.INVALID_ARGUMENT and not h.value
    text = Lb.sprs_last_error(ctx.h).decode()
    assert "single precision" in text, text
    with pytest.raises(ValueError, match="single precision"):
        sa.Refine.new(A, n)
    inf = d.copy(); inf[3] = np.inf                                             # an infinity was one before the demotion
    sa.Refine.new(sa.HipCsr.new((n, n), ip, ix, inf), n).close()
    good = sa.HipCsr.new((n, n), ip, ix, d)
    with pytest.raises(ValueError):
        sa.Refine.new(good, n, inner="gmres", restart=65)
    with pytest.raises(sa.error.DimensionMismatch):
        sa.Refine.new(good, n - 1)
    with pytest.raises(sa.error.DimensionMismatch):
        sa.Refine.new(good, n, precond=sa.DiagPrecond.new(np.ones(n - 1)))
    with pytest.raises(ValueError):
        sa.Refine.new(good, n, precond=sa.DiagPrecond.new(np.ones(n), t_dtype=C64))
    with pytest.raises(TypeError):
        sa.Refine.new(sa.HipCsr.new((n, n), ip, ix, d.astype(F32)), n)
    assert Lb.sprs_refine_create_d(None, n, None, 0, 0, C.byref(h)) == _lib.INVALID_ARGUMENT
    assert Lb.sprs_refine_create_z(good.h, n, None, 0, 0, C.byref(h)) == _lib.INVALID_ARGUMENT      # an f64 handle
    assert Lb.sprs_refine_create_d(good.h, n, None, 2, 0, C.byref(h)) == _lib.INVALID_ARGUMENT      # no such inner solver
    assert Lb.sprs_refine_destroy(None) == 0 and not Lb.sprs_refine_low_csr(None)


def test_distributed_operator_is_refused(sa):
    import torch
    from sprsolve_amd import _lib, dist as sdist
    from test_gpu_dist import _self_halo_plan
    ctx = sa.default_ctx(0)
    dev = torch.device("cuda", 0)
    comm = sdist.Comm(ctx, 0, 1)
    try:
        ip, ix, d, rhs = _system(F64)
        n = rhs.size
        plan = _self_halo_plan(torch, dev, n, ix, lambda c: np.zeros(c.shape, bool))
        A = sdist.DistCsr.from_plan(comm, plan, int(ip[-1]), torch.from_numpy(ip).to(dev), torch.from_numpy(d).to(dev), adopt=True,
                                    to_device=lambda a: torch.from_numpy(a).to(dev))
        h = C.c_void_p()
        st = _lib.lib().sprs_refine_create_d(A.h, n, None, _lib.INNER_CG, 0, C.byref(h))
        text = _lib.lib().sprs_last_error(ctx.h).decode()
        assert st == _lib.INVALID_ARGUMENT and not h.value and "distributed" in text, (st, text)
        with pytest.raises(ValueError, match="distributed"):
            sa.Refine.new(A, n)
    finally:
        comm.close()


# ------------------------------------------------------------------------------------------------ 3. solves against the checker
@pytest.mark.parametrize("inner_tol", [1e-4, 1e-2])
@pytest.mark.parametrize("pc", ["none", "jacobi"])
@pytest.mark.parametrize("inner", ["cg", "gmres"])
@pytest.mark.parametrize("dt", [F64, C64], ids=lambda d: np.dtype(d).name)
def test_solves_follow_the_checker(sa, dt, inner, pc, inner_tol):
    ip, ix, d, rhs = _system(dt)
    n = rhs.size
    o = _checker(dt, inner=inner, jacobi=pc == "jacobi", inner_tol=inner_tol)
    assert o.status == ref.OK and 2 * o.outer <= MAX_OUTER
    A = sa.HipCsr.new((n, n), ip, ix, d)
    P = sa.DiagPrecond.new(_diag(ip, ix, d), t_dtype=dt) if pc == "jacobi" else None
    R = sa.Refine.new(A, n, inner=inner, restart=10, precond=P)
    x = np.zeros(n, dt)
    st, outer, inner_its, res = _run(sa, R, rhs, x, inner_tol=inner_tol)
    true = _true_res(ip, ix, d, rhs, x)
    a1 = np.max(np.abs(_csr(ip, ix, d)).sum(axis=0))
    bound = 64 * np.finfo(F64).eps * (a1 * np.linalg.norm(x) + np.linalg.norm(rhs)) / np.linalg.norm(rhs)
    xs = _exact(dt)
    err = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
    print("refine %s %s %s %g: outer %d (checker %d) inner %d (checker %d = %s) res %.3e true %.3e |res - true| %.1e (bound %.1e) err %.1e"
          % (np.dtype(dt).name, inner, pc, inner_tol, outer, o.outer, inner_its, sum(o.inner), o.inner, res, true, abs(res - true), bound, err))
    assert st == ref.OK
    assert abs(outer - o.outer) <= 1
    assert abs(inner_its - sum(o.inner)) <= 2 * max(outer, o.outer)
    assert true <= TOL
    assert abs(res - true) <= bound
    assert err <= 1e-9


# ------------------------------------------------------------------------------------------------ 4. what it is for
def test_f32_stalls_where_refinement_arrives(sa):
    ip, ix, d, rhs = _system(F64)
    n = rhs.size
    A32 = sa.HipCsr.new((n, n), ip, ix, d.astype(F32))
    x32 = np.zeros(n, F32)
    try:
        its32, res32 = sa.CG.new(A32, n).solve(rhs.astype(F32), x32, 200, 1e-12)
    except sa.error.InsufficientIterNum as e:                                   # its recurrence residual need not reach 1e-12
        its32, res32 = e.iters, float("nan")
    true32 = _true_res(ip, ix, d, rhs, x32.astype(F64))
    A = sa.HipCsr.new((n, n), ip, ix, d)
    R = sa.Refine.new(A, n)
    x = np.zeros(n)
    outer, inner_its, res = R.solve(rhs, x, MAX_OUTER, TOL, INNER_MAX, 1e-4)
    true = _true_res(ip, ix, d, rhs, x)
    print("f32 CG: its %d reported %.2e true %.2e; refine: outer %d inner %d res %.2e true %.2e" % (its32, res32, true32, outer, inner_its, res, true))
    assert true32 > 1e-8
    assert true <= 1e-12
    assert inner_its < 3 * 26                # f64 CG needs 26 iterations for 1e-10 on this system (tests/test_gpu_cg.py)


# ------------------------------------------------------------------------------------------------ 5. events
def test_events_land_where_the_recurrence_says(sa):
    ip, ix, d, rhs = _system(F64)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    R = sa.Refine.new(A, n)
    x = np.full(n, 3.0)
    assert _run(sa, R, np.zeros(n), x) == (ref.OK, 0, 0, 0.0) and not np.any(x)
    exact = _exact(F64)
    x = exact.copy()
    st, outer, inner_its, res = _run(sa, R, rhs, x)
    assert (st, outer, inner_its) == (ref.OK, 0, 0) and 0 <= res <= TOL and np.array_equal(x, exact)
    # max_outer = 1: one correction is made, then the second residual test gives up
    o = _checker(F64, max_outer=1, inner_tol=1e-2, keep_iterates=True)
    assert (o.status, o.outer) == (ref.INSUFFICIENT_ITER, 1)
    x = np.zeros(n)
    with pytest.raises(sa.error.InsufficientIterNum) as ei:
        R.solve(rhs, x, 1, TOL, INNER_MAX, 1e-2)
    assert ei.value.iters == 1 and abs(R.last[1] - o.inner[0]) <= 2
    assert np.max(np.abs(x - o.xs[0])) <= 1e-5 * np.max(np.abs(o.xs[0]))
    assert TOL < R.last[2] < 0.1                                                # the residual the second test found
    # an inner solve that runs out of iterations still corrects
    o = _checker(F64, max_outer=100, inner_max_iter=2)
    assert o.status == ref.OK and o.outer == 24
    x = np.zeros(n)
    st, outer, inner_its, res = _run(sa, R, rhs, x, max_outer=2 * o.outer, inner_max_iter=2)
    print("inner_max_iter 2: outer %d (checker %d) inner %d" % (outer, o.outer, inner_its))
    assert st == ref.OK and inner_its == 2 * outer and _true_res(ip, ix, d, rhs, x) <= TOL
    # an indefinite matrix: the inner CG breaks down, x is what it was
    neg = d.copy()
    rows = np.repeat(np.arange(n), np.diff(ip))
    neg[np.flatnonzero(rows == ix)[n // 2]] *= -1.0
    x0 = np.linspace(-1.0, 1.0, n)
    assert ref.refine(ip, ix, neg, rhs, x0, MAX_OUTER, TOL, INNER_MAX, 1e-4).status == ref.BREAKDOWN
    Rn = sa.Refine.new(sa.HipCsr.new((n, n), ip, ix, neg), n)
    x = x0.copy()
    with pytest.raises(sa.error.BreakDown):
        Rn.solve(rhs, x, MAX_OUTER, TOL, INNER_MAX, 1e-4)
    assert np.array_equal(x, x0) and Rn.last[0] == 0
    # sizes
    for bad_rhs, bad_x, code in ((rhs[:-1], np.zeros(n), "Input vec dimension"), (rhs, np.zeros(n + 1), "Input and output vec")):
        with pytest.raises(sa.error.IncompatibleMatrixFormat, match=code):
            R.solve(bad_rhs, bad_x, MAX_OUTER, TOL, INNER_MAX, 1e-4)
    # a NaN in the right-hand side ends in a status
    bad = rhs.copy(); bad[n // 3] = np.nan
    assert _run(sa, R, bad, np.zeros(n))[0] == ref.BREAKDOWN


@pytest.mark.parametrize("dt", [F64, C64], ids=lambda d: np.dtype(d).name)
def test_poll_and_entry_points_do_not_change_a_bit(sa, dt):
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = _system(dt)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    P = sa.DiagPrecond.new(_diag(ip, ix, d), t_dtype=dt)
    for inner, pc in (("cg", None), ("cg", P), ("gmres", None)):
        R = sa.Refine.new(A, n, inner=inner, restart=10, precond=pc)
        got = []
        for poll in (1, 8):
            ctx.set("poll", poll)
            x = np.zeros(n, dt)
            got.append(_run(sa, R, rhs, x) + (x,))
        assert got[0][0] == ref.OK and got[0][:4] == got[1][:4] and _same_bits(got[0][4], got[1][4]), inner
        d_rhs = sa.DevVec.from_numpy(rhs); d_x = sa.DevVec.from_numpy(np.zeros(n, dt))
        assert _run(sa, R, d_rhs, d_x) == got[1][:4]
        assert _same_bits(d_x.to_numpy(), got[1][4])


def test_unaligned_device_vectors(sa):
    import torch
    dev = torch.device("cuda", 0)
    ip, ix, d, rhs = _system(F64)
    n = rhs.size
    R = sa.Refine.new(sa.HipCsr.new((n, n), ip, ix, d), n)
    x = np.zeros(n)
    want = _run(sa, R, rhs, x)
    t_rhs = torch.zeros(n + 1, dtype=torch.float64, device=dev); t_rhs[1:] = torch.from_numpy(rhs).to(dev)
    t_x = torch.zeros(n + 1, dtype=torch.float64, device=dev)
    assert t_x[1:].data_ptr() % 16 == 8
    assert _run(sa, R, t_rhs[1:], t_x[1:]) == want
    got = t_x.cpu().numpy()
    assert got[0] == 0.0 and _same_bits(got[1:], x)


def test_every_spmv_knob_on_the_f64_side(sa):
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = _system(F64)
    n = rhs.size
    base = None
    for knob in (None,) + _KNOBS:
        if knob is not None:
            ctx.set(knob, 0)
        A = sa.HipCsr.new((n, n), ip, ix, d)
        R = sa.Refine.new(A, n)
        x = np.zeros(n)
        st, outer, inner_its, res = _run(sa, R, rhs, x)
        print("knob %s = 0: route %s low %s outer %d inner %d res %.2e" % (knob, A.spmv_route()["kernel"], R.low.spmv_route()["kernel"], outer, inner_its, res))
        assert st == ref.OK and _true_res(ip, ix, d, rhs, x) <= TOL
        if base is None:
            base = outer
        assert outer == base, knob
        if knob is not None:
            ctx.set(knob, 1 if knob == "halo_overlap" else -1)
    assert base == _checker(F64).outer


# ------------------------------------------------------------------------------------------------ 6. one larger shape
def _larger():
    from sprsolve_amd import gen
    if "larger" not in _SYS:
        _SYS["larger"] = gen.poisson3d(64, 64, 32, values="random")
    return _SYS["larger"]


LARGER_INNER_MAX, LARGER_OUTER = 4, 16


def test_larger_shape_inner_cg(sa):
    """gen.poisson3d(64, 64, 32, values="random") at tol 1e-10 with inner CG: 131072 rows, the operator in its plain stream.

    That generator keys every off-diagonal on (row, slot), so the matrix is NOT symmetric (max |A - A^T| = 2.0): conjugate
    gradients are no solver for it (run to 200 iterations, inner or alone in f64, they diverge in the numpy checkers: refinement
    ends in status 3 with a residual of 7.9e26 after 30 steps).  Its symmetric part is strictly diagonally dominant, hence positive
    definite, so conj(p).A p > 0 and CG's FIRST steps still shrink the residual: tests/_cg_ref.py in f32 on the normalised
    right-hand side gives |r| = 0.33, 0.17, 0.11, 0.090 after steps 1 .. 4, a minimum of 0.078 at step 7, growth from there.  An
    inner solve capped at LARGER_INNER_MAX = 4 iterations (it ends in InsufficientIterNum, which corrects) therefore contracts
    the outer residual by about 0.1 a step, and tests/_refine_ref.py reaches 1e-10 in LARGER_OUTER = 16 outer steps (64 inner
    iterations; caps of 2, 3, 6, 8 need 22, 16, 18, 22 steps).  max_outer is twice that count."""
    import time
    ip, ix, d, rhs = _larger()
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    R = sa.Refine.new(A, n)
    kw = dict(max_outer=2 * LARGER_OUTER, tol=1e-10, inner_max_iter=LARGER_INNER_MAX, inner_tol=1e-2)
    _run(sa, R, rhs, np.zeros(n), **kw)                                         # the first solve loads the kernels
    x = np.zeros(n)
    t0 = time.perf_counter()
    st, outer, inner_its, res = _run(sa, R, rhs, x, **kw)
    dt = time.perf_counter() - t0
    true = _true_res(ip, ix, d, rhs, x)
    print("larger, inner CG capped at %d: status %d outer %d (checker %d) inner %d res %.3e true %.3e in %.3f s"
          % (LARGER_INNER_MAX, st, outer, LARGER_OUTER, inner_its, res, true, dt))
    assert st == ref.OK and true <= 1e-10 and res <= 1e-10
    assert inner_its == LARGER_INNER_MAX * outer
    assert dt < 0.5                                                             # well under a second


def test_larger_shape_inner_gmres(sa):
    """The same 131072-row system with inner GMRES(10), which needs no symmetry: lengths that are several trips of the grid
    on the f64 side and fewer on the f32 side, the operator in its plain stream."""
    import time
    ip, ix, d, rhs = _larger()
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    R = sa.Refine.new(A, n, inner="gmres", restart=10)
    x = np.zeros(n)
    _run(sa, R, rhs, np.zeros(n), tol=1e-10)                                    # the first solve loads the kernels
    t0 = time.perf_counter()
    st, outer, inner_its, res = _run(sa, R, rhs, x, tol=1e-10)
    dt = time.perf_counter() - t0
    true = _true_res(ip, ix, d, rhs, x)
    print("larger, inner GMRES(10): status %d outer %d inner %d res %.3e true %.3e in %.3f s" % (st, outer, inner_its, res, true, dt))
    assert st == ref.OK and true <= 1e-10 and res <= 1e-10
    assert dt < 1.0
