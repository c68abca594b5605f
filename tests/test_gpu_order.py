"""The orderings on the GPU (sprs_csr_color, sprs_csr_permute, sprs_ilu0_create_ordered; csrc/order.hip, csrc/ilu0.hip) against
the loops of tests/_order_ref.py: the colours, their count and the rounds EXACTLY; the permuted arrays, the ordered factors and
the three ordered solves BIT FOR BIT in all four scalar types; the refusals; and the solvers preconditioned by
ILU0(order="multicolor") — CG and GMRES against the checker with the comparisons and tolerances of tests/test_gpu_ilu.py,
BiCGStab, MINRES and IDR(s) to their tolerance with the true residual formed on the host.

The systems (tests/test_order_cpu.py): poisson3d(12,11,10) and poisson3d(16,15,14), whose larger colours have more than 256 rows
(per-level launches beside a batch of the small ones); convection_diffusion_2d(13,9) and coupled_grid(6,5,3), every colour within
one workgroup (one batched launch per solve); awkward1
(70 colours and more, rows of 70 and of 300 entries, rows with only a diagonal, a non-symmetric pattern); awkward2 (edges from
the superdiagonal alone); n = 1.  MINRES runs on the Poisson system only: it needs a symmetric operator, and the
convection-diffusion matrix is not one."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ilu_ref as ref  # noqa: E402
import _order_ref as oref  # noqa: E402
from _special import fold_spmv  # noqa: E402
from test_gmres_cpu import trace_close as gm_trace_close  # noqa: E402
from test_gpu_ilu import _cg_trace_array, _cg_trace_close, _margin, _run, _true_res  # noqa: E402
from test_ilu_cpu import ALL, F64, GMRES_RESTART, GMRES_TRACE_ROWS, bits, is_single  # noqa: E402
from test_order_cpu import colouring_of, system, typed  # noqa: E402

pytestmark = pytest.mark.gpu

_ids = lambda v: v if isinstance(v, str) else np.dtype(v).name

GRIDS = ["p3:12,11,10", "p3:16,15,14", "cd:13,9", "cg:6,5,3"]
NAMES = GRIDS + ["awkward1", "awkward2", "one"]


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


def _matrix(sa, name, dt):
    ip, ix, d, rhs = colouring_of(name)[:4]
    d, rhs = typed(d, rhs, dt)
    n = ip.size - 1
    return ip, ix, d, rhs, sa.HipCsr.new((n, n), ip, ix, d)


def _perms(name):
    """identity, reversal, a seeded random permutation and the colour-major one."""
    from sprsolve_amd import gen
    ip, ix, d, rhs, col, nc, _ = colouring_of(name)
    n = ip.size - 1
    rnd = np.argsort(gen.splitmix64(0x0DE7, n), kind="stable").astype(np.int32)
    return {"identity": np.arange(n, dtype=np.int32), "reversal": np.arange(n - 1, -1, -1, dtype=np.int32), "random": rnd,
            "colour": oref.color_order(col)}


@functools.lru_cache(maxsize=None)
def ordered_of(name, dtname):
    """The checker's multicolour ILU(0) of a system in a dtype, computed once and shared."""
    ip, ix, d, rhs, col, nc, _ = colouring_of(name)
    d, rhs = typed(d, rhs, dtname)
    o = oref.OrderedIlu(ip, ix, d, oref.color_order(col))
    assert o.status == ref.OK
    return o


# ------------------------------------------------------------------------------------------------ 1. colouring
@pytest.mark.parametrize("seed", [0, 12345])
@pytest.mark.parametrize("name", NAMES)
def test_colours_equal_the_checker(sa, name, seed):
    ip, ix, d, rhs, col, nc, rounds = colouring_of(name, seed)
    n = ip.size - 1
    A = sa.HipCsr.new((n, n), ip, ix, d)
    got, gnc = A.color(seed)
    print("%s seed %d: n %d colours %d rounds %d (checker %d, %d)" % (name, seed, n, gnc, A.color_rounds, nc, rounds))
    assert got.dtype == np.int32 and np.array_equal(got, col)
    assert (gnc, A.color_rounds) == (nc, rounds)
    perm, ptr = sa.HipCsr.color_order(got)
    assert np.array_equal(perm, oref.color_order(col)) and ptr[-1] == n and ptr.size == nc + 1


@pytest.mark.parametrize("name", ["cg:6,5,3", "awkward1"])
def test_colours_do_not_depend_on_the_scalar_type(sa, name):
    want = colouring_of(name)[4]
    for dt in ALL:
        ip, ix, d, rhs, A = _matrix(sa, name, dt)
        got, _ = A.color()
        assert np.array_equal(got, want), np.dtype(dt).name


def test_colouring_an_empty_matrix(sa):
    A = sa.HipCsr.new((0, 0), np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    col, nc = A.color()
    assert col.size == 0 and nc == 0 and A.color_rounds == 0


# ------------------------------------------------------------------------------------------------ 2. permutation
@pytest.mark.parametrize("dt", ALL, ids=_ids)
@pytest.mark.parametrize("name", GRIDS + ["awkward1", "awkward2", "one"])
def test_permuted_arrays_have_the_checkers_bits(sa, name, dt):
    ip, ix, d, rhs, A = _matrix(sa, name, dt)
    n = ip.size - 1
    for what, perm in _perms(name).items():
        bp, bx, bd, _ = oref.permute(ip, ix, d, perm)
        B = A.permute(perm)
        gp, gx, gd = B.to_host()
        assert np.array_equal(gp, bp) and np.array_equal(gx, bx), what
        assert gd.dtype == d.dtype and np.array_equal(bits(gd), bits(bd)), what
        y = np.zeros(n, dt)
        B.mul_vec(rhs, y)
        # the left-to-right fold, on every row the SpMV folds that way: a row of more than 96 entries (LONG_ROW; awkward1 has
        # one) is strided by a wavefront and summed across its lanes, so there B must equal a handle made of the checker's arrays
        short = np.diff(bp) <= 96
        assert np.array_equal(bits(y[short]), bits(fold_spmv(bp, bx, bd, rhs)[short])), what
        assert np.all(short) or name == "awkward1"
        y2 = np.zeros(n, dt)
        sa.HipCsr.new((n, n), bp, bx, bd).mul_vec(rhs, y2)
        assert np.array_equal(bits(y), bits(y2)), what
        back = B.permute(oref.inverse(perm))
        ap, ax, ad = back.to_host()
        assert np.array_equal(ap, ip) and np.array_equal(ax, ix) and np.array_equal(bits(ad), bits(d)), what
    B = A.permute(_perms(name)["colour"])
    A.close()                                                                     # B owns its arrays
    assert np.array_equal(B.to_host()[1], oref.permute(ip, ix, d, _perms(name)["colour"])[1])


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_permuting_unsorted_rows_and_duplicate_columns(sa, dt):
    """Rows stored in any order, rows that repeat a column (twice and five times), a repeated diagonal, and a row of 130 entries
    that is both (the long-row path): every slot of B is written once, duplicates keep their stored order, and the SpMV through
    B is the SpMV through a handle made of the checker's arrays."""
    from sprsolve_amd import gen
    n = 140
    rows = {i: [i, (i * 3 + 1) % n] for i in range(n)}
    rows[3] = [9, 3, 0, 7]                                                       # unsorted
    rows[4] = [4, 8, 4, 1, 8]                                                    # unsorted, a repeated diagonal and a repeated column
    rows[5] = [2, 2, 2, 5, 2, 2]                                                 # one column five times
    rows[6] = [int(c) for c in (gen.splitmix64(0x0DE8, 130) % np.uint64(90))]    # 130 entries over 90 columns, any order
    ip = np.zeros(n + 1, np.int32); np.cumsum([len(rows[i]) for i in range(n)], out=ip[1:])
    ix = np.concatenate([rows[i] for i in range(n)]).astype(np.int32)
    assert len(set(rows[6])) < 130 and np.any(np.diff(ix[ip[6]:ip[7]]) < 0)
    d, rhs = typed(gen.uniform(0x0DE8, ix.size, stream=1), gen.uniform(0x0DE8, n, stream=2), dt)
    A = sa.HipCsr.new((n, n), ip, ix, d)
    perms = {"identity": np.arange(n, dtype=np.int32), "reversal": np.arange(n - 1, -1, -1, dtype=np.int32),
             "random": np.argsort(gen.splitmix64(0x0DE9, n), kind="stable").astype(np.int32)}
    for what, perm in perms.items():
        bp, bx, bd, src = oref.permute(ip, ix, d, perm)
        assert sorted(src) == list(range(ix.size))
        B = A.permute(perm)
        gp, gx, gd = B.to_host()
        assert np.array_equal(gp, bp) and np.array_equal(gx, bx), what
        assert np.array_equal(bits(gd), bits(bd)), what
        assert all(np.all(np.diff(gx[gp[p]:gp[p + 1]]) >= 0) for p in range(n)), what
        y = np.zeros(n, dt); y2 = np.zeros(n, dt)
        B.mul_vec(rhs, y)
        sa.HipCsr.new((n, n), bp, bx, bd).mul_vec(rhs, y2)
        assert np.array_equal(bits(y), bits(y2)), what
    # the identity sorts the rows and nothing else: sorted rows come back as they are
    gp, gx, gd = A.permute(perms["identity"]).to_host()
    assert np.array_equal(gx[ip[0]:ip[3]], ix[ip[0]:ip[3]]) and list(gx[ip[4]:ip[5]]) == [1, 4, 4, 8, 8]
    assert np.array_equal(bits(gd[ip[4]:ip[5]]), bits(d[ip[4]:ip[5]][[3, 0, 2, 1, 4]]))
    # ordered ILU(0) needs distinct ascending columns and says so
    with pytest.raises(ValueError, match="strictly ascending"):
        sa.ILU0.new(A, order=perms["reversal"])


def test_permute_refusals(sa):
    from sprsolve_amd import _lib
    ip, ix, d, rhs, A = _matrix(sa, "cd:13,9", F64)
    n = ip.size - 1
    good = np.arange(n, dtype=np.int32)
    with pytest.raises(ValueError, match="entries"):
        A.permute(good[:-1])
    for bad_value in (-1, n):
        bad = good.copy(); bad[5] = bad_value
        with pytest.raises(ValueError, match=r"perm\[5\]"):
            A.permute(bad)
    dup = good.copy(); dup[7] = 3
    with pytest.raises(ValueError, match="twice"):
        A.permute(dup)
    h = C.c_void_p(1)
    assert _lib.lib().sprs_csr_permute(A.h, dup.ctypes.data_as(C.c_void_p), n, C.byref(h)) == _lib.INVALID_ARGUMENT and not h.value
    R = sa.HipCsr.new((2, 3), np.array([0, 2, 4], np.int32), np.array([0, 1, 0, 1], np.int32), np.ones(4))
    with pytest.raises(sa.error.IncompatibleMatrixFormat):
        R.permute(np.arange(2, dtype=np.int32))
    with pytest.raises(sa.error.IncompatibleMatrixFormat):
        R.color()
    with pytest.raises(sa.error.IncompatibleMatrixFormat):
        sa.ILU0.new(R, order="multicolor")


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
        perm = np.arange(n, dtype=np.int32)
        for call in (lambda: sa.HipCsr.color(A), lambda: sa.HipCsr.permute(A, perm), lambda: sa.ILU0.new(A, order="multicolor"),
                     lambda: sa.ILU0.new(A, order=perm)):
            with pytest.raises(ValueError, match="distributed"):
                call()
    finally:
        comm.close()


# ------------------------------------------------------------------------------------------------ 3. ordered ILU(0)
def _launches(level):
    """The header's plan: a level of more than 256 rows is a launch, a run of up to 128 consecutive smaller levels is one."""
    size = np.bincount(level)
    launches = run = 0
    for sz in size:
        if sz > 256:
            launches += 1; run = 0
        else:
            launches += run % 128 == 0; run += 1
    return launches


@pytest.mark.parametrize("dt", ALL, ids=_ids)
@pytest.mark.parametrize("name", GRIDS + ["awkward1", "awkward2"])
def test_ordered_factors_and_solves_have_the_checkers_bits(sa, name, dt):
    ip, ix, d, rhs, A = _matrix(sa, name, dt)
    n = ip.size - 1
    nc = colouring_of(name)[5]
    o = ordered_of(name, np.dtype(dt).name)
    P = sa.ILU0.new(A, order="multicolor")
    lv = P.levels
    print("%s %s: colours %d %s" % (name, np.dtype(dt).name, nc, lv))
    assert np.array_equal(P.order, o.perm) and P.sweeps == 0
    assert (lv["lower_levels"], lv["upper_levels"]) == o.levels() and max(o.levels()) <= nc
    want_launches = tuple(_launches(l) for l in ref.levels(o.bp, o.bx))
    assert (lv["lower_launches"], lv["upper_launches"]) == want_launches
    if name in ("cd:13,9", "cg:6,5,3", "awkward1", "awkward2"):
        assert want_launches == (1, 1)                                           # every level fits one workgroup: one batch
    if name.startswith("p3"):
        assert min(want_launches) >= 3                                           # colours of more than 256 rows: a launch each
    assert np.array_equal(bits(P.factors()), bits(o.val))
    A.close()                                                                    # the handle borrows nothing from A
    apply = {0: P.mul_vec, 1: P.solve_lower, 2: P.solve_upper}
    for which in (1, 2, 0):
        want = o.solve(which, rhs)
        out = np.zeros(n, dt)
        apply[which](rhs, out)                                                   # host entry point
        assert np.array_equal(bits(out), bits(want)), (which, "host")
        d_in = sa.DevVec.from_numpy(rhs); d_out = sa.DevVec.from_numpy(np.zeros(n, dt))
        apply[which](d_in, d_out)                                                # device entry point
        assert np.array_equal(bits(d_out.to_numpy()), bits(want)), (which, "device")
        assert np.array_equal(bits(d_in.to_numpy()), bits(rhs)), (which, "input kept")
        apply[which](d_in, d_in)                                                 # in == out
        assert np.array_equal(bits(d_in.to_numpy()), bits(want)), (which, "in place")
        h_io = rhs.copy()
        apply[which](h_io, h_io)                                                 # in == out through the host entry point
        assert np.array_equal(bits(h_io), bits(want)), (which, "host, in place")


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_explicit_permutations(sa, dt):
    ip, ix, d, rhs, A = _matrix(sa, "cd:13,9", dt)
    n = ip.size - 1
    nat = sa.ILU0.new(A)
    assert nat.order is None
    for what in ("identity", "random", "reversal"):
        perm = _perms("cd:13,9")[what]
        o = oref.OrderedIlu(ip, ix, d, perm)
        P = sa.ILU0.new(A, order=perm)
        assert np.array_equal(P.order, perm)
        assert np.array_equal(bits(P.factors()), bits(o.val)), what
        lv = P.levels
        assert (lv["lower_levels"], lv["upper_levels"]) == o.levels(), what
        for which, fn, fn_nat in ((1, P.solve_lower, nat.solve_lower), (2, P.solve_upper, nat.solve_upper), (0, P.mul_vec, nat.mul_vec)):
            out = np.zeros(n, dt)
            fn(rhs, out)
            assert np.array_equal(bits(out), bits(o.solve(which, rhs))), (what, which)
            if what == "identity":                                               # the bits of order=None
                out_nat = np.zeros(n, dt)
                fn_nat(rhs, out_nat)
                assert np.array_equal(bits(out), bits(out_nat)), which
        if what == "identity":
            assert np.array_equal(bits(P.factors()), bits(nat.factors())) and P.levels == nat.levels


def test_red_black_has_two_levels(sa):
    ip, ix, d, rhs, A = _matrix(sa, "p3:12,11,10", F64)
    g = np.arange(12 * 11 * 10)
    colour = (g % 12 + (g // 12) % 11 + g // 132) % 2
    perm, ptr = sa.color_order(colour)
    P = sa.ILU0.new(A, order=perm)
    lv = P.levels
    assert (lv["lower_levels"], lv["upper_levels"]) == (2, 2)
    o = oref.OrderedIlu(ip, ix, d, perm)
    out = np.zeros(rhs.size)
    P.mul_vec(rhs, out)
    assert np.array_equal(bits(P.factors()), bits(o.val)) and np.array_equal(bits(out), bits(o.solve(0, rhs)))


def test_ordered_creation_errors(sa):
    from sprsolve_amd import _lib
    ip, ix, d, rhs, A = _matrix(sa, "cd:13,9", F64)
    n = ip.size - 1
    good = np.arange(n, dtype=np.int32)
    with pytest.raises(ValueError, match="sweeps"):
        sa.ILU0.new(A, sweeps=3, order="multicolor")
    with pytest.raises(ValueError, match="sweeps"):
        sa.ILU0.new(A, sweeps=3, order=good)
    with pytest.raises(ValueError):
        sa.ILU0.new(A, order="rcm")
    dup = good.copy(); dup[0] = 1
    for bad, text in ((good[:-1], "entries"), (dup, "twice"), (np.where(good == 4, n, good), r"perm\[4\]")):
        with pytest.raises(ValueError, match=text):
            sa.ILU0.new(A, order=bad)
    h = C.c_void_p(1); row = C.c_int64(-7)
    assert _lib.lib().sprs_ilu0_create_ordered(A.h, 0, 7, None, 0, C.byref(h), C.byref(row)) == _lib.INVALID_ARGUMENT and not h.value
    # the 2 x 2 all-ones matrix: the zero pivot is row 1 in natural order, and row 0 of A under perm = [1, 0]
    ip2 = np.array([0, 2, 4], np.int32); ix2 = np.array([0, 1, 0, 1], np.int32)
    for dt in ALL:
        A2 = sa.HipCsr.new((2, 2), ip2, ix2, np.ones(4, dt))
        with pytest.raises(sa.error.ZeorDiagonalElem) as ei:
            sa.ILU0.new(A2)
        assert ei.value.row == 1
        with pytest.raises(sa.error.ZeorDiagonalElem) as ei:
            sa.ILU0.new(A2, order=np.array([1, 0], np.int32))
        assert ei.value.row == 0
    ip3 = np.array([0, 2, 3, 5, 6], np.int32); ix3 = np.array([0, 1, 0, 1, 2, 2], np.int32)   # rows 1 and 3 store no diagonal
    with pytest.raises(sa.error.ZeorDiagonalElem) as ei:
        sa.ILU0.new(sa.HipCsr.new((4, 4), ip3, ix3, np.ones(6)), order=np.array([3, 2, 1, 0], np.int32))
    assert ei.value.row == 3                                                      # the first of them in the new order
    one = sa.ILU0.new(sa.HipCsr.new((1, 1), np.array([0, 1], np.int32), np.array([0], np.int32), np.array([4.0])), order="multicolor")
    out = np.zeros(1)
    one.mul_vec(np.array([2.0]), out)
    assert out[0] == 0.5 and list(one.order) == [0]


# ------------------------------------------------------------------------------------------------ 4. the solvers
def test_cg_literal_follows_the_checker_and_fused_follows_literal(sa):
    dt = F64
    name = "p3:12,11,10"
    ip, ix, d, rhs, A = _matrix(sa, name, dt)
    n = rhs.size
    tol = 1e-10
    o = ref.cg(ip, ix, d, rhs, np.zeros(n, dt), 400, tol, prec=ordered_of(name, "float64"))
    assert o.status == ref.OK
    max_iter = 2 * o.its
    P = sa.ILU0.new(A, order="multicolor")
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
    print("cg+multicolour ilu: literal its %d (checker %d) res %.3e (checker %.3e) max|x - checker| %.3e; fused its %d res %.3e true %.3e max|dx| %.3e"
          % (il, o.its, rl, o.res, err, itf, rf, true_res, np.max(np.abs(xf - xl))))
    # literal against the checker
    assert (sl, il) == (o.status, o.its)
    assert tl.shape == want.shape == (o.its - 1, 8)
    assert _cg_trace_close(tl, want, rtol=1e-9, atol=1e-12)
    assert err <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
    assert np.isclose(rl, o.res, rtol=1e-9, atol=1e-12)
    # fused against literal
    assert sf == sl == ref.OK
    assert abs(itf - il) <= _margin(il)
    assert true_res <= 10 * tol
    assert np.max(np.abs(xf - xl)) <= 1e-7 * np.max(np.abs(xl))
    k = min(tf.shape[0], tl.shape[0])
    assert k >= il - 2 and _cg_trace_close(tf[:k], tl[:k], rtol=1e-9, atol=1e-12)
    # Jacobi beside it needs more iterations
    rows = np.repeat(np.arange(n), np.diff(ip))
    J = sa.DiagPrecond.new(d[rows == ix].real.copy(), t_dtype=d.dtype)
    xj = np.zeros(n, dt)
    stj, itj, _ = _run(sa, sa.CG.new(A, n), J, rhs, xj, 400, tol)
    assert stj == ref.OK and itj > itf


def test_gmres_literal_follows_the_checker_and_fused_follows_literal(sa):
    dt = F64
    name = "cd:13,9"
    ip, ix, d, rhs, A = _matrix(sa, name, dt)
    n = rhs.size
    tol = 1e-10
    m = GMRES_RESTART
    o = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), 400, tol, restart=m, prec=ordered_of(name, "float64"))
    assert o.status == ref.OK and o.its > m                                      # at least two cycles
    max_iter = 2 * o.its
    P = sa.ILU0.new(A, order="multicolor")
    out = {}
    for mode in ("literal", "fused"):
        s = sa.GMRES.new(A, n, m); s.set_mode(mode); s.set_trace(max_iter)
        x = np.zeros(n, dt)
        st, its, res = _run(sa, s, P, rhs, x, max_iter, tol)
        out[mode] = (st, its, res, x, s.trace(), _true_res(ip, ix, d, rhs, x))
    (sl, il, rl, xl, tl, true_l), (sf, itf, rf, xf, tf, true_f) = out["literal"], out["fused"]
    want = np.array([[t[0], t[1], t[2], t[3].real, t[3].imag, t[4], t[5].real, t[5].imag] for t in o.trace]).reshape(-1, 8)
    err = np.max(np.abs(xl - o.x))
    print("gmres+multicolour ilu: literal its %d (checker %d) res %.3e (checker %.3e) true %.3e max|x - checker| %.3e; fused its %d res %.3e true %.3e"
          % (il, o.its, rl, o.res, true_l, err, itf, rf, true_f))
    # literal against the checker
    assert sl == o.status == ref.OK
    assert abs(il - o.its) <= _margin(o.its)
    assert tl.shape == (il, 8) and np.array_equal(tl[:, 0], np.arange(1, il + 1))
    assert rl <= tol and true_l <= 10 * tol
    k = min(GMRES_TRACE_ROWS, il, o.its)
    assert gm_trace_close(tl[:k], want[:k], rtol=1e-9, atol=1e-12)
    assert err <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
    assert il == o.its and np.isclose(rl, o.res, rtol=1e-9, atol=1e-12)
    # fused against literal
    assert sf == sl == ref.OK
    assert abs(itf - il) <= _margin(il)
    assert rf <= tol and true_f <= 10 * tol
    assert tf.shape == (itf, 8) and np.array_equal(tf[:, 0], np.arange(1, itf + 1))
    k = min(GMRES_TRACE_ROWS, itf, il)
    assert np.max(np.abs(xf - xl)) <= 1e-7 * np.max(np.abs(xl))
    assert gm_trace_close(tf[:k], tl[:k], rtol=1e-9, atol=1e-12)
    assert itf == il and np.isclose(rf, rl, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("solver,name", [("BiCGStab", "p3:12,11,10"), ("BiCGStab", "cd:13,9"), ("IDRS", "p3:12,11,10"), ("IDRS", "cd:13,9"),
                                         ("MinRes", "p3:12,11,10")])
def test_the_other_solvers_converge_with_it(sa, solver, name):
    ip, ix, d, rhs, A = _matrix(sa, name, F64)
    n = rhs.size
    tol = 1e-10
    P = sa.ILU0.new(A, order="multicolor")
    s = getattr(sa, solver).new(A, n)
    x = np.zeros(n)
    st, its, res = _run(sa, s, P, rhs, x, 400, tol)
    true_res = _true_res(ip, ix, d, rhs, x)
    print("%s + multicolour ilu on %s: its %d res %.3e true %.3e" % (solver, name, its, res, true_res))
    assert st == ref.OK and res <= tol and true_res <= 10 * tol
