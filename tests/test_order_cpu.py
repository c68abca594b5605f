"""The orderings' checker (tests/_order_ref.py) checked on the CPU: the Jones-Plassmann rounds give the greedy colouring, the
colourings are proper, the colour-major permutation leaves at most as many dependency levels as colours, multicolour ILU(0) still
beats Jacobi in the checker's own CG and GMRES, and the library exports the three entry points.  The systems of
tests/test_gpu_order.py are built here."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ilu_ref as ref  # noqa: E402
import _order_ref as oref  # noqa: E402


# ------------------------------------------------------------------------------------------------ the systems
def awkward1(n=320, seed=0x0DE5):
    """Non-symmetric pattern, strictly diagonally dominant: rows 0 .. 9 hold only their diagonal; rows 100 .. 169 hold a dense
    70 x 70 diagonal block (70 mutually adjacent vertices: at least 70 colours, past one 64-colour window, and rows of more
    than 64 entries); row 200 holds columns 0 .. 299 (more than 256 entries); every other row its diagonal, column
    (7 i + 3) mod n and (odd rows) column i + 1.  -> (indptr, indices, data f64, rhs)."""
    from sprsolve_amd import gen
    R, Cc = [], []
    for i in range(n):
        if i < 10:
            c = {i}
        elif 100 <= i < 170:
            c = set(range(100, 170))
        elif i == 200:
            c = set(range(300))
        else:
            c = {i, (7 * i + 3) % n}
            if i % 2 and i + 1 < n:
                c.add(i + 1)
        c = sorted(c)
        R += [i] * len(c); Cc += c
    R = np.array(R); Cc = np.array(Cc)
    v = gen.uniform_keys(seed, R * n + Cc, stream=3)
    absrow = np.zeros(n)
    np.add.at(absrow, R[R != Cc], np.abs(v[R != Cc]))
    v[R == Cc] = 1.0 + absrow
    ip = np.zeros(n + 1, np.int64); np.cumsum(np.bincount(R, minlength=n), out=ip[1:])
    return ip.astype(np.int32), Cc.astype(np.int32), v, gen.uniform(seed, n, stream=4)


def awkward2(n=150, seed=0x0DE6):
    """The diagonal and the first superdiagonal only: every edge of the graph comes from a stored (i, i + 1) whose mirror is
    not stored."""
    from sprsolve_amd import gen
    ip = np.minimum(2 * np.arange(n + 1), 2 * n - 1).astype(np.int32)
    ix = np.stack([np.arange(n), np.arange(1, n + 1)], axis=1).ravel()[:2 * n - 1].astype(np.int32)
    d = gen.uniform(seed, 2 * n - 1, stream=5)
    d[0::2] = 2.0 + np.abs(d[0::2])
    return ip, ix, d, gen.uniform(seed, n, stream=6)


def system(name):
    from sprsolve_amd import gen
    if name == "awkward1":
        return awkward1()
    if name == "awkward2":
        return awkward2()
    if name == "one":
        return np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.0]), np.array([1.0])
    kind, args = name.split(":")
    args = [float(a) if "." in a else int(a) for a in args.split(",")]
    if kind == "p3":
        ip, ix, d, _ = gen.poisson3d(*args)
        return ip, ix, d, gen.uniform(gen.SEED, ip.size - 1, stream=84)
    if kind == "cd":
        return gen.convection_diffusion_2d(args[0], args[1], *([] if len(args) == 2 else [args[2], args[3]]))
    if kind == "cg":
        return gen.coupled_grid(*args)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def colouring_of(name, seed=0):
    """(ip, ix, d, rhs, colours, ncolours, rounds) by the round-by-round simulation, computed once and shared (read-only)."""
    ip, ix, d, rhs = system(name)
    col, nc, rounds = oref.jones_plassmann(ip, ix, seed)
    for a in (ip, ix, d, rhs, col):
        a.setflags(write=False)
    return ip, ix, d, rhs, col, nc, rounds


def typed(d, rhs, dt):
    """The system's values in dtype dt: the complex types turn every entry by 1 + 0.25i and the rhs by 1 - 0.5i."""
    dt = np.dtype(dt)
    if dt.kind == "c":
        return (d * (1.0 + 0.25j)).astype(dt), (rhs * (1.0 - 0.5j)).astype(dt)
    return d.astype(dt), rhs.astype(dt)


TABLE = ["p3:12,11,10", "p3:24,22,20", "cd:48,40", "cd:48,40,2.0,0.2", "cg:12,11,3"]
# (colours, levels after P, natural levels) where the grids give them in closed form
EXPECT = {"p3:12,11,10": (31, 31), "p3:24,22,20": (64, 64), "cd:48,40": (87, 87), "cd:48,40,2.0,0.2": (87, 87), "cg:12,11,3": (66, 66)}


# ------------------------------------------------------------------------------------------------ 1. the colouring
@pytest.mark.parametrize("name", TABLE + ["awkward1", "awkward2", "one"])
def test_rounds_give_the_greedy_colouring(name):
    ip, ix, d, rhs, col, nc, rounds = colouring_of(name)
    g, gnc = oref.greedy(ip, ix, 0)
    n = ip.size - 1
    print("%s: n %d colours %d rounds %d" % (name, n, nc, rounds))
    assert np.array_equal(col, g) and nc == gnc
    assert oref.is_proper(ip, ix, col)
    assert col.min() >= 0 and set(col) == set(range(nc))     # first-fit leaves no colour unused
    assert 1 <= rounds <= n
    if name == "awkward1":
        assert nc >= 70 and np.diff(ip).max() == 300 and np.sum(np.diff(ip) == 1) >= 10
    if name == "awkward2":
        assert nc in (2, 3)                                   # a path: first-fit in a random order needs at most 3
    if name == "one":
        assert (list(col), nc, rounds) == ([0], 1, 1)


def test_another_seed_gives_another_proper_colouring():
    ip, ix, d, rhs, col0, _, _ = colouring_of("cd:48,40")
    _, _, _, _, col1, nc1, _ = colouring_of("cd:48,40", 12345)
    g, gnc = oref.greedy(ip, ix, 12345)
    assert np.array_equal(col1, g) and nc1 == gnc and oref.is_proper(ip, ix, col1)
    assert not np.array_equal(col0, col1)


def test_weight_is_the_generators_splitmix64():
    from sprsolve_amd import gen
    for seed in (0, 12345, gen.SEED, 2**64 - 1):
        want = gen.splitmix64_keys(seed, np.arange(50))
        assert [oref.weight(seed, i) for i in range(50)] == [int(v) for v in want]


def test_empty_matrix_has_no_colours():
    ip = np.zeros(1, np.int32); ix = np.zeros(0, np.int32)
    assert oref.jones_plassmann(ip, ix)[1:] == (0, 0) and oref.greedy(ip, ix)[1] == 0


# ------------------------------------------------------------------------------------------------ 2. the permutation and its levels
@pytest.mark.parametrize("name", TABLE + ["awkward1", "awkward2"])
def test_colour_major_levels_are_at_most_the_colours(name):
    ip, ix, d, rhs, col, nc, _ = colouring_of(name)
    perm = oref.color_order(col)
    bp, bx, bd, src = oref.permute(ip, ix, d, perm)
    lv = ref.level_counts(bp, bx)
    nat = ref.level_counts(ip, ix)
    print("%s: colours %d levels after P %s natural %s" % (name, nc, lv, nat))
    assert max(lv) <= nc
    if name in EXPECT:
        assert nat == EXPECT[name]
    n = ip.size - 1
    assert sorted(perm) == list(range(n))
    assert all(np.all(np.diff(bx[bp[p]:bp[p + 1]]) > 0) for p in range(n))        # columns strictly ascending
    import scipy.sparse as sp
    A = sp.csr_matrix((d, ix, ip), shape=(n, n))
    B = A[perm][:, perm].tocsr(); B.sort_indices()
    assert np.array_equal(B.indptr, bp) and np.array_equal(B.indices, bx) and np.array_equal(B.data, bd)
    assert np.array_equal(d[src], bd)


def test_permuting_back_gives_the_matrix():
    ip, ix, d, rhs, col, nc, _ = colouring_of("awkward1")
    perm = oref.color_order(col)
    bp, bx, bd, _ = oref.permute(ip, ix, d, perm)
    ap, ax, ad, _ = oref.permute(bp, bx, bd, oref.inverse(perm))
    assert np.array_equal(ap, ip) and np.array_equal(ax, ix) and np.array_equal(ad, d)


def test_identity_order_is_the_natural_ilu():
    ip, ix, d, rhs = system("cd:13,9")
    n = ip.size - 1
    o = oref.OrderedIlu(ip, ix, d, np.arange(n, dtype=np.int32))
    f = ref.ilu0(ip, ix, d)
    assert o.status == ref.OK and np.array_equal(o.val, f.val)
    assert np.array_equal(o.solve(0, rhs), ref.Applier(ip, ix, f.val).solve(0, rhs))


def test_ordered_factors_sit_at_the_matrix_positions():
    """Entry (i, j) holds l where ord(j) < ord(i) and u otherwise: L U of the permuted matrix reproduces A on its pattern."""
    ip, ix, d, rhs, col, nc, _ = colouring_of("cd:13,9")
    perm = oref.color_order(col); ordv = oref.inverse(perm)
    o = oref.OrderedIlu(ip, ix, d, perm)
    n = ip.size - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    Lm = np.eye(n); Um = np.zeros((n, n))
    low = ordv[ix] < ordv[rows]
    Lm[ordv[rows[low]], ordv[ix[low]]] = o.val[low]
    Um[ordv[rows[~low]], ordv[ix[~low]]] = o.val[~low]
    LU = Lm @ Um
    assert np.allclose(LU[ordv[rows], ordv[ix]], d, rtol=1e-13, atol=1e-13)
    assert o.row == -1 and max(o.levels()) <= nc


def test_zero_pivot_is_reported_in_the_matrix_numbering():
    ip = np.array([0, 2, 4], np.int32); ix = np.array([0, 1, 0, 1], np.int32); d = np.ones(4)
    assert ref.ilu0(ip, ix, d)[:2] == (ref.ZERO_DIAGONAL, 1)
    o = oref.OrderedIlu(ip, ix, d, [1, 0])
    assert (o.status, o.row) == (ref.ZERO_DIAGONAL, 0)


# ------------------------------------------------------------------------------------------------ 3. the method still pays
@functools.lru_cache(maxsize=None)
def counts(name):
    """(Jacobi, multicolour ILU(0)) iterations of the checker's own CG (the Poisson matrix) / GMRES(30), f64, x0 = 0, tol 1e-8."""
    ip, ix, d, rhs, col, nc, _ = colouring_of(name)
    n = ip.size - 1
    o = oref.OrderedIlu(ip, ix, d, oref.color_order(col))
    assert o.status == ref.OK
    out = []
    for prec in (ref.jacobi(ip, ix, d), o):
        if name.startswith("p3"):
            r = ref.cg(ip, ix, d, rhs, np.zeros(n), 1000, 1e-8, prec=prec)
        else:
            r = ref.gmres(ip, ix, d, rhs, np.zeros(n), 1000, 1e-8, restart=30, prec=prec)
        assert r.status == ref.OK
        out.append(r.its)
    return tuple(out)


@pytest.mark.parametrize("name", ["p3:12,11,10", "cd:48,40"])
def test_multicolour_ilu_needs_fewer_iterations_than_jacobi(name):
    jac, mc = counts(name)
    print("%s: Jacobi %d, multicolour ILU(0) %d" % (name, jac, mc))
    assert mc < jac


# ------------------------------------------------------------------------------------------------ 4. the library
def test_library_exports_the_entry_points():
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    h = C.c_void_p(1); nc = C.c_int64(); rounds = C.c_int64(); row = C.c_int64()
    perm = np.zeros(1, np.int32)
    p = perm.ctypes.data_as(C.c_void_p)
    assert L.sprs_csr_color(None, 0, p, C.byref(nc), C.byref(rounds)) == _lib.INVALID_ARGUMENT == 7
    assert L.sprs_csr_permute(None, p, 1, C.byref(h)) == 7
    assert L.sprs_ilu0_create_ordered(None, 0, _lib.ORDER_MULTICOLOR, None, 0, C.byref(h), C.byref(row)) == 7
    assert L.sprs_ilu0_create_ordered(None, 0, _lib.ORDER_PERM, p, 1, C.byref(h), C.byref(row)) == 7
    assert L.sprs_ilu0_order(None, None) == -1
    import sprsolve_amd as sa
    perm, ptr = sa.color_order(np.array([1, 0, 1, 2, 0], np.int32))
    assert list(perm) == [1, 4, 0, 2, 3] and list(ptr) == [0, 2, 4, 5] and perm.dtype == np.int32
    assert list(sa.inverse_permutation(perm)) == [2, 0, 3, 4, 1]
    assert sa.HipCsr.color_order([0, 0])[0].tolist() == [0, 1]
