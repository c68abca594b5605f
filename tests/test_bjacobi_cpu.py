"""The block-Jacobi checker (tests/_bjacobi_ref.py) checked on the CPU against independent arithmetic — every inverse block against
np.linalg.inv in double, a regular block with a zero (0, 0) entry, a singular block and its reported row, a reducible block — the
properties of gen.coupled_grid, the iteration counts of the project's checkers (tests/_ilu_ref.py's cg and gmres,
tests/_krylov_prec_ref.py's bicgstab and minres) under its apply, the conditions 2 * (block-Jacobi count) <= Jacobi count, and the
null-handle answers of the library's entry points.  The counts stand behind every max_iter of tests/test_gpu_bjacobi.py: at least
twice the count, the rule of tests/test_gpu_cg.py.  The systems, the checker's inverses and runs and the trace prefixes of the GPU
file are built here, once, and shared read-only."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bjacobi_ref as br  # noqa: E402
import _ilu_ref as ref  # noqa: E402
import _krylov_prec_ref as kp  # noqa: E402
from test_ilu_cpu import ALL, C32, C64, F32, F64, bits, is_single, tol_of  # noqa: E402,F401
from test_krylov_prec_cpu import gpu_tols, rows_close  # noqa: E402

_ids = lambda v: v if isinstance(v, str) else np.dtype(v).name
GMRES_RESTART = 10
REAL = [F64, F32]
# name -> (block size, the scalar types it is run in, the solvers it is run with)
SYSTEMS = {"cgrid": (3, ALL, ("cg", "bicgstab", "gmres", "minres")), "cdline": (16, REAL, ("bicgstab", "gmres"))}

# the checkers' counts, x0 = 0, f64 / c64 at tol 1e-10 and f32 / c32 at 1e-5: solver -> (Jacobi, block-Jacobi).  MINRES: the real
# types only (the header says why)
BJ_COUNTS = {
    "cgrid": {
        "float64": {"cg": (252, 67), "bicgstab": (203, 52), "gmres": (676, 88), "minres": (241, 60)},
        "complex128": {"cg": (252, 67), "bicgstab": (218, 46), "gmres": (927, 106)},
        "float32": {"cg": (169, 40), "bicgstab": (138, 28), "gmres": (326, 40), "minres": (147, 32)},
        "complex64": {"cg": (159, 39), "bicgstab": (144, 28), "gmres": (486, 47)},
    },
    "cdline": {
        "float64": {"bicgstab": (57, 17), "gmres": (148, 43)},
        "float32": {"bicgstab": (42, 12), "gmres": (93, 25)},
    },
}
CASES = [(name, dt, solver) for name, (_, dts, solvers) in SYSTEMS.items() for dt in dts for solver in solvers
         if not (solver == "minres" and np.dtype(dt).kind == "c")]


def eps_of(dt):
    return float(np.finfo(np.float32 if is_single(dt) else np.float64).eps)


# ------------------------------------------------------------------------------------------------ the systems
@functools.lru_cache(maxsize=None)
def system(name, dtname):
    """"cgrid": gen.coupled_grid(12, 11, 3), blocks of 3 (a node each); "cdline": gen.convection_diffusion_2d(24, 16, cx=2.0, cy=0.2),
    blocks of 16 (a grid line each); "cgrid40": gen.coupled_grid(40, 33, 3), 3960 rows."""
    from sprsolve_amd import gen
    dt = np.dtype(dtname).type
    if name == "cgrid":
        ip, ix, d, rhs = gen.coupled_grid(12, 11, 3, dtype=dt)
    elif name == "cgrid40":
        ip, ix, d, rhs = gen.coupled_grid(40, 33, 3, dtype=dt)
    elif name == "cdline":
        ip, ix, d, rhs = gen.convection_diffusion_2d(24, 16, cx=2.0, cy=0.2, dtype=dt)
    else:
        raise KeyError(name)
    ip = ip.astype(np.int32); ix = ix.astype(np.int32)
    for a in (ip, ix, d, rhs):
        a.setflags(write=False)
    return ip, ix, d, rhs


def block_size_of(name):
    return 3 if name == "cgrid40" else SYSTEMS[name][0]


@functools.lru_cache(maxsize=None)
def inverse_of(name, dtname):
    """The checker's inverse blocks of a named system, computed once and shared (read-only)."""
    ip, ix, d, _ = system(name, dtname)
    inv = br.bjacobi(ip, ix, d, block_size=block_size_of(name))
    assert inv.status == br.OK, (name, dtname, inv[:2])
    for X in inv.blocks:
        X.setflags(write=False)
    return inv


@functools.lru_cache(maxsize=None)
def applier(name, dtname):
    inv = inverse_of(name, dtname)
    return br.Applier(inv.block_ptr, inv.blocks)


def max_iter_of(solver, name, dtname, kind="bjacobi"):
    """At least twice the checker's count (tests/test_gpu_cg.py's rule)."""
    return 2 * BJ_COUNTS[name][dtname][solver][kind == "bjacobi"] + 2


@functools.lru_cache(maxsize=None)
def checker_run(solver, name, dtname, kind="bjacobi", sums="numpy"):
    ip, ix, d, rhs = system(name, dtname)
    dt = np.dtype(dtname).type
    x0 = np.zeros(rhs.size, dt)
    mi, tol = max_iter_of(solver, name, dtname, kind), tol_of(dt)
    M = applier(name, dtname) if kind == "bjacobi" else ref.jacobi(ip, ix, d)
    if solver == "cg":
        return br.cg(ip, ix, d, rhs, x0, mi, tol, prec=M, sums=sums)       # (sums="numpy": the bits of tests/_ilu_ref.py's cg)
    if solver == "gmres":
        return ref.gmres(ip, ix, d, rhs, x0, mi, tol, restart=GMRES_RESTART, prec=M, sums=sums)
    o = getattr(kp, solver)(ip, ix, d, rhs, x0, mi, tol, prec=M, sums=sums)
    o.x.setflags(write=False); o.trace.setflags(write=False)
    return o


def _true_res(ip, ix, d, rhs, x):
    wide = np.complex128 if rhs.dtype.kind == "c" else np.float64
    A = ref._matvec(ip, ix, d.astype(wide))
    return float(np.linalg.norm(rhs.astype(wide) - A(x.astype(wide))) / np.linalg.norm(rhs.astype(wide)))


@functools.lru_cache(maxsize=None)
def minres_true_bound(name, dtname):
    """What a GPU MINRES run's TRUE residual may be: tests/test_gpu_krylov_prec.py's 10 tol, or twice the checker's own true
    residual where that is more.  The reference's MINRES (minres.rs, restated in tests/_krylov_prec_ref.py) reports
    e_k = |r_0|_2 * prod |s_i|, and prod |s_i| is the decrease of the residual in the M-norm, so the true 2-norm residual may
    exceed e_k by up to sqrt(cond(M)) (31.6 on gen.coupled_grid, whose blocks inherit the spread 1e3 of C): the checker itself
    stops at a true residual of 1.3e-9 for tol 1e-10.  ILU(0), AMG and FSAI are well scaled and never met this.  The GPU runs the
    same recurrence with its sums in another order; the checker's two orders of summation differ by less than a tenth in the true
    residual (asserted below), so a factor of two over the larger of them is a generous margin for a third order and far below
    the theoretical 31.6."""
    ip, ix, d, rhs = system(name, dtname)
    t = [_true_res(ip, ix, d, rhs, checker_run("minres", name, dtname, "bjacobi", sums).x) for sums in ("numpy", "pairwise")]
    return max(10 * tol_of(np.dtype(dtname).type), 2 * max(t)), t


def _herm(X):
    X = np.asarray(X).astype(np.complex128 if X.dtype.kind == "c" else np.float64)
    return (X + X.conj().T) / 2


def gmres_trace_array(trace):
    return np.array([[t[0], t[1], t[2], t[3].real, t[3].imag, t[4], t[5].real, t[5].imag] for t in trace]).reshape(-1, 8)


@functools.lru_cache(maxsize=None)
def trace_prefix(solver, name, dtname):
    """The trace rows the GPU test may compare (tests/test_fsai_cpu.py::trace_prefix, the rule of tests/test_ilu_cpu.py's
    GMRES_TRACE_ROWS): the leading rows on which the checker against itself with its sums taken pairwise holds a TENTH of the GPU
    tolerance."""
    rtol, atol = gpu_tols(np.dtype(dtname).type)
    a, b = checker_run(solver, name, dtname), checker_run(solver, name, dtname, "bjacobi", "pairwise")
    if solver == "gmres":
        from test_gmres_cpu import trace_close
        ta, tb = gmres_trace_array(a.trace), gmres_trace_array(b.trace)
        k = 0
        while k < min(len(ta), len(tb)) and trace_close(ta[:k + 1], tb[:k + 1], rtol=rtol / 10, atol=atol / 10):
            k += 1
        return k
    if solver == "cg":
        from test_gpu_ilu import _cg_trace_array
        return rows_close(_cg_trace_array(a.trace), _cg_trace_array(b.trace), rtol / 10, atol / 10)
    return rows_close(a.trace, b.trace, rtol / 10, atol / 10)


@functools.lru_cache(maxsize=None)
def whole_run_is_comparable(solver, name, dtname):
    """The prefix is the whole run: the checker against itself under a change of summation order takes the same number of steps,
    holds a tenth of the GPU tolerance on every trace row and on the reported residual.  Only then may a GPU test demand the
    reported residual itself at that tolerance (np.isclose), as tests/test_gpu_ilu.py does for its short runs; otherwise the
    residual is compared through the trace rows of the prefix and bounded by tol at the end."""
    rtol, atol = gpu_tols(np.dtype(dtname).type)
    a, b = checker_run(solver, name, dtname), checker_run(solver, name, dtname, "bjacobi", "pairwise")
    return bool(a.its == b.its and len(a.trace) == len(b.trace) == trace_prefix(solver, name, dtname)
                and np.isclose(a.res, b.res, rtol=rtol / 10, atol=atol / 10))


def dense_csr(W, keep=None):
    """A dense matrix as CSR, with the entries where `keep` is False left out of the pattern."""
    W = np.asarray(W)
    keep = np.ones(W.shape, bool) if keep is None else keep
    r, c = np.nonzero(keep)
    ip = np.zeros(W.shape[0] + 1, np.int32); np.cumsum(np.bincount(r, minlength=W.shape[0]), out=ip[1:])
    return ip, c.astype(np.int32), W[r, c].copy()


@functools.lru_cache(maxsize=None)
def dense_blocks(dtname, sizes, stream=310):
    """A block-diagonal matrix of dense seeded blocks (entries uniform in [-1, 1), 2 added to the diagonal) of the given sizes,
    with one seeded coupling entry per row outside the block that the preconditioner must ignore.  -> (indptr, indices, data, block_ptr)."""
    from sprsolve_amd import gen
    dt = np.dtype(dtname)
    n = int(sum(sizes))
    bp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    A = np.zeros((n, n), dt); keep = np.zeros((n, n), bool)
    u = gen.uniform(gen.SEED, n * 32, stream=stream).reshape(n, 32)
    w = gen.uniform(gen.SEED, n * 32, stream=stream + 1).reshape(n, 32)
    for b in range(len(sizes)):
        s, e = int(bp[b]), int(bp[b + 1])
        A[s:e, s:e] = u[s:e, :e - s] + (1j * w[s:e, :e - s] if dt.kind == "c" else 0)
        A[np.arange(s, e), np.arange(s, e)] += 2
        keep[s:e, s:e] = True
    far = (np.arange(n) + n // 2 + 1) % n
    bi = np.searchsorted(bp, np.arange(n), side="right") - 1
    out = (far < bp[bi]) | (far >= bp[bi + 1])
    A[np.arange(n)[out], far[out]] = 0.5; keep[np.arange(n)[out], far[out]] = True
    ip, ix, d = dense_csr(A, keep)
    for a in (ip, ix, d, bp):
        a.setflags(write=False)
    return ip, ix, d, bp


# ------------------------------------------------------------------------------------------------ 1. independent arithmetic
def _wide(a):
    return np.asarray(a).astype(np.complex128 if np.asarray(a).dtype.kind == "c" else np.float64)


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_inverse_against_linalg_inv(dt):
    """max |X - inv(W)| <= 64 eps cond(W) on dense seeded blocks of 1 .. 32 rows, np.linalg.inv in double; the coupling entries
    outside the blocks change nothing."""
    dtname = np.dtype(dt).name
    sizes = (1, 2, 3, 5, 8, 13, 17, 32)
    ip, ix, d, bp = dense_blocks(dtname, sizes)
    inv = br.bjacobi(ip, ix, d, block_ptr=bp)
    assert inv.status == br.OK and len(inv.blocks) == len(sizes)
    A = np.zeros((bp[-1], bp[-1]), d.dtype); A[np.repeat(np.arange(bp[-1]), np.diff(ip)), ix] = d
    worst = 0.0
    for b, X in enumerate(inv.blocks):
        W = _wide(A[bp[b]:bp[b + 1], bp[b]:bp[b + 1]])
        want = np.linalg.inv(W)
        err = np.max(np.abs(_wide(X) - want)) / np.linalg.cond(W)
        worst = max(worst, err)
        assert X.dtype == np.dtype(dt) and X.shape == (sizes[b], sizes[b])
    print("bjacobi inverse %s: worst max|X - inv(W)| / cond(W) = %.2e (64 eps = %.2e)" % (dtname, worst, 64 * eps_of(dt)))
    assert worst <= 64 * eps_of(dt)
    # ... and the apply is that product, folded
    M = br.Applier(inv.block_ptr, inv.blocks)
    v = np.arange(1, bp[-1] + 1).astype(dt)
    want = np.concatenate([_wide(X) @ _wide(v[bp[b]:bp[b + 1]]) for b, X in enumerate(inv.blocks)])
    out = M(v)
    assert out.dtype == np.dtype(dt) and np.max(np.abs(_wide(out) - want)) <= 64 * eps_of(dt) * np.max(np.abs(want))


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_zero_leading_entry_pivots(dt):
    """[[0, 2], [3, 1]] (the (0, 0) entry stored as zero, and not stored at all): regular, the elimination takes row 1 first."""
    W = np.array([[0, 2], [3, 1]], dt)
    want = np.linalg.inv(W.real.astype(np.float64))
    for keep in (None, np.array([[False, True], [True, True]])):
        inv = br.bjacobi(*dense_csr(W, keep), block_size=2)
        assert inv.status == br.OK
        assert np.max(np.abs(_wide(inv.blocks[0]) - want)) <= 8 * eps_of(dt)
    # the permutation [2, 0, 1]: every pivot lies off the diagonal, and the inverse is exact
    Pm = np.zeros((3, 3), dt); Pm[0, 2] = 4; Pm[1, 0] = -2; Pm[2, 1] = 0.5
    inv = br.bjacobi(*dense_csr(Pm, Pm != 0), block_size=3)
    assert inv.status == br.OK and np.array_equal(_wide(inv.blocks[0]), np.linalg.inv(_wide(Pm)))


def test_singular_block_reports_its_first_row():
    ok = np.array([[2.0, 1.0], [1.0, 2.0]])
    sing = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [1.0, 0.0, 1.0]])
    A = np.zeros((9, 9)); A[0:2, 0:2] = ok; A[2:5, 2:5] = sing; A[5:7, 5:7] = ok; A[7:9, 7:9] = 0.0
    bp = np.array([0, 2, 5, 7, 9])
    inv = br.bjacobi(*dense_csr(A), block_ptr=bp)
    assert (inv.status, inv.row, inv.blocks) == (br.INVALID_PRECOND, 2, None)            # the lowest singular block's first row
    A[2:5, 2:5] = np.eye(3)
    assert br.bjacobi(*dense_csr(A), block_ptr=bp)[:2] == (br.INVALID_PRECOND, 7)          # an all-zero block
    A[7:9, 7:9] = [[np.inf, 1.0], [1.0, 1.0]]
    assert br.bjacobi(*dense_csr(A), block_ptr=bp)[:2] == (br.INVALID_PRECOND, 7)          # a pivot that is not finite
    A[7:9, 7:9] = [[np.nan, 1.0], [1.0, 1.0]]
    assert br.bjacobi(*dense_csr(A), block_ptr=bp)[:2] == (br.INVALID_PRECOND, 7)
    # an empty block row (nothing stored inside the block)
    ip, ix, d = dense_csr(np.eye(4), np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]], bool))
    assert br.bjacobi(ip, ix, d, block_size=2)[:2] == (br.INVALID_PRECOND, 0)
    # unsorted columns come first
    ipb = np.array([0, 2, 4], np.int32)
    assert br.bjacobi(ipb, np.array([1, 0, 0, 1], np.int32), np.zeros(4), block_size=2)[:2] == (br.INVALID_ARGUMENT, 0)


@pytest.mark.parametrize("dt", [F64, C32], ids=_ids)
def test_reducible_block_keeps_its_zeros(dt):
    """A block that is itself block diagonal (two uncoupled 2 x 2 parts) and one that is triangular: the structural zeros of the
    inverse are zeros (of either sign: the loops run over them and their signs are part of the bits), the rest is the inverse."""
    W = np.zeros((4, 4), dt); W[0:2, 0:2] = [[4, -1], [-1, 4]]; W[2:4, 2:4] = [[-3, 1], [2, 5]]
    inv = br.bjacobi(*dense_csr(W, W != 0), block_size=4)
    X = inv.blocks[0]
    assert inv.status == br.OK and np.all(X[0:2, 2:4] == 0) and np.all(X[2:4, 0:2] == 0)
    assert np.max(np.abs(_wide(X) - np.linalg.inv(_wide(W)))) <= 8 * eps_of(dt)
    T =np.triu(np.arange(1, 17).reshape(4, 4)).astype(dt)
    X = br.bjacobi(*dense_csr(T, T != 0), block_size=4).blocks[0]
    assert np.all(np.tril(X, -1) == 0) and np.max(np.abs(_wide(X) - np.linalg.inv(_wide(T)))) <= 16 * eps_of(dt)


# ------------------------------------------------------------------------------------------------ 2. the generator
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_coupled_grid_properties(dt):
    from sprsolve_amd import gen
    rows, cols, bs = 5, 4, 3
    ip, ix, d, rhs = gen.coupled_grid(rows, cols, bs, dtype=dt)
    n = rows * cols * bs
    assert ip.dtype == ix.dtype == np.int32 and d.dtype == rhs.dtype == np.dtype(dt) and ip.size == n + 1 and rhs.size == n
    assert all(np.all(np.diff(ix[ip[i]:ip[i + 1]]) > 0) for i in range(n))                # sorted, no duplicates
    A = np.zeros((n, n), dt); A[np.repeat(np.arange(n), np.diff(ip)), ix] = d
    assert np.array_equal(A, A.conj().T) and np.all(A.diagonal().imag == 0)                # Hermitian, a real diagonal
    ev = np.linalg.eigvalsh(_wide(A))
    assert ev[0] > 0                                                                       # positive definite
    # the pattern is the 5-point graph of the nodes, dense in the node blocks
    node = np.arange(n) // bs
    P = (A != 0)
    i, j = node // cols, node % cols
    near = (np.abs(i[:, None] - i[None, :]) + np.abs(j[:, None] - j[None, :])) <= 1
    assert np.array_equal(P, near)
    # an off-diagonal node block is -C, the same everywhere; C has the spectrum 1 .. spread
    Cm = -_wide(A[0:bs, bs:2 * bs])
    assert np.array_equal(A[bs:2 * bs, 2 * bs:3 * bs], A[0:bs, bs:2 * bs])
    cev = np.linalg.eigvalsh(Cm)
    assert np.allclose(cev, 1e3 ** (np.arange(bs) / (bs - 1)), rtol=1e-4 if is_single(dt) else 1e-10)
    # a diagonal node block is 4 C + e e^H: the difference has rank one and is positive semi-definite
    D = _wide(A[0:bs, 0:bs]) - 4 * Cm
    dev = np.linalg.eigvalsh(D)
    assert dev[-1] > 0 and np.all(np.abs(dev[:-1]) <= (1e-2 if is_single(dt) else 1e-10))
    if np.dtype(dt).kind == "c":
        assert np.any(d.imag != 0)
    # seeded: the same again, and other streams give another matrix
    assert np.array_equal(gen.coupled_grid(rows, cols, bs, dtype=dt)[2], d)
    assert not np.array_equal(gen.coupled_grid(rows, cols, bs, dtype=dt, stream=400)[2], d)
    assert gen.coupled_grid(3, 3, 1)[0].size == 10                                         # bs = 1 is a scalar grid


# ------------------------------------------------------------------------------------------------ 3. iteration counts
@pytest.mark.parametrize("name,dt,solver", CASES, ids=_ids)
def test_counts(name, dt, solver):
    dtname = np.dtype(dt).name
    want_j, want_b = BJ_COUNTS[name][dtname][solver]
    oj, ob = checker_run(solver, name, dtname, "jacobi"), checker_run(solver, name, dtname)
    print("%s %s %s: Jacobi %d, block-Jacobi %d iterations" % (solver, name, dtname, oj.its, ob.its))
    assert [(o.status, o.its) for o in (oj, ob)] == [(ref.OK, want_j), (ref.OK, want_b)]


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_block_jacobi_halves_the_cg_count_on_the_coupled_grid(dt):
    dtname = np.dtype(dt).name
    oj, ob = checker_run("cg", "cgrid", dtname, "jacobi"), checker_run("cg", "cgrid", dtname)
    assert oj.status == ob.status == ref.OK and 2 * ob.its <= oj.its, (oj.its, ob.its)


@pytest.mark.parametrize("solver", ["gmres", "bicgstab"])
@pytest.mark.parametrize("dt", REAL, ids=_ids)
def test_line_blocks_halve_the_count_on_convection_diffusion(dt, solver):
    dtname = np.dtype(dt).name
    oj, ob = checker_run(solver, "cdline", dtname, "jacobi"), checker_run(solver, "cdline", dtname)
    assert oj.status == ob.status == ref.OK and 2 * ob.its <= oj.its, (oj.its, ob.its)


@pytest.mark.parametrize("dt", REAL, ids=_ids)
def test_minres_true_residual_of_the_checker(dt):
    """The checker's own MINRES run reports res <= tol and leaves a true residual above 10 tol in f64 (1.3e-9 at tol 1e-10): the
    estimate lives in the M-norm.  It stays below tol sqrt(cond(M)), and it moves by less than a tenth with the order of the sums:
    what minres_true_bound's factor of two rests on."""
    dtname = np.dtype(dt).name
    o = checker_run("minres", "cgrid", dtname)
    bound, (t_np, t_pw) = minres_true_bound("cgrid", dtname)
    ev = np.concatenate([np.linalg.eigvalsh(_herm(X)) for X in inverse_of("cgrid", dtname).blocks])
    root_cond = float(np.sqrt(ev.max() / ev.min()))
    print("minres cgrid %s: reported %.3e, true %.3e (pairwise sums %.3e), tol %g, sqrt(cond(M)) %.1f, GPU bound %.3e"
          % (dtname, o.res, t_np, t_pw, tol_of(dt), root_cond, bound))
    assert o.res <= tol_of(dt) and ev.min() > 0 and max(t_np, t_pw) <= tol_of(dt) * root_cond
    assert abs(t_np - t_pw) <= 0.1 * min(t_np, t_pw)
    assert bound <= 30 * tol_of(dt)


@pytest.mark.parametrize("solver", ["cg", "bicgstab", "minres", "gmres"])
def test_trace_prefix_of_the_gpu_cases(solver):
    """Every GPU case keeps at least one comparable row; CG in f64 / c64 keeps its whole run (the full comparison of
    tests/test_gpu_ilu.py applies there), and the checker's x and step count do not move with the order of its sums."""
    for name, dt, s in CASES:
        if s == solver:
            dtname = np.dtype(dt).name
            k = trace_prefix(solver, name, dtname)
            a, b = checker_run(solver, name, dtname), checker_run(solver, name, dtname, "bjacobi", "pairwise")
            whole = whole_run_is_comparable(solver, name, dtname)
            print("prefix %s %s %s: %d of %d, whole run %s, its %d / %d, max|dx| %.2e" % (solver, name, dtname, k, len(a.trace), whole, a.its, b.its,
                                                                                        np.max(np.abs(a.x - b.x))))
            assert k >= 1
            if solver in ("cg", "gmres"):
                assert a.its == b.its
                if not is_single(dt):
                    assert np.max(np.abs(a.x - b.x)) <= 1e-8 * max(1.0, np.max(np.abs(a.x)))       # a tenth of the GPU test's 1e-7
            if solver == "cg" and not is_single(dt):
                assert whole


def test_cg_with_numpy_sums_is_the_project_checker():
    """tests/_bjacobi_ref.py's cg with sums="numpy" is tests/_ilu_ref.py's cg bit for bit."""
    ip, ix, d, rhs = system("cgrid", "complex128")
    M = applier("cgrid", "complex128")
    a = ref.cg(ip, ix, d, rhs, np.zeros(rhs.size, C64), 200, 1e-10, prec=M)
    b = br.cg(ip, ix, d, rhs, np.zeros(rhs.size, C64), 200, 1e-10, prec=M)
    assert (a.status, a.its, a.res) == (b.status, b.its, b.res) and np.array_equal(bits(a.x), bits(b.x)) and a.trace == b.trace


# ------------------------------------------------------------------------------------------------ 4. the library without a GPU
def test_null_handles():
    """What sprs_bjacobi_* answers before any HIP call."""
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    h = C.c_void_p(1); row = C.c_int64(-7)
    assert L.sprs_bjacobi_create(None, 3, None, 0, C.byref(h), C.byref(row)) == _lib.INVALID_ARGUMENT
    assert L.sprs_bjacobi_create(None, 3, None, 0, None, None) == _lib.INVALID_ARGUMENT
    assert L.sprs_bjacobi_destroy(None) == _lib.OK
    assert L.sprs_bjacobi_info(None, None, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.sprs_bjacobi_block_ptr(None, None) == _lib.INVALID_ARGUMENT
    for s in "dzsc":
        assert getattr(L, "sprs_bjacobi_mul_vec_dev_" + s)(None, None, None) == _lib.INVALID_ARGUMENT
        assert getattr(L, "sprs_bjacobi_mul_vec_" + s)(None, None, 0, None, 0) == _lib.INVALID_ARGUMENT
        assert getattr(L, "sprs_bjacobi_inverse_" + s)(None, None, 0) == _lib.INVALID_ARGUMENT
    import sprsolve_amd
    assert sprsolve_amd.BlockJacobi is sprsolve_amd.bjacobi.BlockJacobi
    from sprsolve_amd._solver import applied_prefix
    assert applied_prefix(sprsolve_amd.BlockJacobi(None, None, np.float64, 0)) == "bjacobi"
