"""Block-Jacobi on the GPU (sprs_bjacobi_*, csrc/bjacobi.hip) against the loops of tests/_bjacobi_ref.py: the inverse blocks BIT FOR
BIT in all four scalar types (every size bin, ragged last blocks, mixed sizes inside one workgroup, many workgroups, pivoting,
zero signs), the application against the checker's fold on every entry point, the creation errors, and the solvers preconditioned
by it — CG, GMRES, BiCGStab and MINRES in literal mode against the project's checkers fed with the checker's apply and fused mode
against literal mode, with the comparisons and tolerances of tests/test_gpu_ilu.py and tests/test_gpu_krylov_prec.py (imported, none
invented).  IDR(s) and LOBPCG do not take the handle: their mirrors refuse it.

The checkers' counts (tests/test_bjacobi_cpu.py: BJ_COUNTS) stand behind every max_iter, each at least twice its count."""
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
from _special import assert_same_special  # noqa: E402
from test_bjacobi_cpu import (ALL, BJ_COUNTS, C32, C64, F32, F64, GMRES_RESTART, REAL, SYSTEMS, applier, bits, block_size_of, checker_run,  # noqa: E402,F401
                              dense_csr, gmres_trace_array, inverse_of, is_single, max_iter_of, minres_true_bound, system, tol_of, trace_prefix, whole_run_is_comparable)
from test_gmres_cpu import trace_close as gm_trace_close  # noqa: E402
from test_gpu_ilu import _cg_trace_array, _cg_trace_close, _margin, _run, _true_res  # noqa: E402
from test_krylov_prec_cpu import gpu_tols  # noqa: E402

pytestmark = pytest.mark.gpu

_ids = lambda v: v if isinstance(v, str) else (np.dtype(v).name if isinstance(v, type) else str(v))
UNIFORM_BS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32)
BAND_N = 131                                                  # prime: no block size but 1 divides it, so the last block is ragged
CYCLE = np.concatenate([[0], np.cumsum(np.arange(1, 33))]).astype(np.int64)     # blocks of 1, 2, .., 32 rows: 528 rows


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


@pytest.fixture(autouse=True)
def _restore_grid(sa):
    ctx = sa.default_ctx(0)
    grid = ctx.get("grid")
    yield
    ctx.set("grid", grid)


@functools.lru_cache(maxsize=None)
def band(n, dtname):
    """A seeded non-symmetric band matrix, half bandwidth 33 (every block of up to 32 rows is full but for the entries left out:
    about one in six off the diagonal is not stored), entries uniform in [-1, 1) and 3 added to the diagonal."""
    from sprsolve_amd import gen
    dt = np.dtype(dtname)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    A = gen.uniform(gen.SEED, n * n, stream=320).reshape(n, n) + (1j * gen.uniform(gen.SEED, n * n, stream=321).reshape(n, n) if dt.kind == "c" else 0)
    A = A + 3 * np.eye(n)
    keep = (np.abs(i - j) <= 33) & ((np.abs(gen.uniform(gen.SEED, n * n, stream=322).reshape(n, n)) > 1 / 6) | (i == j))
    ip, ix, d = dense_csr(A.astype(dt), keep)
    for a in (ip, ix, d):
        a.setflags(write=False)
    return ip, ix, d


@functools.lru_cache(maxsize=None)
def band_inverse(n, dtname, bs):
    """The checker's inverse of band(n): uniform blocks of bs rows, or bs = 0: the blocks of CYCLE."""
    ip, ix, d = band(n, dtname)
    inv = br.bjacobi(ip, ix, d, block_size=bs) if bs else br.bjacobi(ip, ix, d, block_ptr=CYCLE)
    assert inv.status == br.OK
    return inv


def _csr(sa, ip, ix, d, shape=None):
    n = ip.size - 1
    return sa.HipCsr.new(shape or (n, n), ip, ix, d)


def _same_inverse(P, inv):
    assert np.array_equal(P.block_ptr, inv.block_ptr), "block_ptr"
    got = P.inverse()
    assert len(got) == len(inv.blocks)
    for b, (g, w) in enumerate(zip(got, inv.blocks)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(bits(g), bits(w)), "block %d (rows from %d)" % (b, inv.block_ptr[b])
    info = P.info
    m = np.diff(inv.block_ptr)
    assert (info["n"], info["nblocks"], info["max_block"]) == (int(inv.block_ptr[-1]), m.size, int(m.max()))
    assert info["slots"] % 64 == 0 and info["slots"] >= int(np.sum(m * m))


# ------------------------------------------------------------------------------------------------ 1. the inverse, bit for bit
@pytest.mark.parametrize("bs", UNIFORM_BS)
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_uniform_blocks_have_the_bits_of_the_checker(sa, dt, bs):
    dtname = np.dtype(dt).name
    P = sa.BlockJacobi.new(_csr(sa, *band(BAND_N, dtname)), block_size=bs)
    inv = band_inverse(BAND_N, dtname, bs)
    assert bs == 1 or inv.block_ptr[-1] - inv.block_ptr[-2] == BAND_N % bs
    _same_inverse(P, inv)


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_block_sizes_cycling_1_to_32(sa, dt):
    """Every bin, and blocks of different sizes in the groups of one workgroup."""
    dtname = np.dtype(dt).name
    P = sa.BlockJacobi.new(_csr(sa, *band(528, dtname)), block_ptr=CYCLE)
    _same_inverse(P, band_inverse(528, dtname, 0))
    assert P.info["max_block"] == 32 and P.info["nblocks"] == 32


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_coupled_grid_over_many_workgroups(sa, dt):
    """gen.coupled_grid(40, 33, 3): 3960 rows, 1320 blocks of 3 (21 to a slice: 63 slices, 21 workgroups of the smallest bin)."""
    dtname = np.dtype(dt).name
    ip, ix, d, rhs = system("cgrid40", dtname)
    P = sa.BlockJacobi.new(_csr(sa, ip, ix, d), block_size=3)
    _same_inverse(P, inverse_of("cgrid40", dtname))
    assert P.info["slots"] == 63 * 3 * 64


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_pivoting_and_reducible_blocks(sa, dt):
    """Blocks whose (0, 0) entry is not stored, a permutation (every pivot off the diagonal), a block-diagonal block and a triangular
    one: the zeros of the inverse carry the checker's signs."""
    W = np.zeros((13, 13), dt)
    W[0:2, 0:2] = [[0, 2], [3, 1]]
    W[2, 4] = 4; W[3, 2] = -2; W[4, 3] = 0.5
    W[5:7, 5:7] = [[4, -1], [-1, 4]]; W[7:9, 7:9] = [[-3, 1], [2, 5]]
    W[9:13, 9:13] = -np.triu(np.arange(1, 17).reshape(4, 4))
    bp = np.array([0, 2, 5, 9, 13])
    ip, ix, d = dense_csr(W, W != 0)
    inv = br.bjacobi(ip, ix, d, block_ptr=bp)
    assert inv.status == br.OK
    P = sa.BlockJacobi.new(_csr(sa, ip, ix, d), block_ptr=bp)
    _same_inverse(P, inv)
    got = P.inverse()
    assert np.array_equal(got[1], np.linalg.inv(W[2:5, 2:5]))                              # exact: powers of two
    assert np.all(got[2][0:2, 2:4] == 0) and np.all(got[2][2:4, 0:2] == 0) and np.all(np.tril(got[3], -1) == 0)


# ------------------------------------------------------------------------------------------------ 2. application
def _raw_apply(sa, P, dt, in_ptr, out_ptr):
    from sprsolve_amd import _lib
    from sprsolve_amd.device import sfx
    assert getattr(_lib.lib(), "sprs_bjacobi_mul_vec_dev_" + sfx(np.dtype(dt)))(P.h, in_ptr, out_ptr) == _lib.OK
    sa.default_ctx(0).sync()


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_application_has_the_bits_of_the_fold(sa, dt):
    from sprsolve_amd import gen
    dtname = np.dtype(dt).name
    A = _csr(sa, *band(528, dtname))
    P = sa.BlockJacobi.new(A, block_ptr=CYCLE)
    inv = band_inverse(528, dtname, 0)
    M = br.Applier(inv.block_ptr, inv.blocks)
    n = 528
    v = (gen.uniform(gen.SEED, n, stream=330) + (1j * gen.uniform(gen.SEED, n, stream=331) if np.dtype(dt).kind == "c" else 0)).astype(dt)
    want = M(v)
    out = np.zeros(n, dt)
    P.mul_vec(v, out)                                                            # host entry point
    assert np.array_equal(bits(out), bits(want)), "host"
    d_in = sa.DevVec.from_numpy(v); d_out = sa.DevVec.from_numpy(np.zeros(n, dt))
    P.mul_vec(d_in, d_out)                                                       # device entry point
    assert np.array_equal(bits(d_out.to_numpy()), bits(want)), "device"
    # device views that start one element into their allocations: aligned to the element and no further
    pad_in = sa.DevVec.from_numpy(np.concatenate([np.zeros(1, dt), v])); pad_out = sa.DevVec.from_numpy(np.full(n + 2, 7, dt))
    item = np.dtype(dt).itemsize
    _raw_apply(sa, P, dt, C.c_void_p(pad_in.ptr.value + item), C.c_void_p(pad_out.ptr.value + item))
    got = pad_out.to_numpy()
    assert np.array_equal(bits(got[1:n + 1]), bits(want)) and got[0] == 7 and got[n + 1] == 7, "unaligned views"
    P.mul_vec(d_in, d_in)                                                        # in is out
    assert np.array_equal(bits(d_in.to_numpy()), bits(want)), "in place"
    A.close()                                                                    # the handle borrows nothing from A
    out2 = np.zeros(n, dt)
    P.mul_vec(v, out2)
    assert np.array_equal(bits(out2), bits(want)), "after A.close()"
    # NaN, +-inf and -0 in `in`: they spread over their own blocks and no further, and padded slots are never multiplied
    sp = v.copy()
    sp[0] = np.nan; sp[7] = np.inf; sp[40] = -np.inf; sp[100] = -0.0; sp[527] = np.nan
    sp[200:210] = -0.0                                                           # a run of -0 inside one block
    want_sp = M(sp)
    out3 = np.zeros(n, dt)
    P.mul_vec(sp, out3)
    assert_same_special(out3, want_sp, "special values")
    clean = np.ones(n, bool)
    for r in (0, 7, 40, 527):
        b = np.searchsorted(CYCLE, r, side="right") - 1
        clean[CYCLE[b]:CYCLE[b + 1]] = False
    assert np.all(np.isfinite(out3[clean])) and not np.all(np.isfinite(out3[~clean]))
    with pytest.raises(sa.error.DimensionMismatch):
        P.mul_vec(v[:-1], np.zeros(n - 1, dt))
    with pytest.raises(NotImplementedError):
        P.mul_vec_dot(v, out)


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_application_with_a_small_grid_walks_several_slices(sa, dt):
    """63 slices on the smallest grid the knob allows (8 workgroups, 32 wavefronts): every wavefront but one walks two slices."""
    dtname = np.dtype(dt).name
    ip, ix, d, rhs = system("cgrid40", dtname)
    n = rhs.size
    P = sa.BlockJacobi.new(_csr(sa, ip, ix, d), block_size=3)
    want = applier("cgrid40", dtname)(rhs)
    ctx = sa.default_ctx(0)
    d_in = sa.DevVec.from_numpy(rhs); d_out = sa.DevVec.from_numpy(np.zeros(n, dt))
    P.mul_vec(d_in, d_out)
    assert np.array_equal(bits(d_out.to_numpy()), bits(want)), "default grid"
    ctx.set("grid", 8)
    assert ctx.get("grid") == 8
    d_out2 = sa.DevVec.from_numpy(np.zeros(n, dt))
    P.mul_vec(d_in, d_out2)
    assert np.array_equal(bits(d_out2.to_numpy()), bits(want)), "grid 8"
    P.mul_vec(d_in, d_in)
    assert np.array_equal(bits(d_in.to_numpy()), bits(want)), "grid 8, in place"


# ------------------------------------------------------------------------------------------------ 3. errors and the handle's life
def test_creation_errors(sa):
    from sprsolve_amd import _lib
    E = sa.error
    L = _lib.lib()
    ip, ix, d = band(BAND_N, "float64")
    A = _csr(sa, ip, ix, d)
    p64 = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(bs, bp, text):
        h = C.c_void_p(1); row = C.c_int64(-7)
        arr = None if bp is None else np.asarray(bp, np.int64)
        st = L.sprs_bjacobi_create(A.h, bs, None if arr is None else p64(arr), 0 if arr is None else arr.size - 1, C.byref(h), C.byref(row))
        assert st == _lib.INVALID_ARGUMENT and not h.value and row.value == -1, (bs, bp, st)
        assert text in L.sprs_last_error(A.ctx.h).decode(), L.sprs_last_error(A.ctx.h)

    refused(0, None, "exactly one of")                                            # neither
    refused(-3, None, "exactly one of")
    refused(4, [0, BAND_N], "exactly one of")                                     # both
    refused(33, None, "more than SPRS_BJACOBI_MAX_BLOCK")
    refused(0, [0, 20, 53, 60, 90, 120, BAND_N], "block 1 has more than")         # a block of 33
    refused(0, [1, 20, BAND_N], "must start at 0")
    refused(0, [0, 20, 20, 40, 70, 100, BAND_N], "does not increase strictly at block 1")
    refused(0, [0, 30, 20, 40, 70, 100, BAND_N], "does not increase strictly at block 1")
    refused(0, [0, 30, 60, 90, 120], "must end at the 131 rows")
    with pytest.raises(ValueError, match="exactly one of"):
        sa.BlockJacobi.new(A)
    with pytest.raises(ValueError, match="exactly one of"):
        sa.BlockJacobi.new(A, block_size=4, block_ptr=[0, BAND_N])
    with pytest.raises(ValueError, match="block_size must be positive"):
        sa.BlockJacobi.new(A, block_size=0)
    with pytest.raises(ValueError, match="more than SPRS_BJACOBI_MAX_BLOCK"):
        sa.BlockJacobi.new(A, block_size=33)
    ipb = np.array([0, 2, 4], np.int32); ixb = np.array([0, 1, 0, 1], np.int32)
    with pytest.raises(E.IncompatibleMatrixFormat, match="Not a square"):
        sa.BlockJacobi.new(sa.HipCsr.new((2, 3), ipb, ixb, np.ones(4)), block_size=2)
    for bad in (np.array([1, 0, 0, 1], np.int32), np.array([0, 1, 1, 1], np.int32)):   # unsorted; duplicate
        with pytest.raises(ValueError, match="strictly ascending"):
            sa.BlockJacobi.new(sa.HipCsr.new((2, 2), ipb, bad, np.ones(4)), block_size=2)
    # a malformed block_ptr is refused before the pattern is looked at
    h = C.c_void_p(1)
    bp_bad = np.array([0, 1, 1, 2], np.int64)
    Abad = sa.HipCsr.new((2, 2), ipb, np.array([1, 0, 0, 1], np.int32), np.ones(4))
    assert L.sprs_bjacobi_create(Abad.h, 0, p64(bp_bad), 3, C.byref(h), None) == _lib.INVALID_ARGUMENT and not h.value
    assert "does not increase strictly" in L.sprs_last_error(Abad.ctx.h).decode()
    # singular blocks: the lowest one's first row, and no handle
    ok = np.array([[2.0, 1.0], [1.0, 2.0]])
    W = np.zeros((9, 9)); W[0:2, 0:2] = ok; W[2:5, 2:5] = [[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [1.0, 0.0, 1.0]]; W[5:7, 5:7] = ok
    bp = np.array([0, 2, 5, 7, 9], np.int64)
    As = _csr(sa, *dense_csr(W))
    assert br.bjacobi(*dense_csr(W), block_ptr=bp)[:2] == (br.INVALID_PRECOND, 2)
    h = C.c_void_p(1); row = C.c_int64(-7)
    assert L.sprs_bjacobi_create(As.h, 0, p64(bp), 4, C.byref(h), C.byref(row)) == _lib.INVALID_PRECOND
    assert row.value == 2 and not h.value
    with pytest.raises(E.InvalidPreconditioner, match="rows 2 .. 4 is singular"):
        sa.BlockJacobi.new(As, block_ptr=bp)
    W[2:5, 2:5] = np.eye(3)
    with pytest.raises(E.InvalidPreconditioner, match="rows 7 .. 8 is singular"):          # an all-zero block
        sa.BlockJacobi.new(_csr(sa, *dense_csr(W)), block_ptr=bp)
    for corner in (np.inf, np.nan):                                                        # a pivot that is not finite
        W[7:9, 7:9] = [[corner, 1.0], [1.0, 1.0]]
        with pytest.raises(E.InvalidPreconditioner, match="rows 7 .. 8 is singular"):
            sa.BlockJacobi.new(_csr(sa, *dense_csr(W)), block_ptr=bp)
    W[7:9, 7:9] = ok
    with pytest.raises(E.InvalidPreconditioner, match="rows 8 .. 8 is singular"):          # uniform blocks: the ragged last one
        W2 = W.copy(); W2[8, :] = 0; W2[:, 8] = 0
        sa.BlockJacobi.new(_csr(sa, *dense_csr(W2, W2 != 0)), block_size=4)
    assert L.sprs_bjacobi_destroy(None) == 0


def test_distributed_operator_is_refused(sa):
    """tests/test_gpu_fsai.py::test_distributed_operator_is_refused for block-Jacobi."""
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
            sa.BlockJacobi.new(A, block_size=4)
        # ... and a single-GPU handle is refused by a solver on the distributed operator
        P = sa.BlockJacobi.new(sa.HipCsr.new((n, n), ip, ix, d), block_size=4)
        with pytest.raises(ValueError):
            sa.CG.new(A, n).precond_solve(P, torch.from_numpy(rhs).to(dev), torch.zeros(n, dtype=torch.float64, device=dev), 10, 1e-10)
    finally:
        comm.close()


def test_lifecycle(sa):
    """A closed before the solve, close twice, and the statuses of applied_check through a solver."""
    ip, ix, d, rhs = system("cgrid", "float64")
    n = rhs.size
    A = _csr(sa, ip, ix, d)
    P = sa.BlockJacobi.new(A, block_size=3)
    A.close()
    A2 = _csr(sa, ip, ix, d)
    x = np.zeros(n)
    its, res = sa.CG.new(A2, n).precond_solve(P, rhs, x, max_iter_of("cg", "cgrid", "float64"), 1e-10)
    assert res <= 1e-10 and _true_res(ip, ix, d, rhs, x) <= 1e-9 and abs(its - BJ_COUNTS["cgrid"]["float64"]["cg"][1]) <= _margin(its)
    P32 = sa.BlockJacobi.new(_csr(sa, ip, ix, d.astype(F32)), block_size=3)
    cd = system("cdline", "float64")
    Psmall = sa.BlockJacobi.new(_csr(sa, *cd[:3]), block_size=16)
    for mk in (lambda: sa.CG.new(A2, n), lambda: sa.GMRES.new(A2, n, 5), lambda: sa.BiCGStab.new(A2, n), lambda: sa.MinRes.new(A2, n)):
        x = np.zeros(n)
        with pytest.raises(ValueError):
            mk().precond_solve(P32, rhs, x, 10, 1e-10)                            # another scalar type
        with pytest.raises(sa.error.DimensionMismatch):
            mk().precond_solve(Psmall, rhs, x, 10, 1e-10)                         # another size
        assert not np.any(x)
    P.close(); P.close()
    assert P.h is None
    P32.close(); Psmall.close()


# ------------------------------------------------------------------------------------------------ 4. solves
def _handles(sa, name, dt):
    ip, ix, d, rhs = system(name, np.dtype(dt).name)
    A = _csr(sa, ip, ix, d)
    return ip, ix, d, rhs, A, sa.BlockJacobi.new(A, block_size=block_size_of(name))


def _jacobi(sa, ip, ix, d, dt):
    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    return sa.DiagPrecond.new(d[rows == ix].real.astype(np.float32 if is_single(dt) else np.float64).copy(), t_dtype=d.dtype)


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_cg_literal_follows_the_checker_and_fused_follows_literal(sa, dt):
    """tests/test_gpu_fsai.py::test_cg_literal_follows_the_checker_and_fused_follows_literal (tests/test_gpu_ilu.py's) with M =
    block-Jacobi on gen.coupled_grid(12, 11, 3), comparison for comparison.  tests/test_bjacobi_cpu.py shows that in f64 / c64 the
    checker holds a tenth of these tolerances against itself over the whole run of 67 steps, so nothing is cut to a prefix."""
    name, dtname = "cgrid", np.dtype(dt).name
    ip, ix, d, rhs, A, P = _handles(sa, name, dt)
    n = rhs.size
    tol = tol_of(dt)
    max_iter = max_iter_of("cg", name, dtname)
    o = checker_run("cg", name, dtname)
    assert o.status == ref.OK and 2 * o.its <= max_iter and (is_single(dt) or whole_run_is_comparable("cg", name, dtname))
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
    print("cg+bjacobi %s %s: literal its %s (checker %d) res %s (checker %.3e) max|x - checker| %.3e; fused its %s res %s true %.3e max|dx| %.3e"
          % (name, dtname, il, o.its, rl, o.res, err, itf, rf, true_res, np.max(np.abs(xf - xl))))
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
    # the Jacobi path beside it is untouched, and needs more iterations
    xj = np.zeros(n, dt)
    stj, itj, _ = _run(sa, s, _jacobi(sa, ip, ix, d, dt), rhs, xj, max_iter_of("cg", name, dtname, "jacobi"), tol)
    assert stj == ref.OK and itj > itf


KRYLOV_CASES = [(solver, name, dt) for name, (_, dts, solvers) in SYSTEMS.items() for dt in dts for solver in solvers
                if solver in ("bicgstab", "minres") and not (solver == "minres" and np.dtype(dt).kind == "c")]


@pytest.mark.parametrize("solver,name,dt", KRYLOV_CASES, ids=_ids)
def test_bicgstab_and_minres_follow_the_checker(sa, solver, name, dt):
    """tests/test_gpu_krylov_prec.py::_follows with M = block-Jacobi (MINRES: the real types only, and its true residual held to
    tests/test_bjacobi_cpu.py::minres_true_bound: 10 tol, or twice the checker's own true residual where that is more)."""
    dtname = np.dtype(dt).name
    cls = {"bicgstab": sa.BiCGStab, "minres": sa.MinRes}[solver]
    ip, ix, d, rhs, A, P = _handles(sa, name, dt)
    n = rhs.size
    tol = tol_of(dt)
    max_iter = max_iter_of(solver, name, dtname)
    o = checker_run(solver, name, dtname)
    prefix = trace_prefix(solver, name, dtname)
    assert o.status == kp.OK and 2 * o.its <= max_iter and prefix >= 1
    out = {}
    for mode in ("literal", "fused"):
        s = cls.new(A, n); s.set_mode(mode); s.set_trace(max_iter + 1)
        x = np.zeros(n, dt)
        st, its, res = _run(sa, s, P, rhs, x, max_iter, tol)
        out[mode] = (st, its, res, x, s.trace(), _true_res(ip, ix, d, rhs, x))
    (sl, il, rl, xl, tl, true_l), (sf, itf, rf, xf, tf, true_f) = out["literal"], out["fused"]
    print("%s+bjacobi %s %s: literal its %s (checker %d) res %s (checker %.3e) true %.3e rows %d; fused its %s res %s true %.3e rows %d; prefix %d"
          % (solver, name, dtname, il, o.its, rl, o.res, true_l, len(tl), itf, rf, true_f, len(tf), prefix))
    rtol, atol = gpu_tols(dt)
    true_max = minres_true_bound(name, dtname)[0] if solver == "minres" else 10 * tol
    # literal against the checker
    assert sl == kp.OK and abs(il - o.its) <= _margin(o.its)
    k = min(prefix, len(tl), len(o.trace))
    assert k >= 1 and _cg_trace_close(tl[:k], o.trace[:k], rtol=rtol, atol=atol)
    assert rl <= tol and true_l <= true_max
    # fused against literal
    assert sf == kp.OK and abs(itf - il) <= _margin(il)
    k = min(prefix, len(tf), len(tl))
    assert k >= 1 and _cg_trace_close(tf[:k], tl[:k], rtol=rtol, atol=atol)
    assert rf <= tol and true_f <= true_max
    # without a trace buffer (lazy polling) and on device vectors the fused solve returns the same bits
    s = cls.new(A, n)
    x2 = np.zeros(n, dt)
    assert _run(sa, s, P, rhs, x2, max_iter, tol)[:2] == (sf, itf) and np.array_equal(x2, xf)
    d_rhs = sa.DevVec.from_numpy(rhs); d_x = sa.DevVec.from_numpy(np.zeros(n, dt))
    assert _run(sa, s, P, d_rhs, d_x, max_iter, tol)[:2] == (sf, itf) and np.array_equal(d_x.to_numpy(), xf)


GMRES_CASES = [(name, dt) for name, (_, dts, solvers) in SYSTEMS.items() for dt in dts if "gmres" in solvers]


@pytest.mark.parametrize("name,dt", GMRES_CASES, ids=_ids)
def test_gmres_literal_follows_the_checker_and_fused_follows_literal(sa, name, dt):
    """tests/test_gpu_fsai.py::test_gmres_literal_follows_the_checker_and_fused_follows_literal (tests/test_gpu_ilu.py's) with M =
    block-Jacobi, comparison for comparison, the trace rows over the prefix that tests/test_bjacobi_cpu.py derives by the rule of
    GMRES_TRACE_ROWS.  One comparison depends on that prefix: the reported residual itself is demanded at 1e-9 only where the
    prefix is the whole run (whole_run_is_comparable).  It is not in these runs of 43 to 106 steps — the checker's own last
    residual moves by 6e-8 to 1e-5 with the order of its sums — so there the residual is compared through the trace rows of the
    prefix and bounded by tol at the end.  Step counts and x are held as in the original."""
    dtname = np.dtype(dt).name
    ip, ix, d, rhs, A, P = _handles(sa, name, dt)
    n = rhs.size
    tol = tol_of(dt)
    m = GMRES_RESTART
    max_iter = max_iter_of("gmres", name, dtname)
    o = checker_run("gmres", name, dtname)
    rows = trace_prefix("gmres", name, dtname)
    whole = whole_run_is_comparable("gmres", name, dtname)
    assert o.status == ref.OK and 2 * o.its <= max_iter and rows >= 1
    out = {}
    for mode in ("literal", "fused"):
        s = sa.GMRES.new(A, n, m); s.set_mode(mode); s.set_trace(max_iter)
        x = np.zeros(n, dt)
        st, its, res = _run(sa, s, P, rhs, x, max_iter, tol)
        out[mode] = (st, its, res, x, s.trace(), _true_res(ip, ix, d, rhs, x))
    (sl, il, rl, xl, tl, true_l), (sf, itf, rf, xf, tf, true_f) = out["literal"], out["fused"]
    want = gmres_trace_array(o.trace)
    err = np.max(np.abs(xl - o.x))
    print("gmres+bjacobi %s %s: literal its %s (checker %d) res %s (checker %.3e) true %.3e max|x - checker| %.3e; fused its %s res %s true %.3e max|dx| %.3e; rows %d, whole %s"
          % (name, dtname, il, o.its, rl, o.res, true_l, err, itf, rf, true_f, np.max(np.abs(xf - xl)), rows, whole))
    # literal against the checker
    assert sl == o.status == ref.OK
    assert abs(il - o.its) <= _margin(o.its)
    assert tl.shape == (il, 8) and np.array_equal(tl[:, 0], np.arange(1, il + 1))
    assert rl <= tol and true_l <= 10 * tol
    k = min(rows, il, o.its)
    if is_single(dt):
        assert gm_trace_close(tl[:1], want[:1], rtol=1e-5, atol=1e-8)
        assert err < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
    else:
        assert gm_trace_close(tl[:k], want[:k], rtol=1e-9, atol=1e-12)
        assert err <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
        assert il == o.its and (not whole or np.isclose(rl, o.res, rtol=1e-9, atol=1e-12))
    # fused against literal
    assert sf == sl == ref.OK
    assert abs(itf - il) <= _margin(il)
    assert rf <= tol and true_f <= 10 * tol
    assert tf.shape == (itf, 8) and np.array_equal(tf[:, 0], np.arange(1, itf + 1))
    k = min(rows, itf, il)
    if is_single(dt):
        assert np.max(np.abs(xf - xl)) < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
        assert gm_trace_close(tf[:1], tl[:1], rtol=1e-5, atol=1e-8)
    else:
        assert np.max(np.abs(xf - xl)) <= 1e-7 * np.max(np.abs(xl))
        assert gm_trace_close(tf[:k], tl[:k], rtol=1e-9, atol=1e-12)
        assert itf == il and (not whole or np.isclose(rf, rl, rtol=1e-9, atol=1e-12))
    # lazy polling and device vectors: the same bits
    s = sa.GMRES.new(A, n, m)
    x2 = np.zeros(n, dt)
    assert _run(sa, s, P, rhs, x2, max_iter, tol)[:2] == (sf, itf) and np.array_equal(x2, xf)
    d_rhs = sa.DevVec.from_numpy(rhs); d_x = sa.DevVec.from_numpy(np.zeros(n, dt))
    assert _run(sa, s, P, d_rhs, d_x, max_iter, tol)[:2] == (sf, itf) and np.array_equal(d_x.to_numpy(), xf)


def test_idrs_and_lobpcg_do_not_take_the_handle(sa):
    """The library has no sprs_bjacobi_idrs_* / sprs_bjacobi_lobpcg_* entry points (their lists are pinned by tests/test_idrs_cpu.py and
    tests/test_lobpcg_cpu.py): the two mirrors say so with a TypeError before anything is launched."""
    ip, ix, d, rhs, A, P = _handles(sa, "cgrid", F64)
    n = rhs.size
    x = np.zeros(n)
    with pytest.raises(TypeError, match="BlockJacobi"):
        sa.IDRS.new(A, n, 4).precond_solve(P, rhs, x, 10, 1e-10)
    with pytest.raises(TypeError, match="DiagPrecond, ILU0, AMG or FSAI"):
        sa.Lobpcg.new(A, n, 8).solve(2, "smallest", precond=P)
    assert not np.any(x)
    from sprsolve_amd import _lib
    assert not any("bjacobi_idrs" in k or "bjacobi_lobpcg" in k for k in _lib.PROTOTYPES)
