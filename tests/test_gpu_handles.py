"""GPU checks of what every solver handle shares: the context's knob table, the staging of a solve's vectors and the life of a
handle, over all 13 kinds."""
import numpy as np
import pytest

import _lsmr_ref

pytestmark = pytest.mark.gpu

F64, C32 = np.float64, np.complex64
INVALID_ARGUMENT = 7
MAX_GRID = 4096


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()          # fail loudly if the HIP extension is missing
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ knobs
TRI = ("xcd_chunk", "spmv_wide", "spmv_uniform", "spmv_period", "spmv_triple", "spmv_seam", "spmv_tile", "spmv_chain", "spmv_fuse",
       "p2p_allreduce", "ew_chunk", "stream_nt", "spmv_eqrows", "spmv_wideload")
# key -> (default, ((value set, what a get then returns; None: the set is refused and the knob keeps its value), ...))
KNOBS = {
    "grid": (None, ((7, None), (8, 8), (13, 8), (MAX_GRID - 1, MAX_GRID - 8), (MAX_GRID, MAX_GRID), (MAX_GRID + 1, None), (-1, None))),
    "spmv_grid": (-1, ((4, None), (0, None), (7, None), (8, 8), (13, 8), (MAX_GRID // 2, MAX_GRID // 2), (MAX_GRID // 2 + 1, None),
                       (-5, -1))),
    "spmv_dict": (-1, ((3, None), (-2, None), (2, 2), (0, 0), (1, 1), (-1, -1))),
    "bicg_k5": (-1, ((3, None), (2, 2), (1, 1), (0, 0), (-5, -1))),
    "p2p_timeout_ms": (20000, ((0, 1), (-3, 1), (5, 5), (1 << 20, 1 << 20))),
    "halo_overlap": (1, ((0, 0), (7, 1), (-5, 1))),
    "gs_graph": (0, ((7, 1), (0, 0), (-1, 1))),
    "poll": (16, ((0, None), (-1, None), (1, 1), (1000, 1000))),
}
KNOBS.update({k: (-1, ((-5, -1), (7, 1), (0, 0), (1, 1), (-1, -1))) for k in TRI})


def test_every_knob_by_set_and_get(sa):
    """Defaults, each accepted extreme, each rounding and each refusal of sprs_ctx_set, as sprs_ctx_get reads them back."""
    from sprsolve_amd import _lib
    L = _lib.lib()
    ctx = sa.Context(0)           # a context of its own: its knobs are the defaults and touch no other test
    try:
        num_cu = L.sprs_ctx_get(ctx.h, b"num_cu")
        assert num_cu > 0 and L.sprs_ctx_get(ctx.h, b"device") == 0
        for key in ("num_cu", "device", "no_such_knob", ""):
            before = L.sprs_ctx_get(ctx.h, key.encode())
            assert L.sprs_ctx_set(ctx.h, key.encode(), 1) == INVALID_ARGUMENT, key
            assert L.sprs_ctx_get(ctx.h, key.encode()) == before, key
        assert L.sprs_ctx_get(ctx.h, b"no_such_knob") == -1 and L.sprs_ctx_get(ctx.h, b"") == -1
        assert len(KNOBS) == 22
        for key, (default, steps) in KNOBS.items():
            k = key.encode()
            if key == "grid":
                default = min((num_cu * 2 + 7) // 8 * 8, MAX_GRID)     # two workgroups per CU, a multiple of 8
            now = L.sprs_ctx_get(ctx.h, k)
            assert now == default, (key, now)
            for value, expect in steps:
                st = L.sprs_ctx_set(ctx.h, k, value)
                assert st == (INVALID_ARGUMENT if expect is None else 0), (key, value, st)
                now = now if expect is None else expect
                assert L.sprs_ctx_get(ctx.h, k) == now, (key, value)
    finally:
        ctx.close()


# ------------------------------------------------------------------ staging
class _View:
    """A device vector of n entries that begins one element into `base`: 8 bytes off a 16-byte boundary for f64 and c32."""

    def __init__(self, base, n):
        self.base, self.n = base, n
        self.is_cuda, self.dtype = True, base.dtype.name

    def data_ptr(self):
        return self.base.ptr.value + self.base.dtype.itemsize

    def numel(self):
        return self.n


def _staging_case(sa, kind, dt):
    """-> (a solver, rhs, x0, a tolerance): n = 33 unknowns, one element past a 32-element pad."""
    from sprsolve_amd import gen
    n = 33
    rng = np.random.default_rng(33)
    if kind == "lsmr":
        ip, ix, d, rhs = _lsmr_ref.system(40, n, dt, seed=73, consistent=True)
        A = sa.HipCsr.new((40, n), ip, ix, d)
        s = sa.LSMR.new(A)
    else:
        ip, ix, d, rhs = (gen.hermitian_banded if np.dtype(dt).kind == "c" else gen.symmetric_banded)(n)
        A = sa.HipCsr.new((n, n), ip, ix, d.astype(dt))
        s = sa.CG.new(A, n)
    x0 = rng.uniform(-0.1, 0.1, n) + (1j * rng.uniform(-0.1, 0.1, n) if np.dtype(dt).kind == "c" else 0)
    return s, np.asarray(rhs).astype(dt), x0.astype(dt), (1e-5 if dt is C32 else 1e-10)


def _outcome(sa, s, rhs, x, max_iter, tol):
    E = sa.error
    try:
        return ("ok",) + tuple(s.solve(rhs, x, max_iter, tol))
    except E.InsufficientIterNum as e:
        return ("insufficient", e.iters)


@pytest.mark.parametrize("kind,dt", [("cg", F64), ("cg", C32), ("lsmr", F64)], ids=["cg-f64", "cg-c32", "lsmr-f64"])
def test_staging_gives_the_same_bits(sa, kind, dt):
    """Host arrays, aligned device vectors (used in place) and device views one element off (staged through the solver's buffers)
    give the same iteration count, residual and x, bit for bit: after a solve that converges, and after one cut short at
    max_iter = 1, whose x must come back as well."""
    s, rhs, x0, tol = _staging_case(sa, kind, dt)
    n, m = x0.size, rhs.size
    for max_iter in (200, 1):
        got = []
        x = x0.copy()                                                           # host
        got.append((_outcome(sa, s, rhs, x, max_iter, tol), x))
        drhs, dx = sa.DevVec.from_numpy(rhs), sa.DevVec.from_numpy(x0)          # aligned device vectors
        assert drhs.ptr.value % 16 == 0 and dx.ptr.value % 16 == 0
        got.append((_outcome(sa, s, drhs, dx, max_iter, tol), dx.to_numpy()))
        orhs = sa.DevVec.from_numpy(np.concatenate([rhs[:1], rhs]))             # views one element off
        ox = sa.DevVec.from_numpy(np.concatenate([x0[:1], x0]))
        vrhs, vx = _View(orhs, m), _View(ox, n)
        assert vrhs.data_ptr() % 16 == 8 and vx.data_ptr() % 16 == 8
        got.append((_outcome(sa, s, vrhs, vx, max_iter, tol), ox.to_numpy()[1:]))
        assert np.array_equal(bits(ox.to_numpy()[:1]), bits(x0[:1]))            # the element before the view is not touched
        for v in (drhs, dx, orhs, ox):
            v.free()
        (out0, xh), rest = got[0], got[1:]
        assert out0[0] == ("ok" if max_iter > 1 else "insufficient"), out0
        assert not np.array_equal(bits(xh), bits(x0)), "x comes back modified"
        for out, xd in rest:
            assert out == out0, (max_iter, out, out0)
            assert np.array_equal(bits(xd), bits(xh)), max_iter
    s.close()


# ------------------------------------------------------------------ lifecycle
def _symband30(sa):
    from sprsolve_amd import gen
    ip, ix, d, rhs = gen.symmetric_banded(30)
    D = np.zeros((30, 30))
    D[np.repeat(np.arange(30), np.diff(ip)), ix] = d
    return sa.HipCsr.new((30, 30), ip, ix, d), D, rhs


# kind -> (the class, new's arguments that are refused, the exception, new's arguments that work).  "n + 1": a wrong size.
def _kinds(sa, A, other):
    E = sa.error
    n = 30
    return {
        "bicgstab": (sa.BiCGStab, (A, n + 1), E.DimensionMismatch, (A, n)),
        "minres": (sa.MinRes, (A, n + 1), E.DimensionMismatch, (A, n)),
        "csminres": (sa.CSMinRes, (A, n + 1), E.DimensionMismatch, (A, n)),
        "cg": (sa.CG, (A, n + 1), E.DimensionMismatch, (A, n)),
        "gmres": (sa.GMRES, (A, n, 65), ValueError, (A, n, 10)),
        "idrs": (sa.IDRS, (A, n, 9), ValueError, (A, n, 2)),
        "cgmany": (sa.CGMany, (A, n, 9), ValueError, (A, n, 2)),
        "cgshift": (sa.CGShift, (A, n, 9), ValueError, (A, n, 2)),
        "lsmr": (sa.LSMR, (A, other), E.DimensionMismatch, (A,)),
        "eigsh": (sa.Eigsh, (A, n, 2), ValueError, (A, n, 12)),
        "lobpcg": (sa.Lobpcg, (A, n, 9), ValueError, (A, n, 3)),
        "svds": (sa.Svds, (A, 2), ValueError, (A, 12)),
        "expm": (sa.Expm, (A, n, 2), ValueError, (A, n, 12)),
    }


def _solves(sa, kind, s, D, rhs):
    """One solve on the 30 x 30 symmetric positive-definite band matrix D (strictly diagonally dominant with unit margin, so
    cond(D) < 20): a relative residual of 1e-10 bounds the relative error of x by 2e-9; eigenvalues and singular values asked
    to 1e-10 |D| are compared to 1e-8 |D|."""
    n = 30
    xs = np.linalg.solve(D, rhs)
    lam = np.linalg.eigvalsh(D)
    close = lambda x, ref, tol: np.linalg.norm(np.asarray(x) - ref) <= tol * np.linalg.norm(ref)
    if kind in ("bicgstab", "minres", "csminres", "cg", "gmres", "idrs", "lsmr"):
        x = np.zeros(n)
        s.solve(rhs, x, 200, 1e-10)
        assert close(x, xs, 1e-8)
    elif kind == "cgmany":
        B = np.ascontiguousarray(np.stack([rhs, 2 * rhs], axis=1)); X = np.zeros((n, 2))
        its, res, status = s.solve(B, X, 200, 1e-10)
        assert not status.any() and close(X[:, 0], xs, 1e-8) and close(X[:, 1], 2 * xs, 1e-8)
    elif kind == "cgshift":
        X = np.zeros((2, n))
        its, res, status = s.solve([0.0, 0.5], rhs, X, 200, 1e-10)
        assert not status.any() and close(X[0], xs, 1e-8) and close(X[1], np.linalg.solve(D + 0.5 * np.eye(n), rhs), 1e-8)
    elif kind == "eigsh":
        vals, X, info = s.solve(2, "largest")
        assert info["nconv"] == 2 and close(vals, lam[::-1][:2], 1e-8)
    elif kind == "lobpcg":
        vals, X, info = s.solve(2, "smallest")
        assert info["nconv"] == 2 and close(vals, lam[:2], 1e-8)
    elif kind == "svds":
        sv, U, V, info = s.solve(2, "largest")
        assert info["nconv"] == 2 and close(sv, lam[::-1][:2], 1e-8)            # positive definite: the singular values are the eigenvalues
    elif kind == "expm":
        w, info = s.apply(0.1, rhs)                                             # tol = sqrt(eps): err <= 1.2 |t| tol |v|-ish, far below 1e-6
        Q = np.linalg.eigh(D)[1]
        assert close(w, Q @ (np.exp(0.1 * lam) * (Q.T @ rhs)), 1e-6)
    else:
        raise KeyError(kind)


def test_lifecycle_of_every_kind(sa):
    """A `new` that the library refuses leaves an object whose close() and __del__ do nothing; after it a good `new` on the same
    context works and solves; close() twice is fine."""
    A, D, rhs = _symband30(sa)
    other = sa.HipCsr.new((5, 5), np.arange(6, dtype=np.int32), np.arange(5, dtype=np.int32), np.ones(5))   # not A's adjoint
    kinds = _kinds(sa, A, other)
    assert len(kinds) == 13
    for kind, (cls, bad, exc, good) in kinds.items():
        s = cls.__new__(cls)
        with pytest.raises(exc):
            s.__init__(*bad)
        assert s.h is None, kind
        s.close(); s.close(); s.__del__()
        assert s.h is None, kind
        s = cls.new(*good)
        assert s.h, kind
        _solves(sa, kind, s, D, rhs)
        s.close()
        assert s.h is None, kind
        s.close(); s.__del__()
    other.close(); A.close()
