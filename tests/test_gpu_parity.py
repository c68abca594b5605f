"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle and the golden
fixtures.  Bit-exact wherever the arithmetic order is the reference's (element-wise BLAS-1,
Jacobi apply, SpMV rows handled by the stream path); stated tolerances for reductions."""
import numpy as np
import pytest

import _golden as G

pytestmark = pytest.mark.gpu

RED_RTOL = 1e-13      # dot / nrm2: same terms, different summation order (relative to sum |terms|)
RED_RTOL_F32 = 2e-5   # the same in single precision (the oracle's serial f32 fold is the less accurate side)
ALL_DTYPES = [np.float64, np.complex128, np.float32, np.complex64]
ALL_IDS = ["f64", "c64", "f32", "c32"]


def is_single(dtype):
    return np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64))
TRACE_RTOL = 1e-9     # lock-step scalar trace over the first iterations (SURVEY §7 hard parts (ii))


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()          # fail loudly if the HIP extension is missing
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize in (8, 16) and a.dtype.kind != "c" or a.dtype == np.complex128 else a.view(np.uint32)


def rand_vec(n, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "c":
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(dtype)
    return rng.uniform(-1, 1, n).astype(dtype)


# ------------------------------------------------------------------ SpMV
@pytest.mark.parametrize("case", G.load("spmv_kat.json")["cases"], ids=lambda c: c["name"])
def test_spmv_golden(sa, oracle, case):
    indptr, indices, data, x, exp = G.spmv_case(case)
    A = sa.HipCsr.new(case["shape"], indptr, indices, data, storage=case["storage"])
    y = np.full(5, 7.0, dtype=data.dtype)      # must be overwritten (zero fill, mat.rs:71)
    A.mul_vec(x, y)
    assert np.all(np.abs(y - exp) < case["eps"] * 1.5)
    ref = (oracle.spmv_csc(5, indptr, indices, data, x) if case["storage"] == "CSC"
           else oracle.spmv(indptr, indices, data, x))
    assert np.array_equal(bits(y), bits(ref)), "short rows must be bit-identical to the reference fold"
    y2 = np.zeros_like(y)
    d = A.mul_vec_dot(x, y2)                    # mkl_mat.rs:432-463
    assert np.array_equal(bits(y2), bits(ref))
    e = oracle.conj_dot(x, ref)
    assert abs(d - e) <= 1e-14 * max(1.0, abs(e))


def test_spmv_dimension_mismatch(sa):
    case = G.load("spmv_kat.json")["cases"][1]
    indptr, indices, data, x, exp = G.spmv_case(case)
    A = sa.HipCsr.new((5, 5), indptr, indices, data)
    with pytest.raises(sa.error.DimensionMismatch):
        A.mul_vec(np.zeros(4), np.zeros(4))
    with pytest.raises(sa.error.DimensionMismatch):
        A.mul_vec(np.zeros(5), np.zeros(6))
    with pytest.raises(ValueError):
        sa.HipCsr.new((5, 5), indptr, np.array([1, 2, 9, 2, 3, 4, 4]), data)   # column out of range
    with pytest.raises(ValueError):
        sa.HipCsr.new((5, 5), np.array([0, 3, 2, 5, 6, 7]), indices, data)     # non-monotone indptr


def random_csr(n, seed, dtype, long_rows=True):
    """Ragged random CSR: empty rows, 1..9-nnz rows, and a few rows longer than the
    wavefront-per-row threshold."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 10, n)
    cnt[rng.integers(0, n, max(1, n // 50))] = 0
    if long_rows and n > 400:
        for r in rng.integers(0, n, 6):
            cnt[r] = rng.integers(97, 400)
        cnt[n // 2] = min(n, 3000)
        cnt[n // 2 + 1] = 130          # consecutive long rows share a vector block
    indptr = np.zeros(n + 1, dtype=np.int64); np.cumsum(cnt, out=indptr[1:])
    indices = np.concatenate([np.sort(rng.choice(n, c, replace=False)) for c in cnt]) if indptr[-1] else np.zeros(0, int)
    data = rand_vec(int(indptr[-1]), dtype, seed + 1)
    return indptr.astype(np.int32), indices.astype(np.int32), data, cnt


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=ALL_IDS)
@pytest.mark.parametrize("n", [1, 63, 257, 5000, 40001])
def test_spmv_random_ragged(sa, oracle, dtype, n):
    indptr, indices, data, cnt = random_csr(n, 100 + n, dtype)
    x = rand_vec(n, dtype, 7)
    A = sa.HipCsr.new((n, n), indptr, indices, data)
    y = np.empty(n, dtype=dtype)
    A.mul_vec(x, y)
    ref = oracle.spmv(indptr, indices, data, x)
    short = cnt <= 96
    assert np.array_equal(bits(y[short]), bits(ref[short])), "stream-path rows must be bit-exact"
    if (~short).any():
        # wavefront-per-row path: re-associated sum, tolerance relative to sum |x*val|
        absA = oracle.spmv(indptr, indices, np.abs(data).astype(dtype), np.abs(x).astype(dtype))
        assert np.all(np.abs(y[~short] - ref[~short]) <= (RED_RTOL_F32 if is_single(dtype) else RED_RTOL) * np.abs(absA[~short]))
    # i64 / u32 index ingest (mat.rs:196-199) gives the same bits
    for idt in (np.int64, np.uint32, np.uint64):
        B = sa.HipCsr.new((n, n), indptr.astype(idt), indices.astype(idt), data)
        y2 = np.empty(n, dtype=dtype); B.mul_vec(x, y2)
        assert np.array_equal(bits(y2), bits(y))
        B.close()


def test_spmv_empty_matrix(sa):
    A = sa.HipCsr.new((4, 4), np.zeros(5, np.int32), np.zeros(0, np.int32), np.zeros(0))
    y = np.ones(4); A.mul_vec(np.ones(4), y)
    assert np.array_equal(y, np.zeros(4))


@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=["f64", "c64"])
def test_spmv_csc_matches_reference_scatter(sa, oracle, dtype):
    import scipy.sparse as sp
    n = 700
    indptr, indices, data, _ = random_csr(n, 5, dtype, long_rows=False)
    M = sp.csr_matrix((data, indices, indptr), shape=(n, n)).tocsc()
    x = rand_vec(n, dtype, 9)
    A = sa.HipCsr.new((n, n), M.indptr, M.indices, M.data, storage="CSC")
    y = np.empty(n, dtype=dtype); A.mul_vec(x, y)
    ref = oracle.spmv_csc(n, M.indptr, M.indices, M.data, x)
    assert np.array_equal(bits(y), bits(ref))


def test_spmv_device_vectors_and_grid_options(sa, oracle):
    from sprsolve_amd import gen
    indptr, indices, data = gen.grid_laplacian_dirichlet(300, 300)
    n = 300 * 300
    x = rand_vec(n, np.float64, 3)
    ref = oracle.spmv(indptr, indices, data, x)
    A = sa.HipCsr.new((n, n), indptr, indices, data)
    ctx = sa.default_ctx()
    g0, c0, s0 = ctx.get("grid"), ctx.get("xcd_chunk"), ctx.get("spmv_grid")
    try:
        for grid, chunk in ((g0, 1), (g0, 0), (8, 1), (64, 0), (2048, 1), (1024, -1)):
            ctx.set("spmv_grid", grid); ctx.set("grid", min(grid, 2048)); ctx.set("xcd_chunk", chunk)
            dx = sa.DevVec.from_numpy(x); dy = sa.DevVec(n, np.float64); dy.upload(np.full(n, np.nan))
            A.mul_vec_unchecked(dx, dy)
            assert np.array_equal(bits(dy.to_numpy()), bits(ref)), (grid, chunk)
            d = A.mul_vec_dot_unchecked(dx, dy)
            e = oracle.conj_dot(x, ref)
            assert abs(d - e) <= RED_RTOL * np.sum(np.abs(x * ref))
    finally:
        ctx.set("grid", g0); ctx.set("xcd_chunk", c0); ctx.set("spmv_grid", s0)


@pytest.mark.parametrize("n", [17, 64, 333, 4099, 70001])
def test_plain_stream_wide_loads(sa, oracle, n):
    """spmv_wide_kernel (f64 plain stream, 16 bytes per lane over each block's 16-byte-aligned window; knob spmv_wideload):
    y bit-identical to the 4/8-byte kernel and to the reference fold for every phase of the window (blocks start at any
    nnz index mod 4), for an nnz count that is not a multiple of 4 (the arrays' last group comes from the padded copy),
    rows of 0..9 and of > 96 entries, rows of 8 entries (blocks of 63 rows: the 508-entry cap) — and on device arrays that
    are NOT 16-byte aligned the handle silently keeps the narrow kernel."""
    import torch
    ctx = sa.default_ctx()
    d0, w0 = ctx.get("spmv_dict"), ctx.get("spmv_wideload")
    try:
        ctx.set("spmv_dict", 0)
        for variant in ("ragged", "eight"):
            if variant == "ragged":
                indptr, indices, data, cnt = random_csr(n, 900 + n, np.float64)
            else:
                rng = np.random.default_rng(n)
                cnt = np.full(n, min(8, n)); cnt[n // 3] = min(3, n)
                indptr = np.zeros(n + 1, np.int32); np.cumsum(cnt, out=indptr[1:])
                indices = np.concatenate([np.sort(rng.choice(n, c, replace=False)) for c in cnt]).astype(np.int32)
                data = rand_vec(int(indptr[-1]), np.float64, n + 1)
            x = rand_vec(n, np.float64, 3 + n)
            ref = oracle.spmv(indptr, indices, data, x)
            short = cnt <= 96
            ys = {}
            for wl in (0, 1):
                ctx.set("spmv_wideload", wl)
                A = sa.HipCsr.new((n, n), indptr, indices, data)
                y = np.full(n, np.nan); A.mul_vec(x, y)
                y2 = np.zeros(n); dd = A.mul_vec_dot(x, y2)
                assert np.array_equal(bits(y[short]), bits(ref[short])), (variant, wl, n)
                assert np.array_equal(bits(y), bits(y2))
                assert abs(dd - np.dot(x, y)) <= RED_RTOL * np.sum(np.abs(x * y)) + 1e-300
                ys[wl] = y
            assert np.array_equal(bits(ys[0][short]), bits(ys[1][short]))
            # device arrays one element off a 16-byte boundary: the wide kernel must not be chosen (and nothing faults)
            ctx.set("spmv_wideload", 1)
            if indptr[-1] > 0:
                dev = torch.device("cuda", 0)
                ci = torch.zeros(int(indptr[-1]) + 1, dtype=torch.int32, device=dev)[1:]; ci.copy_(torch.from_numpy(indices.astype(np.int32)))
                va = torch.zeros(int(indptr[-1]) + 1, dtype=torch.float64, device=dev)[1:]; va.copy_(torch.from_numpy(data))
                ip = torch.from_numpy(indptr.astype(np.int32)).to(dev)
                assert ci.data_ptr() % 16 != 0 or va.data_ptr() % 16 != 0
                Au = sa.HipCsr.from_device((n, n), int(indptr[-1]), ip, ci, va, adopt=True)
                xd = torch.from_numpy(x).to(dev); yd = torch.empty_like(xd)
                Au.mul_vec_unchecked(xd, yd)
                assert np.array_equal(bits(yd.cpu().numpy()[short]), bits(ref[short]))
    finally:
        ctx.set("spmv_dict", d0); ctx.set("spmv_wideload", w0)


def test_eqrows_poll_and_chunk_knobs(sa, oracle):
    """The three knobs no other test turns: spmv_eqrows (plain stream: equal-length blocks take their extents from the
    descriptor — read at creation; y bit-identical either way), poll (how often the host looks at the status word: the
    iterates cannot depend on it), ew_chunk (XCD-chunked walk of the fused kernels: groups the reductions' partials
    differently, nothing else)."""
    from sprsolve_amd import gen
    R = 96
    indptr, indices, data = gen.grid_laplacian_dirichlet(R, R)
    rhs = gen.dirichlet_rhs(R, R)
    n = R * R
    x = rand_vec(n, np.float64, 17)
    ref = oracle.spmv(indptr, indices, data, x)
    ctx = sa.default_ctx()
    e0, p0, c0, d0 = ctx.get("spmv_eqrows"), ctx.get("poll"), ctx.get("ew_chunk"), ctx.get("spmv_dict")
    try:
        ctx.set("spmv_dict", 0)
        for eq in (0, 1):
            ctx.set("spmv_eqrows", eq)
            A = sa.HipCsr.new((n, n), indptr, indices, data)
            nb, ne = A.wide_blocks()
            assert nb == (n + 63) // 64 and (ne > 0) == (eq == 1), (eq, nb, ne)      # rows 1..R-2 of the grid hold 5-entry runs
            y = np.full(n, np.nan); A.mul_vec(x, y)
            assert np.array_equal(bits(y), bits(ref)), eq
        ctx.set("spmv_dict", -1); ctx.set("spmv_eqrows", -1)
        A = sa.HipCsr.new((n, n), indptr, indices, data)
        out = {}
        for poll in (1, 16, 7):
            ctx.set("poll", poll)
            s = sa.BiCGStab.new(A, n)
            xs = np.zeros(n)
            out[poll] = s.solve(rhs, xs, 3000, 1e-10) + (xs.copy(),)
        assert out[1][0] == out[16][0] == out[7][0] and out[1][1] == out[16][1] == out[7][1]
        assert np.array_equal(bits(out[1][2]), bits(out[16][2])) and np.array_equal(bits(out[1][2]), bits(out[7][2]))
        ctx.set("poll", 16)
        g = np.arange(n)
        exact = (g // R + g % R).astype(float)
        for ch in (0, 1):
            ctx.set("ew_chunk", ch)
            s = sa.BiCGStab.new(A, n)
            xs = np.zeros(n)
            its, res = s.solve(rhs, xs, 3000, 1e-10)
            assert res <= 1e-10 and np.max(np.abs(xs - exact)) < 1e-6, (ch, its, res)
    finally:
        ctx.set("spmv_eqrows", e0); ctx.set("poll", p0); ctx.set("ew_chunk", c0); ctx.set("spmv_dict", d0)


# ------------------------------------------------------------------ vecalg
def _run_vecalg(va, case):
    dt = case["dtype"]; op = case["op"]
    x = G.vec(case["x"], dt)
    if op == "norm2":
        return va.norm2(x)
    if op in ("dot", "conj_dot"):
        return getattr(va, op)(x, G.vec(case["y"], dt))
    if op == "scale":
        va.scale(G.scalar(case["a"], dt), x); return x
    if op == "rscale":
        va.rscale(case["a"], x); return x
    if op == "conj":
        out = np.empty_like(x); va.conj(x, out); return out
    if op == "axpy":
        y = G.vec(case["y"], dt)
        a = float(case["a_real"]) if "a_real" in case else G.scalar(case["a"], dt)
        va.axpy(a, x, y); return y
    if op == "axpy_repeat":
        y = G.vec(case["y"], dt)
        for _ in range(case["repeat"]):
            va.axpy(G.scalar(case["a"], dt), x, y)
        return y
    raise KeyError(op)


@pytest.mark.parametrize("case", G.load("vecalg_kat.json")["cases"], ids=lambda c: c["name"])
def test_vecalg_golden(sa, case):
    va = sa.vecalg
    dt = case["dtype"]; eps = case.get("eps", 1e-13)
    if case["op"] == "axpby_sequence":
        x = G.vec(case["x"], dt); y = G.vec(case["y"], dt)
        for st in case["steps"]:
            for _ in range(st["repeat"]):
                va.axpby(G.scalar(st["a"], dt), x, G.scalar(st["b"], dt), y)
            assert np.all(np.abs(y - st["expected_fill"]) <= eps)
        return
    got = _run_vecalg(va, case)
    if "expected" in case:
        assert abs(got - G.scalar(case["expected"], dt)) <= eps
    elif "expected_fill" in case:
        assert np.all(np.abs(got - G.scalar(case["expected_fill"], dt)) <= eps)
    else:
        assert np.all(np.abs(got - G.vec({"array": case["expected_array"]}, dt)) <= eps)


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=ALL_IDS)
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1023, 100003, 1 << 20])
def test_vecalg_random_vs_oracle(sa, oracle, dtype, n):
    va = sa.vecalg
    x = rand_vec(n, dtype, 11); y = rand_vec(n, dtype, 12)
    a = rand_vec(1, dtype, 13)[0]; b = rand_vec(1, dtype, 14)[0]
    cx = np.dtype(dtype).kind == "c"
    a = complex(a) if cx else float(a)
    b = complex(b) if cx else float(b)
    tol = RED_RTOL_F32 if is_single(dtype) else RED_RTOL
    # element-wise ops: same rounding sequence => bit-exact
    yy = y.copy(); va.axpy(a, x, yy)
    assert np.array_equal(bits(yy), bits(oracle.axpy(a, x, y.copy())))
    yy = y.copy(); va.axpby(a, x, b, yy)
    assert np.array_equal(bits(yy), bits(oracle.axpby(a, x, b, y.copy())))
    xx = x.copy(); va.scale(a, xx)
    assert np.array_equal(bits(xx), bits(oracle.scale(a, x.copy())))
    xx = x.copy(); va.rscale(0.3, xx)
    assert np.array_equal(bits(xx), bits(oracle.rscale(0.3, x.copy())))
    out = np.empty_like(x); va.conj(x, out)
    assert np.array_equal(bits(out), bits(oracle.conj(x)))
    if cx:
        yy = y.copy(); va.axpy(0.7, x, yy)        # S = Real, T = Complex
        assert np.array_equal(bits(yy), bits(oracle.axpy(0.7, x, y.copy())))
    # reductions: tolerance relative to the sum of magnitudes
    mag = float(np.sum(np.abs(x).astype(np.float64) * np.abs(y).astype(np.float64)))
    assert abs(va.dot(x, y) - oracle.dot(x, y)) <= tol * max(mag, 1e-300)
    assert abs(va.conj_dot(x, y) - oracle.conj_dot(x, y)) <= tol * max(mag, 1e-300)
    exact = float(np.linalg.norm(x.astype(np.complex128 if cx else np.float64)))
    # single precision: the GPU tree sum is the more accurate side; both must be near the f64 value
    assert abs(va.norm2(x) - oracle.norm2(x)) <= (2e-3 if is_single(dtype) else RED_RTOL) * max(exact, 1e-300)
    assert abs(va.norm2(x) - exact) <= (2e-5 if is_single(dtype) else 1e-13) * max(exact, 1e-300)


def test_vecalg_unaligned_device_views(sa, oracle):
    """Vectors that start 8 bytes off a 16-byte boundary take the scalar-access kernels."""
    import ctypes as C
    n = 10001
    x = rand_vec(n + 1, np.float64, 1); y = rand_vec(n + 1, np.float64, 2)
    dx = sa.DevVec.from_numpy(x); dy = sa.DevVec.from_numpy(y)

    class View:      # a device vector one element into another
        def __init__(self, base, n):
            self.base, self.n = base, n
            self.is_cuda, self.dtype = True, "float64"
        def data_ptr(self): return self.base.ptr.value + 8
        def numel(self): return self.n
    vx, vy = View(dx, n), View(dy, n)
    sa.vecalg.axpy(0.5, vx, vy)
    ref = oracle.axpy(0.5, x[1:], y[1:].copy())
    assert np.array_equal(bits(dy.to_numpy()[1:]), bits(ref))
    assert abs(sa.vecalg.dot(vx, vy) - oracle.dot(x[1:], ref)) <= RED_RTOL * np.sum(np.abs(x[1:] * ref))


# ------------------------------------------------------------------ Jacobi preconditioner
def test_diag_precond(sa, oracle):
    n = 5003
    d = rand_vec(n, np.float64, 1) + 2.0
    v = rand_vec(n, np.float64, 2)
    P = sa.DiagPrecond.new(d)
    out = np.empty(n); P.mul_vec(v, out)
    assert np.array_equal(bits(out), bits(oracle.diag_apply(oracle.diag_inv(d), v)))
    vz = rand_vec(n, np.complex128, 3)
    Pzd = sa.DiagPrecond.new(d, t_dtype=np.complex128)      # DiagPrecond<Complex64, f64>
    outz = np.empty(n, np.complex128); Pzd.mul_vec(vz, outz)
    assert np.array_equal(bits(outz), bits(oracle.diag_apply(oracle.diag_inv(d), vz)))
    dz = rand_vec(n, np.complex128, 4) + 2.0
    Pz = sa.DiagPrecond.new(dz)                              # DiagPrecond<Complex64, Complex64>
    Pz.mul_vec(vz, outz)
    assert np.array_equal(bits(outz), bits(oracle.diag_apply(oracle.diag_inv(dz), vz)))
    with pytest.raises(sa.error.DimensionMismatch):
        P.mul_vec(np.zeros(n - 1), np.zeros(n - 1))
    with pytest.raises(NotImplementedError):
        P.mul_vec_dot(v, out)


# ------------------------------------------------------------------ solvers
def _make(sa, case, p):
    n = p["rhs"].size
    A = sa.HipCsr.new((n, n), p["indptr"], p["indices"], p["data"])
    cls = {"bicgstab": sa.BiCGStab, "minres": sa.MinRes, "csminres": sa.CSMinRes}[case["solver"]]
    solver = cls.new(A, A.cols())
    pc = None
    if p["diag"] is not None:
        pc = sa.DiagPrecond.new(p["diag"], t_dtype=p["data"].dtype)
    return A, solver, pc


@pytest.mark.parametrize("mode", ["fused", "literal"])
@pytest.mark.parametrize("case", G.load("solver_kat.json")["cases"], ids=lambda c: c["name"])
def test_solver_golden(sa, oracle, case, mode):
    """The reference's integration tests (assert Ok) + the exact solutions they imply."""
    p = G.solver_problem(case)
    A, solver, pc = _make(sa, case, p)
    solver.set_mode(mode)
    x = np.zeros_like(p["rhs"])
    # sub-epsilon tolerances make the iteration count reduction-order noise: the
    # reference asserts only Ok; we assert Ok and the implied exact solution
    if pc is not None:
        iters, res = solver.precond_solve(pc, p["rhs"], x, case["max_iter"], case["tol"])
    else:
        iters, res = solver.solve(p["rhs"], x, case["max_iter"], case["tol"])
    scale = max(1.0, np.max(np.abs(p["exact"])))
    assert np.max(np.abs(x - p["exact"])) / scale < 1e-9, (iters, res)
    true_res = np.linalg.norm(oracle.spmv(p["indptr"], p["indices"], p["data"], x) - p["rhs"]) / np.linalg.norm(p["rhs"])
    assert true_res < 1e-10
    assert res <= case["tol"]


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=ALL_IDS)
def test_reductions_in_the_oracles_emulated_gpu_order(sa, oracle, dtype):
    """The oracle can add the terms of a dot product / norm in the order of the library's stand-alone reduction kernels
    (oracle/krylov_tmpl.h, "reductions as the SOLVERS call them"): grid-stride fold per thread over 16-byte packs, wavefront
    butterfly, the workgroup's four wavefronts left to right, one partial per workgroup, the partials folded the same
    way.  The GPU's conj_dot / norm2 must then equal it BIT FOR BIT — the premise of the test below."""
    grid = sa.default_ctx().get("grid")
    oracle.set_reduction_order("gpu", grid)
    try:
        for n in (1, 3, 255, 256, 257, 511, 5000, 131072, 131075, 1_000_003):
            x = rand_vec(n, dtype, 40 + n % 7); y = rand_vec(n, dtype, 50 + n % 5)
            d = sa.vecalg.conj_dot(x, y); e = oracle.conj_dot_gpu_order(x, y)
            assert np.array_equal(bits(np.array([d], dtype=dtype)), bits(np.array([e], dtype=dtype))), (n, d, e)
            rdt = np.float32 if is_single(dtype) else np.float64
            assert np.array_equal(bits(np.array([sa.vecalg.norm2(x)], dtype=rdt)), bits(np.array([oracle.norm2_gpu_order(x)], dtype=rdt))), n
    finally:
        oracle.set_reduction_order("reference")


_BITWISE_CASES = [c for c in G.load("solver_kat.json")["cases"]]


@pytest.mark.parametrize("case", _BITWISE_CASES, ids=lambda c: c["name"])
def test_literal_mode_is_the_oracle_bit_for_bit(sa, oracle, case):
    """The strongest statement about the host recurrences this repository can make: with SpMV and every element-wise
    kernel bit-exact, and the oracle adding its dot products in the GPU kernels' order (the only freedom the parity
    contract leaves), the library's LITERAL mode — one kernel per reference op, scalars consumed on the host where
    bicg_stab.rs / minres.rs / cs_minres.rs consume them — must reproduce the oracle's restatement of the reference
    recurrence BIT FOR BIT over the whole solve of the reference's own test problems: every traced scalar of every
    iteration (so every restart, breakdown and convergence decision), the iteration count, the residual and x.
    (The default fused mode regroups the same terms differently again and is compared with this one to rounding.)"""
    p = G.solver_problem(case)
    A, solver, pc = _make(sa, case, p)
    solver.set_mode("literal")
    K = 4096
    solver.set_trace(K)
    x = np.zeros_like(p["rhs"])
    oracle.set_reduction_order("gpu", sa.default_ctx().get("grid"))
    try:
        ref = getattr(oracle, case["solver"])(p["indptr"], p["indices"], p["data"], p["rhs"], np.zeros_like(p["rhs"]),
                                              case["max_iter"], case["tol"], precond_diag=p["diag"], trace_cap=K)
    finally:
        oracle.set_reduction_order("reference")
    assert ref.status == oracle.OK
    if pc is not None:
        iters, res = solver.precond_solve(pc, p["rhs"], x, case["max_iter"], case["tol"])
    else:
        iters, res = solver.solve(p["rhs"], x, case["max_iter"], case["tol"])
    tr = solver.trace()
    assert iters == ref.its and res == ref.res, (iters, ref.its, res, ref.res)
    assert tr.shape == ref.trace.shape and tr.shape[0] >= min(ref.its, 2)
    assert np.array_equal(tr.view(np.uint64), ref.trace.view(np.uint64)), \
        "first differing trace row: %d" % int(np.argmax(np.any(tr.view(np.uint64) != ref.trace.view(np.uint64), axis=1)))
    assert np.array_equal(bits(x), bits(ref.x))


def test_literal_mode_bit_for_bit_on_the_bench_problem_and_cfg2(sa, oracle):
    """The same on the reference's own bench (benches/bicgstab.rs: 100 x 100 Dirichlet grid, tol 1e-16, max 1500 — about
    900 iterations, the restart branch live) and on a cfg-2-shaped system (300 x 300, BiCGStab + Jacobi)."""
    from sprsolve_amd import gen
    oracle.set_reduction_order("gpu", sa.default_ctx().get("grid"))
    try:
        for R, jac, tol, mx in ((100, False, 1e-16, 1500), (300, True, 1e-12, 4000)):
            indptr, indices, data = gen.grid_laplacian_dirichlet(R, R)
            rhs = gen.dirichlet_rhs(R, R)
            n = R * R
            diag = np.where(np.diff(indptr) == 1, 1.0, -4.0) if jac else None
            ref = oracle.bicgstab(indptr, indices, data, rhs, np.zeros(n), mx, tol, precond_diag=diag, trace_cap=mx + 1)
            A = sa.HipCsr.new((n, n), indptr, indices, data)
            s = sa.BiCGStab.new(A, n); s.set_mode("literal"); s.set_trace(mx + 1)
            x = np.zeros(n)
            try:
                if jac:
                    iters, res = s.precond_solve(sa.DiagPrecond.new(diag), rhs, x, mx, tol)
                else:
                    iters, res = s.solve(rhs, x, mx, tol)
                status = oracle.OK
            except sa.error.InsufficientIterNum as e:
                iters, res, status = e.iters, 0.0, oracle.INSUFFICIENT_ITER
            assert status == ref.status and iters == ref.its and (status != oracle.OK or res == ref.res), (R, iters, ref.its)
            tr = s.trace()
            assert tr.shape == ref.trace.shape and tr.shape[0] > 100
            assert np.array_equal(tr.view(np.uint64), ref.trace.view(np.uint64)), (R, int(np.argmax(np.any(tr != ref.trace, axis=1))))
            assert np.array_equal(bits(x), bits(ref.x))
    finally:
        oracle.set_reduction_order("reference")


def test_literal_csminres_and_f32_bit_for_bit(sa, oracle):
    """CSMINRES has no reference fixture (its complex branch stays "parity unpinned" against the REFERENCE), but the
    library and the oracle's line-by-line restatement of cs_minres.rs:29-158 must agree bit for bit over a whole
    complex-symmetric solve once the reductions share their order; likewise the f32 BiCGStab of the Dirichlet grid."""
    from sprsolve_amd import gen
    oracle.set_reduction_order("gpu", sa.default_ctx().get("grid"))
    try:
        for rows, cols in ((8, 8), (40, 60)):
            indptr, indices, data, rhs, diag = gen.complex_symmetric_grid(rows, cols)
            n = rows * cols
            ref = oracle.csminres(indptr, indices, data, rhs, np.zeros(n, np.complex128), 2000, 1e-12, trace_cap=2001)
            A = sa.HipCsr.new((n, n), indptr, indices, data)
            s = sa.CSMinRes.new(A, n); s.set_mode("literal"); s.set_trace(2001)
            x = np.zeros(n, np.complex128)
            its, res = s.solve(rhs, x, 2000, 1e-12)
            assert ref.status == oracle.OK and its == ref.its and res == ref.res
            assert np.array_equal(s.trace().view(np.uint64), ref.trace.view(np.uint64)) and np.array_equal(bits(x), bits(ref.x))
        indptr, indices, data = gen.grid_laplacian_dirichlet(40, 40)
        rhs = gen.dirichlet_rhs(40, 40).astype(np.float32); data = data.astype(np.float32)
        n = 1600
        ref = oracle.bicgstab(indptr, indices, data, rhs, np.zeros(n, np.float32), 800, 1e-6, trace_cap=801)
        A = sa.HipCsr.new((n, n), indptr, indices, data)
        s = sa.BiCGStab.new(A, n); s.set_mode("literal"); s.set_trace(801)
        x = np.zeros(n, np.float32)
        its, res = s.solve(rhs, x, 800, 1e-6)
        assert ref.status == oracle.OK and its == ref.its and np.float32(res) == np.float32(ref.res), (its, ref.its, res, ref.res)
        assert np.array_equal(s.trace().view(np.uint64), ref.trace.view(np.uint64)) and np.array_equal(bits(x), bits(ref.x))
    finally:
        oracle.set_reduction_order("reference")


@pytest.mark.parametrize("mode", ["fused", "literal"])
@pytest.mark.parametrize("case", G.load("solver_kat.json")["cases"], ids=lambda c: c["name"])
def test_solver_trace_lockstep(sa, oracle, case, mode):
    """Scalars of the recurrence agree with the oracle's in lock-step over the first iterations."""
    p = G.solver_problem(case)
    A, solver, pc = _make(sa, case, p)
    solver.set_mode(mode)
    K = 8
    solver.set_trace(K)
    x = np.zeros_like(p["rhs"])
    try:
        if pc is not None:
            solver.precond_solve(pc, p["rhs"], x, K, 0.0)
        else:
            solver.solve(p["rhs"], x, K, 0.0)
    except sa.error.InsufficientIterNum as e:
        assert e.iters == K
    tr = solver.trace()
    ref = getattr(oracle, case["solver"])(p["indptr"], p["indices"], p["data"], p["rhs"], np.zeros_like(p["rhs"]),
                                          K, 0.0, precond_diag=p["diag"], trace_cap=K)
    assert ref.status == oracle.INSUFFICIENT_ITER
    assert tr.shape == ref.trace.shape and tr.shape[0] == K
    assert np.array_equal(tr[:, 0], ref.trace[:, 0])
    # the bench-style Dirichlet problems make rho at its=1 a pure rounding residue:
    # compare every scalar relative to the scale of its column instead of element-wise
    if case["solver"] == "bicgstab" and abs(ref.trace[1][2]) < 1e-9 * abs(ref.trace[0][2]):
        # Dirichlet grids: r0 is supported on the border rows only and the first step zeroes r there, so
        # rho = r0.r at its=1 is EXACTLY 0 in exact arithmetic: what either implementation computes is a
        # pure rounding residue (1.4e-9 against 5e6 in the oracle on the 100x100 bench problem), beta at
        # its=1 is noise and the trajectories part from there.  Lock-step is then only
        # defined for the unrolled iteration and the residual norm it leaves behind.
        assert np.allclose(tr[0], ref.trace[0], rtol=TRACE_RTOL, atol=0)
        # row 1 in full: rho is a residue (1.4e-9 against 5e6) but the SAME residue — the few non-zero products are
        # added in the same order — so alpha = rho / (r0.v), w and |r| agree to rounding as well
        assert np.isclose(tr[1][1], ref.trace[1][1], rtol=TRACE_RTOL)
        assert abs(tr[1][2]) <= 1e-9 * ref.trace[0][2]
        assert np.allclose(tr[1][[4, 6]], ref.trace[1][[4, 6]], rtol=TRACE_RTOL, atol=0)
        # from row 2 on, lock-step until the first LEGITIMATELY ill-conditioned branch: the trajectories may part only
        # at a row whose rho is a cancellation residue on at least one side (|rho| < 1e-10 |r0| |r|: that is where
        # bicg_stab.rs:131 compares it with (|r0| eps)^2 — on the 100x100 bench problem the oracle gets 4.4e-25, just
        # above the threshold 2.6e-25, the GPU's summation order lands below it and restarts), and |r| of that row —
        # computed before the branch — must still agree.  Rows before it must agree in every column.
        r0n = ref.trace[0][1]
        scale = np.maximum(np.max(np.abs(ref.trace), axis=0), 1e-300)
        parted = None
        for k in range(2, K):
            if np.all(np.abs(tr[k] - ref.trace[k]) <= 1e-7 * scale):
                continue
            parted = k
            break
        if parted is not None:
            k = parted
            assert np.isclose(tr[k][1], ref.trace[k][1], rtol=1e-7), (k, tr[k], ref.trace[k])
            residue = 1e-10 * r0n * ref.trace[k][1]
            assert min(abs(tr[k][2]), abs(ref.trace[k][2])) < residue, (k, tr[k], ref.trace[k])
        else:
            assert np.max(np.abs(x - ref.x)) / max(1.0, np.max(np.abs(ref.x))) < 1e-7
        return
    # complex scalars: compare against the magnitude of the (re, im) pair, not of each part
    scale = np.maximum(np.max(np.abs(ref.trace), axis=0), 1e-300)
    pairs = [(2, 3), (4, 5)] + ([(6, 7)] if case["solver"] == "bicgstab" else [])
    for a, b in pairs:
        scale[a] = scale[b] = max(scale[a], scale[b])
    assert np.all(np.abs(tr - ref.trace) <= TRACE_RTOL * scale), np.abs(tr - ref.trace) / scale
    xerr = np.max(np.abs(x - ref.x)) / max(1.0, np.max(np.abs(ref.x)))
    assert xerr < 1e-8


def _dense_case(c, copies=1):
    import scipy.sparse as sp
    M = np.array(c["A"], float)
    A = sp.block_diag([sp.csr_matrix(M)] * copies, format="csr")
    b = np.tile(np.array(c["b"], float), copies)
    return A, b


@pytest.mark.parametrize("copies", [1, 700])
@pytest.mark.parametrize("case", G.load("branch_kat.json")["restart"], ids=lambda c: c["name"])
def test_bicgstab_restart_branch(sa, oracle, case, copies):
    """bicg_stab.rs:131-145: rho == 0 exactly at its=1 -> r, r0, rho are rebuilt."""
    M, b = _dense_case(case, copies)
    ref = oracle.bicgstab(M.indptr, M.indices, M.data, b, np.zeros_like(b), case["max_iter"], case["tol"], trace_cap=4)
    assert ref.trace[1][2] == ref.trace[1][1] ** 2 or np.isclose(ref.trace[1][2], ref.trace[1][1] ** 2, rtol=1e-15)
    A = sa.HipCsr.from_scipy(M)
    for mode in ("fused", "literal"):
        s = sa.BiCGStab.new(A, A.cols()); s.set_mode(mode); s.set_trace(4)
        x = np.zeros_like(b)
        try:
            its, res = s.solve(b, x, case["max_iter"], case["tol"])
            st = oracle.OK
        except sa.error.InsufficientIterNum as e:
            its, st = e.iters, oracle.INSUFFICIENT_ITER
        assert st == ref.status and its == ref.its
        tr = s.trace()
        # the restart replaces rho by |A x - b|^2 at its=1 — visible in the trace
        assert np.isclose(tr[1][2], ref.trace[1][2], rtol=1e-12)
        if ref.status == oracle.OK:
            assert np.allclose(x, ref.x, rtol=1e-9, atol=1e-12)
        else:
            assert np.array_equal(np.isnan(x), np.isnan(ref.x))


@pytest.mark.parametrize("case", G.load("branch_kat.json")["breakdown"], ids=lambda c: c["name"])
def test_bicgstab_breakdown_branch(sa, oracle, case):
    """bicg_stab.rs:164-167: |r0.v| <= 0 -> Err(BreakDown(its))."""
    M, b = _dense_case(case)
    ref = oracle.bicgstab(M.indptr, M.indices, M.data, b, np.zeros_like(b), case["max_iter"], case["tol"])
    assert ref.status == oracle.BREAKDOWN
    A = sa.HipCsr.from_scipy(M)
    for mode in ("fused", "literal"):
        s = sa.BiCGStab.new(A, A.cols()); s.set_mode(mode)
        x = np.zeros_like(b)
        with pytest.raises(sa.error.BreakDown) as ei:
            s.solve(b, x, case["max_iter"], case["tol"])
        assert ei.value.its == ref.its
        assert np.allclose(x, ref.x, rtol=1e-12, atol=1e-14)


def test_solver_error_paths(sa, oracle):
    from sprsolve_amd import gen
    indptr, indices, data = gen.grid_laplacian_dirichlet(12, 12)
    rhs = gen.dirichlet_rhs(12, 12)
    n = 144
    A = sa.HipCsr.new((n, n), indptr, indices, data)
    for cls in (sa.BiCGStab, sa.MinRes, sa.CSMinRes):
        s = cls.new(A, n)
        with pytest.raises(sa.error.IncompatibleMatrixFormat, match="doesn't match the matrix size"):
            s.solve(rhs[:-1], np.zeros(n - 1), 10, 1e-8)
        with pytest.raises(sa.error.IncompatibleMatrixFormat, match="do not match"):
            s.solve(rhs, np.zeros(n + 1), 10, 1e-8)
        # rhs == 0: x := 0, Ok((0, rhs_norm))  (bicg_stab.rs:56-60 — absolute, not relative)
        x = np.ones(n)
        assert s.solve(np.zeros(n), x, 10, 1e-8) == (0, 0.0)
        assert not x.any()
    s = sa.BiCGStab.new(A, n)
    # convergence is tested at the top of the loop: max_iter iterations without the final check
    x = np.zeros(n)
    with pytest.raises(sa.error.InsufficientIterNum) as ei:
        s.solve(rhs, x, 3, 1e-30)
    assert ei.value.iters == 3
    ref = oracle.bicgstab(indptr, indices, data, rhs, np.zeros(n), 3, 1e-30)
    assert np.allclose(x, ref.x, rtol=1e-10, atol=1e-12)
    # warm start from the exact solution: Ok((0, ...)) before any iteration (bicg_stab.rs:81-83)
    i, j = np.meshgrid(np.arange(12), np.arange(12), indexing="ij")
    x = (i + j).ravel().astype(float)
    its, res = s.solve(rhs, x, 10, 1e-12)
    assert its == 0 and res <= 1e-12
    # solver handles of the wrong size are refused instead of indexing out of bounds
    with pytest.raises(sa.error.DimensionMismatch):
        sa.BiCGStab.new(A, n + 1)


def test_minres_invalid_preconditioner(sa, oracle):
    """minres.rs:236-244: r^H M^-1 r must be positive — a negative diagonal is rejected."""
    from sprsolve_amd import gen
    indptr, indices, data, rhs = gen.symmetric_banded(300)
    n = 300
    A = sa.HipCsr.new((n, n), indptr, indices, data)
    s = sa.MinRes.new(A, n)
    bad = sa.DiagPrecond.new(-np.ones(n))
    with pytest.raises(sa.error.InvalidPreconditioner):
        s.precond_solve(bad, rhs, np.zeros(n), 50, 1e-10)
    ref = oracle.minres(indptr, indices, data, rhs, np.zeros(n), 50, 1e-10, precond_diag=-np.ones(n))
    assert ref.status == oracle.INVALID_PRECOND
    # an indefinite diagonal fails later, inside the loop (minres.rs:279-287), at the same iteration
    d = np.ones(n); d[::2] = -1.0
    ref = oracle.minres(indptr, indices, data, rhs, np.zeros(n), 50, 1e-10, precond_diag=d)
    P = sa.DiagPrecond.new(d)
    x = np.zeros(n)
    if ref.status == oracle.INVALID_PRECOND:
        with pytest.raises(sa.error.InvalidPreconditioner):
            s.precond_solve(P, rhs, x, 50, 1e-10)


@pytest.mark.parametrize("mode", ["fused", "literal"])
def test_csminres_complex_symmetric(sa, oracle, mode):
    """CSMinRes has no test upstream: complex-symmetric grid of
    tests/test_complex_solve2.rs with its implied exact solution, lock-step with the oracle."""
    from sprsolve_amd import gen
    for rows, cols in ((8, 8), (40, 60)):
        indptr, indices, data, rhs, diag = gen.complex_symmetric_grid(rows, cols)
        n = rows * cols
        A = sa.HipCsr.new((n, n), indptr, indices, data)
        s = sa.CSMinRes.new(A, n); s.set_mode(mode)
        x = np.zeros(n, np.complex128)
        its, res = s.solve(rhs, x, 2000, 1e-12)
        ref = oracle.csminres(indptr, indices, data, rhs, np.zeros(n, np.complex128), 2000, 1e-12)
        assert ref.status == oracle.OK
        assert abs(its - ref.its) <= max(3, ref.its // 20)
        assert np.max(np.abs(x - gen.grid_exact_solution(rows, cols))) < 1e-8
        K = 6
        s.set_trace(K); x[:] = 0
        with pytest.raises(sa.error.InsufficientIterNum):
            s.solve(rhs, x, K, 0.0)
        reft = oracle.csminres(indptr, indices, data, rhs, np.zeros(n, np.complex128), K, 0.0, trace_cap=K)
        tr = s.trace()
        assert np.allclose(tr, reft.trace, rtol=TRACE_RTOL, atol=1e-12)
        s.set_trace(0)


@pytest.mark.parametrize("mode", ["fused", "literal"])
@pytest.mark.parametrize("name", ["test_minres", "minres_ident"])
def test_csminres_is_minres_for_real_scalars(sa, oracle, name, mode):
    """Pins the shared Saunders code path on reference-held fixtures: for real T cs_minres.rs is arithmetically
    minres.rs (conj = identity), so `csminres_d` must reproduce `minres_d` BIT FOR BIT — trace and x — on the
    reference's two MINRES problems (tests/test_minres.rs:1-60), and both follow the oracle in lock-step."""
    case = [c for c in G.load("solver_kat.json")["cases"] if c["name"] == name][0]
    p = G.solver_problem(case)
    n = p["rhs"].size
    A = sa.HipCsr.new((n, n), p["indptr"], p["indices"], p["data"])
    K = 24
    got = {}
    for cls in (sa.MinRes, sa.CSMinRes):
        s = cls.new(A, n); s.set_mode(mode); s.set_trace(K)
        x = np.zeros(n)
        try:
            s.solve(p["rhs"], x, K, 0.0)
        except sa.error.InsufficientIterNum:
            pass
        got[cls.__name__] = (s.trace(), x.copy())
    (ta, xa), (tb, xb) = got["MinRes"], got["CSMinRes"]
    assert ta.shape == tb.shape and ta.shape[0] == K
    assert np.array_equal(ta.view(np.uint64), tb.view(np.uint64))
    assert np.array_equal(bits(xa), bits(xb))
    ref = oracle.csminres(p["indptr"], p["indices"], p["data"], p["rhs"], np.zeros(n), K, 0.0, trace_cap=K)
    # lock-step with the oracle while the recurrence residual is above rounding level (after convergence the Lanczos
    # vectors are normalised noise; minres_ident converges exactly and its later rows are 0/0)
    ok = np.isfinite(ref.trace).all(axis=1) & (ref.trace[:, 7] > 1e-7 * ref.trace[0, 7])
    assert ok.sum() >= 4
    assert np.allclose(tb[ok], ref.trace[ok], rtol=1e-6, atol=1e-12)
    # to convergence, reference tolerance: same iteration count, same bits
    res = {}
    for cls in (sa.MinRes, sa.CSMinRes):
        s = cls.new(A, n); s.set_mode(mode)
        x = np.zeros(n)
        res[cls.__name__] = s.solve(p["rhs"], x, case["max_iter"], case["tol"]) + (x.copy(),)
    assert res["MinRes"][:2] == res["CSMinRes"][:2]
    assert np.array_equal(bits(res["MinRes"][2]), bits(res["CSMinRes"][2]))
    assert np.max(np.abs(res["CSMinRes"][2] - p["exact"])) < 1e-9


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=ALL_IDS)
def test_copy_and_zero_direct(sa, dtype):
    """a12 — the reference's `ptr::copy_nonoverlapping` (bicg_stab.rs:78,91,140; minres.rs:77,156) and zero fill
    (minres.rs:86-88, bicg_stab.rs:58) as their own entry points: sprs_memcpy_d2d / sprs_memset_zero, every scalar
    type, odd lengths and unaligned offsets, neighbours untouched."""
    import ctypes as C

    from sprsolve_amd import _lib
    L = _lib.lib()
    ctx = sa.default_ctx(0)
    isz = np.dtype(dtype).itemsize
    for n in (1, 63, 1000, 4097):
        src = rand_vec(n + 8, dtype, 11)
        a = sa.DevVec.from_numpy(src); b = sa.DevVec.from_numpy(rand_vec(n + 8, dtype, 12))
        before = b.to_numpy()
        for off in (0, 3):
            st = L.sprs_memcpy_d2d(ctx.h, C.c_void_p(b.ptr.value + off * isz), C.c_void_p(a.ptr.value + (off + 1) * isz), n * isz)
            assert st == 0
            ctx.sync()
            got = b.to_numpy()
            assert np.array_equal(bits(got[off:off + n]), bits(src[off + 1:off + 1 + n]))
            assert np.array_equal(bits(got[off + n:]), bits(before[off + n:])) and np.array_equal(bits(got[:off]), bits(before[:off]))
            before = got
        st = L.sprs_memset_zero(ctx.h, C.c_void_p(b.ptr.value + 2 * isz), (n - 1) * isz)
        assert st == 0
        ctx.sync()
        got = b.to_numpy()
        assert not np.any(bits(got[2:2 + n - 1])) and np.array_equal(bits(got[:2]), bits(before[:2]))
        assert np.array_equal(bits(got[n + 1:]), bits(before[n + 1:]))
        a.free(); b.free()


def test_device_built_row_blocks_from_summaries(sa, oracle):
    """A matrix built in HBM (sprs_csr_create_dev_*) of >= 65536 rows is cut into row blocks from per-64-row-group
    summaries computed on the device (csrc/spmv.hip, rowblocks_from_summaries): row_ptr crosses PCIe only for the runs of
    irregular groups (a row > 96 entries, or more entries than a block holds), or as a whole when there are many.
    y must be bit-identical to the reference fold in every case, and a malformed row_ptr must be refused wherever the
    flaw sits (inside a group, across groups, at either end)."""
    import torch
    dev = torch.device("cuda", 0)
    ctx = sa.default_ctx()
    rng = np.random.default_rng(77)
    n = 200_003                                                     # last group partial
    for case in ("regular", "few-irregular", "many-irregular"):
        cnt = np.full(n, 5, dtype=np.int64)
        cnt[::1000] = 3                                             # rows of another length: blocks that are not equal-length
        if case != "regular":
            cnt[12345] = 300; cnt[12346] = 120                      # two long rows: vector blocks inside one run
            cnt[50_000:50_200] = 9                                  # 64 x 9 = 576 > 508: groups that do not fit one block
            cnt[n - 30] = 0
        if case == "many-irregular":
            cnt[(np.arange(n) // 64) % 20 == 0] = 9                 # 5 % of the groups: the whole row_ptr goes to the host
        indptr = np.zeros(n + 1, dtype=np.int64); np.cumsum(cnt, out=indptr[1:])
        nnz = int(indptr[-1])
        base = np.repeat(np.arange(n), cnt)
        k_in_row = np.arange(nnz) - np.repeat(indptr[:-1], cnt)
        indices = ((base + k_in_row * 37) % n).astype(np.int32)       # distinct columns within a row (37 k mod n, k < 300)
        data = rng.uniform(-1, 1, nnz)
        x = rng.uniform(-1, 1, n)
        ref = oracle.spmv(indptr, indices, data, x)
        ip_d = torch.from_numpy(indptr.astype(np.int32)).to(dev); ix_d = torch.from_numpy(indices).to(dev); dv_d = torch.from_numpy(data).to(dev)
        xd = torch.from_numpy(x).to(dev); yd = torch.empty_like(xd)
        for stream in (0, -1):
            ctx.set("spmv_dict", stream)
            try:
                A = sa.HipCsr.from_device((n, n), nnz, ip_d, ix_d, dv_d, adopt=True)
                A.mul_vec_unchecked(xd, yd)
            finally:
                ctx.set("spmv_dict", -1)
            y = yd.cpu().numpy()
            short = cnt <= 96
            assert np.array_equal(bits(y[short]), bits(ref[short])), (case, stream)
            assert np.all(np.abs(y[~short] - ref[~short]) <= RED_RTOL * 300)
        if case == "few-irregular":
            # The two creation paths may cut an irregular run into different row blocks (the summary path restarts blocks at
            # 64-row group boundaries): y is bit-identical all the same (the per-row fold does not depend on the block), the
            # fused dot groups its partials by block and may differ in summation order only — stated tolerance below.
            Ah = sa.HipCsr.new((n, n), indptr.astype(np.int32), indices, data)
            Ad = sa.HipCsr.from_device((n, n), nnz, ip_d, ix_d, dv_d, adopt=True)
            yh = np.empty(n); dh = Ah.mul_vec_dot(x, yh)
            dd = Ad.mul_vec_dot(xd, yd)
            assert np.array_equal(bits(yh), bits(yd.cpu().numpy()))
            assert abs(dh - dd) <= RED_RTOL * float(np.sum(np.abs(x * yh))), (dh, dd)
        if case == "regular":
            nb, ne = (ctx.set("spmv_dict", 0), sa.HipCsr.from_device((n, n), nnz, ip_d, ix_d, dv_d, adopt=True).wide_blocks())[1]
            ctx.set("spmv_dict", -1)
            assert nb == (n + 63) // 64 and 0 < ne < nb               # equal-length flags straight from the summaries
            for where, val in ((0, 1), (777, int(indptr[779]) + 1), (64 * 500, int(indptr[64 * 500 + 1]) + 5), (n, nnz + 1), (n, nnz - 1)):
                bad = indptr.astype(np.int32).copy(); bad[where] = val
                with pytest.raises(ValueError):
                    sa.HipCsr.from_device((n, n), nnz, torch.from_numpy(bad).to(dev), ix_d, dv_d, adopt=True)


def test_malformed_host_matrix_is_refused(sa):
    """A matrix whose arrays would make a kernel read outside x / val must be refused at creation with
    SPRS_INVALID_ARGUMENT — never reach a launch.  Covers the off-by-one that a page-boundary fault looks like
    (column == ncols: one element past x), negative columns, a decreasing row_ptr, row_ptr[n] != nnz — for the plain
    and for the dictionary-compressed stream (same creation path), CSR and CSC."""
    from sprsolve_amd import gen
    indptr, indices, data = gen.grid_laplacian_dirichlet(12, 12)
    n = 144

    def refused(ip, ix, dv, **kw):
        with pytest.raises(ValueError):
            sa.HipCsr.new((n, n), ip, ix, dv, **kw)
    for stream in (0, -1):
        sa.default_ctx(0).set("spmv_dict", stream)
        try:
            bad = indices.copy(); bad[len(bad) // 2] = n            # one past the end of x
            refused(indptr, bad, data)
            bad = indices.copy(); bad[0] = -1
            refused(indptr, bad, data)
            ipb = indptr.copy(); ipb[50] = ipb[51] + 2              # decreasing row_ptr
            refused(ipb, indices, data)
            ipb = indptr.copy(); ipb[-1] += 1                       # row_ptr[n] != nnz: the last row would run past val
            refused(ipb, indices, data)
            refused(indptr.astype(np.int64), np.where(np.arange(indices.size) == 7, 2**31 + 5, indices.astype(np.int64)), data)
            bad = indices.copy(); bad[5] = n
            refused(indptr, bad, data, storage="CSC")
            A = sa.HipCsr.new((n, n), indptr, indices, data)      # the well-formed one is accepted
            assert A.nnz() == int(indptr[-1])
        finally:
            sa.default_ctx(0).set("spmv_dict", -1)


def test_sampled_spmv_profile_counts(sa, oracle):
    """sprs_solver_set_profile(k): 1 = HIP events around every SpMV launch, k >= 2 = around one pair of consecutive launches in k
    (csrc/krylov.hpp profiled(): a launch that carries events costs ~6 us).  The profile says how many launches it timed, how many
    of those read a dot operand that is not their input (BiCGStab's K2: r0) and how many launches the solve had; the iterates do
    not depend on it."""
    from sprsolve_amd import gen
    ip, ix, d, rhs = gen.poisson3d(20, 17, 15)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    out = {}
    for k in (0, 1, 2, 4, 7):
        s = sa.BiCGStab.new(A, n); s.set_profile(k)
        x = np.zeros(n)
        with pytest.raises(sa.error.InsufficientIterNum):
            s.solve(rhs, x, 23, 0.0)
        out[k] = (bits(x).copy(), s.profile())
        s.set_profile(0)
    steps = 1 + 2 * 23                                  # the set-up SpMV (bicg_stab.rs:73), then K2 and K4 of every iteration
    for k in (1, 2, 4, 7):
        assert np.array_equal(out[k][0], out[0][0])
        prof = out[k][1]
        timed = [c for c in range(steps) if k == 1 or (c >> 1) % k == 0]
        assert prof["steps"] == steps and prof["spmv_launches"] == len(timed), (k, prof)
        assert prof["timed_dot_other"] == sum(1 for c in timed if c >= 1 and (c - 1) % 2 == 0)      # the K2 launches among them
        assert prof["timed_fused_k2"] == 0 and prof["timed_fused_k4"] == 0                          # (no chain plan at this size)
        assert prof["spmv_ms_total"] > 0 and prof["solve_ms"] >= prof["spmv_ms_total"]
    assert out[0][1]["spmv_launches"] == 0
    # MINRES: one SpMV per iteration, its Lanczos operand is its input
    ipb, ixb, db, rhsb = gen.symmetric_banded(3000)
    Ab = sa.HipCsr.new((3000, 3000), ipb, ixb, db)
    m = sa.MinRes.new(Ab, 3000); m.set_profile(4)
    xb = np.zeros(3000)
    with pytest.raises(sa.error.InsufficientIterNum):
        m.solve(rhsb, xb, 21, 0.0)
    prof = m.profile()
    assert prof["steps"] == 22 and prof["spmv_launches"] == len([c for c in range(22) if (c >> 1) % 4 == 0]) and prof["timed_dot_other"] == 0


def test_device_resident_solve(sa, oracle):
    """The *_solve_dev entry points: rhs / x stay in HBM."""
    from sprsolve_amd import gen
    indptr, indices, data = gen.grid_laplacian_dirichlet(64, 64)
    rhs = gen.dirichlet_rhs(64, 64)
    n = 64 * 64
    A = sa.HipCsr.new((n, n), indptr, indices, data)
    P = sa.DiagPrecond.new(np.where(np.diff(indptr) == 1, 1.0, -4.0))
    s = sa.BiCGStab.new(A, n)
    drhs = sa.DevVec.from_numpy(rhs); dx = sa.DevVec(n, np.float64); dx.zero()
    its, res = s.precond_solve(P, drhs, dx, 2000, 1e-10)
    i, j = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    assert np.max(np.abs(dx.to_numpy() - (i + j).ravel())) < 1e-6
    ref = oracle.bicgstab(indptr, indices, data, rhs, np.zeros(n), 2000, 1e-10,
                          precond_diag=np.where(np.diff(indptr) == 1, 1.0, -4.0))
    assert ref.status == oracle.OK and abs(its - ref.its) <= max(5, ref.its // 4)


# ------------------------------------------------------------------ full-size properties (BASELINE configs)
def test_cfg2_poisson2d_1m_properties(sa):
    """BASELINE cfg 2 at full size (1 M rows): size-independent properties instead of the oracle."""
    from sprsolve_amd import gen
    R = 1000
    indptr, indices, data = gen.grid_laplacian_dirichlet(R, R)
    rhs = gen.dirichlet_rhs(R, R)
    n = R * R
    assert indptr[-1] == 4984016
    A = sa.HipCsr.new((n, n), indptr, indices, data)
    exact = rhs.copy()
    i, j = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    exact = (i + j).ravel().astype(float)
    # A * (i+j) == rhs exactly: a linear function is discretely harmonic, integers are exact
    y = np.empty(n); A.mul_vec(exact, y)
    assert np.array_equal(y, rhs)
    # linearity with exactly representable scalars
    u = rand_vec(n, np.float64, 1); v = rand_vec(n, np.float64, 2)
    yu = np.empty(n); yv = np.empty(n); yuv = np.empty(n)
    A.mul_vec(u, yu); A.mul_vec(v, yv); A.mul_vec(2.0 * u, yuv)
    assert np.array_equal(yuv, 2.0 * yu)
    # Jacobi-preconditioned BiCGStab reaches the known solution
    diag = np.where(np.diff(indptr) == 1, 1.0, -4.0)
    P = sa.DiagPrecond.new(diag)
    s = sa.BiCGStab.new(A, n)
    x = np.zeros(n)
    its, res = s.precond_solve(P, rhs, x, 20000, 1e-9)
    r = np.empty(n); A.mul_vec(x, r)
    assert np.linalg.norm(r - rhs) / np.linalg.norm(rhs) < 1e-8
    assert np.max(np.abs(x - exact)) < 1e-3 * np.max(exact)


def test_cfg3_banded_minres_1m(sa):
    from sprsolve_amd import gen
    n = 1_000_000
    indptr, indices, data, rhs = gen.symmetric_banded(n)
    assert indptr[-1] == 8999980
    A = sa.HipCsr.new((n, n), indptr, indices, data)
    s = sa.MinRes.new(A, n)
    x = np.zeros(n)
    its, res = s.solve(rhs, x, 500, 1e-10)
    r = np.empty(n); A.mul_vec(x, r)
    assert np.linalg.norm(r - rhs) / np.linalg.norm(rhs) < 1e-9


def test_cfg4_complex_symmetric_500k(sa):
    from sprsolve_amd import gen
    rows, cols = 500, 1000
    indptr, indices, data, rhs, diag = gen.complex_symmetric_grid(rows, cols)
    n = rows * cols
    assert indptr[-1] == 2497000
    A = sa.HipCsr.new((n, n), indptr, indices, data)
    s = sa.CSMinRes.new(A, n)
    x = np.zeros(n, np.complex128)
    its, res = s.solve(rhs, x, 5000, 1e-10)
    assert np.max(np.abs(x - gen.grid_exact_solution(rows, cols))) < 1e-5 * max(rows, cols)
    # the reference's own pairing for this matrix: BiCGStab + complex Jacobi (test_complex_solve2.rs)
    P = sa.DiagPrecond.new(diag)
    b = sa.BiCGStab.new(A, n)
    x[:] = 0
    its, res = b.precond_solve(P, rhs, x, 5000, 1e-10)
    assert np.max(np.abs(x - gen.grid_exact_solution(rows, cols))) < 1e-5 * max(rows, cols)


# ------------------------------------------------------------------ f32 / Complex<f32>
def test_f32_solvers_against_oracle(sa, oracle):
    """The reference is generic over cauchy::Scalar; its f32/c32 unit tests are BLAS-1 only, so the
    solver path in single precision is checked against the oracle's f32 instantiation."""
    from sprsolve_amd import gen
    indptr, indices, data = gen.grid_laplacian_dirichlet(20, 20)
    rhs = gen.dirichlet_rhs(20, 20).astype(np.float32)
    data = data.astype(np.float32)
    n = 400
    A = sa.HipCsr.new((n, n), indptr, indices, data)
    s = sa.BiCGStab.new(A, n); s.set_trace(4)
    x = np.zeros(n, np.float32)
    its, res = s.solve(rhs, x, 500, 1e-5)
    ref = oracle.bicgstab(indptr, indices, data, rhs, np.zeros(n, np.float32), 500, 1e-5, trace_cap=4)
    assert ref.status == oracle.OK and ref.x.dtype == np.float32
    i, j = np.meshgrid(np.arange(20), np.arange(20), indexing="ij")
    exact = (i + j).ravel()
    assert np.max(np.abs(x - exact)) < 2e-3 and np.max(np.abs(ref.x - exact)) < 2e-3
    assert np.allclose(s.trace()[0], ref.trace[0], rtol=1e-5)          # unrolled iteration, f32 rounding
    assert isinstance(res, float) and res <= 1e-5
    # Jacobi in f32 and the literal mode
    P = sa.DiagPrecond.new(np.where(np.diff(indptr) == 1, 1.0, -4.0).astype(np.float32))
    s.set_mode("literal"); x[:] = 0
    its, res = s.precond_solve(P, rhs, x, 500, 1e-5)
    assert np.max(np.abs(x - exact)) < 2e-3
    # c32: MINRES on the Hermitian grid of tests/test_complex_solve.rs, real f32 Jacobi
    ip, ix, d, b, dg = gen.complex_hermitian_grid(8, 8)
    d = d.astype(np.complex64); b = b.astype(np.complex64)
    Az = sa.HipCsr.new((64, 64), ip, ix, d)
    m = sa.MinRes.new(Az, 64)
    xz = np.zeros(64, np.complex64)
    its, res = m.solve(b, xz, 300, 1e-5)
    refz = oracle.minres(ip, ix, d, b, np.zeros(64, np.complex64), 300, 1e-5)
    assert refz.status == oracle.OK and abs(its - refz.its) <= 5
    assert np.max(np.abs(xz - gen.grid_exact_solution(8, 8))) < 5e-3
    Pz = sa.DiagPrecond.new(dg.astype(np.float32), t_dtype=np.complex64)      # DiagPrecond<Complex32, f32>
    xz[:] = 0
    its, res = m.precond_solve(Pz, b, xz, 300, 1e-5)
    assert np.max(np.abs(xz - gen.grid_exact_solution(8, 8))) < 5e-3
    # c32 CSMINRES on the complex-symmetric grid
    ip, ix, d, b, dg = gen.complex_symmetric_grid(8, 8)
    Ac = sa.HipCsr.new((64, 64), ip, ix, d.astype(np.complex64))
    cs = sa.CSMinRes.new(Ac, 64)
    xz[:] = 0
    its, res = cs.solve(b.astype(np.complex64), xz, 500, 1e-5)
    assert np.max(np.abs(xz - gen.grid_exact_solution(8, 8))) < 5e-3


def test_f32_jacobi_and_mul_vec_dot(sa, oracle):
    n = 3001
    d = (rand_vec(n, np.float32, 1) + 2).astype(np.float32)
    v = rand_vec(n, np.complex64, 2)
    P = sa.DiagPrecond.new(d, t_dtype=np.complex64)
    out = np.empty(n, np.complex64); P.mul_vec(v, out)
    assert np.array_equal(bits(out), bits(oracle.diag_apply(oracle.diag_inv(d), v)))
    dz = (rand_vec(n, np.complex64, 3) + 2).astype(np.complex64)
    Pz = sa.DiagPrecond.new(dz); Pz.mul_vec(v, out)
    assert np.array_equal(bits(out), bits(oracle.diag_apply(oracle.diag_inv(dz), v)))
    with pytest.raises(TypeError):
        sa.DiagPrecond.new(d, t_dtype=np.complex128)       # T: Mul<V> needs matching precision


def test_cfg5_poisson3d_50m_properties(sa):
    """BASELINE cfg 5 at full size (50 M rows, 349.1 M nnz), built in HBM: exact identities and the
    known solution (the oracle is far too slow here; size-independent properties instead)."""
    import torch
    from sprsolve_amd import gen_torch
    dev = torch.device("cuda", 0)
    nx, ny, nz = 500, 500, 200
    ip, ix, dv, rhs = gen_torch.poisson3d(nx, ny, nz, device=dev)
    n = nx * ny * nz
    nnz = int(ip[-1].item())
    assert nnz == 349_100_000
    A = sa.HipCsr.from_device((n, n), nnz, ip, ix, dv, adopt=True)
    ones = torch.ones(n, dtype=torch.float64, device=dev)
    y = torch.empty_like(ones)
    A.mul_vec_unchecked(ones, y)
    assert torch.equal(y, rhs)                                # A*1 = row sums, small integers: exact
    # linearity with an exactly representable scale, and symmetry: u.(A v) == v.(A u) to rounding
    u = torch.rand(n, dtype=torch.float64, device=dev) - 0.5
    v = torch.rand(n, dtype=torch.float64, device=dev) - 0.5
    Au = torch.empty_like(u); Av = torch.empty_like(u); A4u = torch.empty_like(u)
    A.mul_vec_unchecked(u, Au); A.mul_vec_unchecked(v, Av); A.mul_vec_unchecked(4.0 * u, A4u)
    assert torch.equal(A4u, 4.0 * Au)
    d1 = sa.vecalg.dot(v, Au); d2 = sa.vecalg.dot(u, Av)
    assert abs(d1 - d2) <= 1e-10 * float(Au.abs().sum().item()) * 0.5
    # mul_vec_dot == conj_dot(x, A x)
    d = A.mul_vec_dot_unchecked(u, y)
    assert abs(d - sa.vecalg.conj_dot(u, Au)) <= 1e-12 * float((u.abs() * Au.abs()).sum().item())
    # BiCGStab reaches the known solution (all ones)
    s = sa.BiCGStab.new(A, n)
    x = torch.zeros(n, dtype=torch.float64, device=dev)
    its, res = s.solve(rhs, x, 5000, 1e-8)
    assert res <= 1e-8 and float((x - 1.0).abs().max().item()) < 1e-4
    A.mul_vec_unchecked(x, y)
    assert float(torch.linalg.vector_norm(y - rhs) / torch.linalg.vector_norm(rhs)) < 2e-8


@pytest.mark.parametrize("values", ["poisson", "random"])
def test_cfg5_full_size_spmv_against_oracle(sa, oracle, values):
    """BASELINE cfg 5 at FULL size (500x500x200: 50 M rows, 349.1 M nnz), both value sets — the constant-coefficient operator
    (pair codes: uniform / seam blocks, column triples, XCD-period walk, 32-bit byte offsets) and U(-1,1) coefficients
    ("identical random CSR inputs": offset codes, uniform 64-row blocks) — one SpMV per stream, y compared BIT FOR BIT with the
    oracle's fold (mat.rs:100-105; its row-parallel path, mat.rs:85-107, whose rows are folded exactly like the serial
    ones) and the streams with each other; the fused mul_vec_dot within 1e-13 * sum|terms| of conj_dot(x, A x)."""
    import torch
    from sprsolve_amd import gen_torch
    dev = torch.device("cuda", 0)
    nx, ny, nz = 500, 500, 200
    n = nx * ny * nz
    ip, ix, dv, _ = gen_torch.poisson3d(nx, ny, nz, device=dev, values=values)
    nnz = int(ip[-1].item())
    assert nnz == 349_100_000
    torch.manual_seed(5)
    x = torch.rand(n, dtype=torch.float64, device=dev) * 2.0 - 1.0
    ctx = sa.default_ctx(0)
    ctx.set("spmv_dict", -1)
    A = sa.HipCsr.from_device((n, n), nnz, ip, ix, dv, adopt=True)
    mode = A.stream_format()[0]
    assert mode == (2 if values == "poisson" else 1), mode          # the stream bench.py times for this value set
    y = torch.empty_like(x); y0 = torch.empty_like(x)
    try:
        A.mul_vec_unchecked(x, y)                                    # the compressed stream
        d_fused = A.mul_vec_dot_unchecked(x, y0)
        assert torch.equal(y.view(torch.int64), y0.view(torch.int64))
        ctx.set("spmv_dict", 0)
        assert A.stream_format()[0] == 0
        A.mul_vec_unchecked(x, y0)                                   # the plain (col_idx, val) stream of the same handle
        d_plain = A.mul_vec_dot_unchecked(x, y0)
    finally:
        ctx.set("spmv_dict", -1)
    assert torch.equal(y.view(torch.int64), y0.view(torch.int64)), "the compressed and the plain stream disagree"
    xh = x.cpu().numpy(); yh = y.cpu().numpy()
    iph, ixh, dvh = ip.cpu().numpy(), ix.cpu().numpy(), dv.cpu().numpy()
    del A, y0, x, y, ip, ix, dv
    torch.cuda.empty_cache()
    oracle.set_threads(min(16, oracle.max_threads()))
    ref = oracle.spmv(iph, ixh, dvh, xh, parallel=True)
    assert np.array_equal(yh.view(np.uint64), ref.view(np.uint64)), \
        "%d of %d rows differ from the reference fold" % (int(np.count_nonzero(yh.view(np.uint64) != ref.view(np.uint64))), n)
    terms = float(np.abs(xh * ref).sum())
    exact = float(np.dot(xh, ref))
    assert abs(d_fused - exact) <= 1e-13 * terms and abs(d_plain - exact) <= 1e-13 * terms, (d_fused, d_plain, exact, terms)


@pytest.mark.parametrize("dtype", ALL_DTYPES, ids=ALL_IDS)
def test_spmv_row_length_boundaries(sa, oracle, dtype):
    """Row lengths around every threshold of the kernel: 0, 1, 8/9 (register fast path), 96/97
    (stream vs wavefront-per-row), 320/321 and 512/513 (LDS slice capacities), plus a 5000-nnz row."""
    rng = np.random.default_rng(11)
    lens = [0, 1, 8, 9, 7, 96, 97, 95, 320, 321, 64, 512, 513, 2, 5000, 3, 96, 96, 96, 96, 96, 96, 0, 0, 5]
    n = 6000
    cnt = np.array(lens * 3, dtype=np.int64)
    m = cnt.size
    indptr = np.zeros(m + 1, dtype=np.int64); np.cumsum(cnt, out=indptr[1:])
    indices = np.concatenate([np.sort(rng.choice(n, c, replace=False)) for c in cnt]).astype(np.int32)
    data = rand_vec(int(indptr[-1]), dtype, 5)
    x = rand_vec(n, dtype, 6)
    A = sa.HipCsr.new((m, n), indptr.astype(np.int32), indices, data)
    y = np.empty(n, dtype=dtype)                      # checked mul_vec wants len(y) == len(x) == cols
    A.mul_vec(x, y)
    ref = oracle.spmv(indptr, indices, data, x)
    short = cnt <= 96
    assert np.array_equal(bits(y[:m][short]), bits(ref[short]))
    tol = RED_RTOL_F32 if is_single(dtype) else RED_RTOL
    absA = oracle.spmv(indptr, indices, np.abs(data).astype(dtype), np.abs(x).astype(dtype))
    assert np.all(np.abs(y[:m][~short] - ref[~short]) <= tol * np.abs(absA[~short]))


def test_c_program_through_the_abi(tmp_path):
    """examples/c_abi_demo.c: a plain C host builds the reference's bench matrix, solves it through the C ABI alone
    (no Python, no torch in the process) and checks the known solution i + j."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "c_abi_demo")
    libdir = os.path.join(root, "sprsolve_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "examples", "c_abi_demo.c"), "-o", exe, "-L", libdir, "-l:libsprsolve_hip.so",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"])
    out = subprocess.run([exe, "96"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "stream=2" in out.stdout and "max_err=" in out.stdout, out.stdout


def test_host_owned_recurrence_through_the_abi(tmp_path):
    """examples/host_loop_bicgstab.c — north_star's literal structure: a C host owns the BiCGStab recurrence
    (bicg_stab.rs:35-200 statement for statement) and calls one kernel per reference op through the C ABI, vectors
    resident in HBM.  Its iteration count, residual and x must be bit-identical to the library's own literal-mode solve
    (same kernels, same order) and agree with the fused default to rounding."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "host_loop")
    libdir = os.path.join(root, "sprsolve_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "examples", "host_loop_bicgstab.c"), "-o", exe, "-L", libdir, "-l:libsprsolve_hip.so",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"])
    for size in ("48", "100"):
        out = subprocess.run([exe, size], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "bit-identical: yes" in out.stdout, out.stdout


def test_non_temporal_accesses_are_a_pure_cache_hint(oracle):
    """Knob stream_nt: at HBM sizes the fused recurrence kernels read and write their vectors, and the pair-code SpMV
    writes y, with non-temporal accesses (automatic from 72 MB per vector; forced here on small systems so that those
    kernel instantiations run in the suite).  Same values, same order: iteration counts, residuals, x and y are
    bit-identical with the hint on and off — BiCGStab plain and Jacobi, MINRES, CSMINRES."""
    import sprsolve_amd as sa
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint8)
    ip, ix, d, rhs = gen.poisson3d(150, 12, 9)
    n = rhs.size
    sp, sx, sd, srhs = gen.symmetric_banded(20011, hbw=4)
    cp_, cx_, cd_c, crhs, _ = gen.complex_symmetric_grid(40, 60)   # tests/test_complex_solve2.rs:35-96
    nc = crhs.size
    out = {}
    try:
        for nt in (0, 1):
            ctx.set("stream_nt", nt)
            A = sa.HipCsr.new((n, n), ip, ix, d)
            xin = np.linspace(-1.0, 1.0, n) ** 3
            y = np.zeros(n); dot = A.mul_vec_dot(xin, y)
            s = sa.BiCGStab.new(A, n); x1 = np.zeros(n); r1 = s.solve(rhs, x1, 3000, 1e-10)
            P = sa.DiagPrecond.new(np.full(n, 6.0)); x2 = np.zeros(n); r2 = s.precond_solve(P, rhs, x2, 3000, 1e-10)
            B = sa.HipCsr.new((20011, 20011), sp, sx, sd)
            m = sa.MinRes.new(B, 20011); x3 = np.zeros(20011); r3 = m.solve(srhs, x3, 3000, 1e-10)
            Cm = sa.HipCsr.new((nc, nc), cp_, cx_, cd_c)
            cs = sa.CSMinRes.new(Cm, nc); x4 = np.zeros(nc, dtype=np.complex128); r4 = cs.solve(crhs, x4, 5000, 1e-9)
            out[nt] = (dot, y, r1, x1, r2, x2, r3, x3, r4, x4)
    finally:
        ctx.set("stream_nt", -1)
    a, b = out[0], out[1]
    assert a[0] == b[0] and a[2] == b[2] and a[4] == b[4] and a[6] == b[6] and a[8] == b[8]
    for k in (1, 3, 5, 7, 9):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert np.array_equal(bits(a[1]), bits(oracle.spmv(ip, ix, d, np.linspace(-1.0, 1.0, n) ** 3)))


def test_minres_converging_launch_finishes_its_own_iteration(sa, oracle):
    """MINRES tests convergence AFTER updating x (minres.rs:162-167), so the kernel that finds the solve converged also holds
    that iteration's x update: a workgroup of that launch which reads the status word late must not take the event its own
    launch set for a reason to skip its tiles.  (The solver fuzz met it once in ~10^5 solves: its / residual right, x updated
    in some tiles only.)  The status word now carries the iteration; this hammers the case — thousands of solves that converge in
    their first iterations, small enough that workgroup 0 is done within microseconds — and compares every x with the oracle."""
    from sprsolve_amd import gen
    rng = np.random.default_rng(99)
    for n, dtype in ((1000, np.complex128), (4099, np.float64), (257, np.complex128)):
        ip, ix, d, _ = gen.symmetric_banded(n, hbw=3)
        d = d.astype(dtype)
        A = sa.HipCsr.new((n, n), ip, ix, d)
        s = sa.MinRes.new(A, n)
        for k in range(400):
            rhs = rng.uniform(-1, 1, n).astype(dtype)
            if np.dtype(dtype).kind == "c":
                rhs = rhs + 1j * rng.uniform(-1, 1, n)
            tol = (0.5, 0.3, 0.1)[k % 3]
            ref = oracle.minres(ip, ix, d, rhs, np.zeros(n, dtype=dtype), 50, tol)
            x = np.zeros(n, dtype=dtype)
            its, res = s.solve(rhs, x, 50, tol)
            assert its == ref.its and np.max(np.abs(x - ref.x)) <= 1e-12 * max(1.0, float(np.max(np.abs(ref.x)))), (n, k, its, ref.its)
