"""Pins the CPU oracle (oracle/sprs_oracle.c) against every known-answer test the reference
holds for the hot path.  CPU only."""
import numpy as np
import pytest

import _golden as G


@pytest.mark.parametrize("case", G.load("spmv_kat.json")["cases"], ids=lambda c: c["name"])
def test_spmv_kat(oracle, case):
    indptr, indices, data, x, exp = G.spmv_case(case)
    if case["storage"] == "CSC":
        y = oracle.spmv_csc(case["shape"][0], indptr, indices, data, x)
    else:
        y = oracle.spmv(indptr, indices, data, x)
        yp = oracle.spmv(indptr, indices, data, x, parallel=True)
        assert np.array_equal(y.view(np.float64), yp.view(np.float64)), "row-parallel bits differ from serial"
    assert np.all(np.abs(y - exp) < case["eps"] * (np.sqrt(2) if case.get("complex") else 1))
    if case.get("complex"):
        assert np.all(np.abs(y.real - exp.real) < case["eps"]) and np.all(np.abs(y.imag - exp.imag) < case["eps"])


def test_mul_vec_dot_kat(oracle):
    """src/mkl_mat.rs:432-463: mul_vec_dot(x, y) == conj_dot(x, A x)."""
    spec = G.load("spmv_kat.json")
    case = [c for c in spec["cases"] if c["name"] == spec["mul_vec_dot"]["case"]][0]
    indptr, indices, data, x, exp = G.spmv_case(case)
    y, d = oracle.spmv_dot(indptr, indices, data, x)
    assert np.all(np.abs(y - exp) < 2e-8)
    e = oracle.conj_dot(x, y)
    assert d == e
    assert abs(d - np.vdot(x, y)) < 1e-14


def _run_vecalg(orc, case):
    dt = case["dtype"]
    op = case["op"]
    x = G.vec(case["x"], dt)
    if op == "norm2":
        return orc.norm2(x)
    if op in ("dot", "conj_dot"):
        return getattr(orc, op)(x, G.vec(case["y"], dt))
    if op == "scale":
        return orc.scale(G.scalar(case["a"], dt), x)
    if op == "rscale":
        return orc.rscale(case["a"], x)
    if op == "conj":
        return orc.conj(x)
    if op == "axpy":
        y = G.vec(case["y"], dt)
        a = float(case["a_real"]) if "a_real" in case else G.scalar(case["a"], dt)
        return orc.axpy(a, x, y)
    if op == "axpy_repeat":
        y = G.vec(case["y"], dt)
        for _ in range(case["repeat"]):
            orc.axpy(G.scalar(case["a"], dt), x, y)
        return y
    raise KeyError(op)


@pytest.mark.parametrize("case", G.load("vecalg_kat.json")["cases"], ids=lambda c: c["name"])
def test_vecalg_kat(oracle, case):
    dt = case["dtype"]
    eps = case.get("eps", 1e-13)
    if case["op"] == "axpby_sequence":
        x = G.vec(case["x"], dt); y = G.vec(case["y"], dt)
        for st in case["steps"]:
            for _ in range(st["repeat"]):
                oracle.axpby(G.scalar(st["a"], dt), x, G.scalar(st["b"], dt), y)
            assert np.all(np.abs(y - st["expected_fill"]) <= eps)
        return
    got = _run_vecalg(oracle, case)
    if "expected" in case:
        assert abs(got - G.scalar(case["expected"], dt)) <= eps
    elif "expected_fill" in case:
        assert np.all(np.abs(got - G.scalar(case["expected_fill"], dt)) <= eps)
    else:
        exp = G.vec({"array": case["expected_array"]}, dt)
        assert np.all(np.abs(got - exp) <= eps)


@pytest.mark.parametrize("case", G.load("solver_kat.json")["cases"], ids=lambda c: c["name"])
def test_solver_kat(oracle, case):
    """The reference asserts only Ok; we additionally assert the exact solution its
    construction implies."""
    p = G.solver_problem(case)
    fn = getattr(oracle, case["solver"])
    x0 = np.zeros_like(p["rhs"])
    r = fn(p["indptr"], p["indices"], p["data"], p["rhs"], x0, case["max_iter"], case["tol"],
           precond_diag=p["diag"])
    assert r.status == oracle.OK, r
    err = np.max(np.abs(r.x - p["exact"]))
    scale = max(1.0, np.max(np.abs(p["exact"])))
    assert err / scale < 1e-9, (r, err)
    # true residual
    res = np.linalg.norm(oracle.spmv(p["indptr"], p["indices"], p["data"], r.x) - p["rhs"]) / np.linalg.norm(p["rhs"])
    assert res < 1e-10, res


@pytest.mark.parametrize("name", ["test_minres", "minres_ident"])
def test_csminres_is_minres_for_real_scalars(oracle, name):
    """CSMinRes has no test in the reference (tests/test_minres.rs:14-15 are commented out).  For REAL T `conj` is the
    identity, so cs_minres.rs:90-154 is arithmetically minres.rs:90-169 — same Lanczos products in the same order,
    same Givens formulas.  The oracle's two restatements must therefore agree BIT FOR BIT on the reference's own two
    MINRES problems (tests/test_minres.rs:1-60): that ties the Saunders code path to reference-held fixtures.  The
    complex-symmetric branch (conjugations live) stays "parity unpinned"."""
    case = [c for c in G.load("solver_kat.json")["cases"] if c["name"] == name][0]
    p = G.solver_problem(case)
    K = 40
    a = oracle.minres(p["indptr"], p["indices"], p["data"], p["rhs"], np.zeros_like(p["rhs"]), K, 0.0, trace_cap=K)
    b = oracle.csminres(p["indptr"], p["indices"], p["data"], p["rhs"], np.zeros_like(p["rhs"]), K, 0.0, trace_cap=K)
    assert a.status == b.status and a.its == b.its
    assert a.trace.shape == b.trace.shape and a.trace.shape[0] > 0
    assert np.array_equal(a.trace.view(np.uint64), b.trace.view(np.uint64))
    assert np.array_equal(a.x.view(np.uint64), b.x.view(np.uint64))
    # and to convergence with the reference's own tolerance
    a = oracle.minres(p["indptr"], p["indices"], p["data"], p["rhs"], np.zeros_like(p["rhs"]), case["max_iter"], case["tol"])
    b = oracle.csminres(p["indptr"], p["indices"], p["data"], p["rhs"], np.zeros_like(p["rhs"]), case["max_iter"], case["tol"])
    assert (a.status, a.its, a.res) == (b.status, b.its, b.res) and a.status == oracle.OK
    assert np.array_equal(a.x.view(np.uint64), b.x.view(np.uint64))


def test_gpu_order_reductions_are_a_reordering_only(oracle):
    """oracle/krylov_tmpl.h, "reductions as the SOLVERS call them": mode "gpu" adds the SAME terms in the order of the
    library's reduction kernels.  On the CPU this can only be checked as a reordering: sums of exactly representable
    terms are identical in any order; generic sums agree to rounding; one term or one workgroup's worth of terms folds
    exactly as the serial loop does for the first lane; the solvers reach the same solutions; the default is the
    reference's serial fold.  (Bit-for-bit equality with the GPU is tests/test_gpu_parity.py's business.)"""
    rng = np.random.default_rng(3)
    for dt in (np.float64, np.complex128, np.float32, np.complex64):
        for n in (1, 2, 255, 256, 257, 4099, 131075, 300001):
            x = rng.integers(-8, 9, n).astype(dt); y = rng.integers(-8, 9, n).astype(dt)
            if np.dtype(dt).kind == "c":
                x = x + 1j * rng.integers(-8, 9, n).astype(dt); y = y - 1j * rng.integers(-8, 9, n).astype(dt)
            assert oracle.conj_dot_gpu_order(x, y) == oracle.conj_dot(x, y), (dt, n)        # small integers: exact in any order
            assert oracle.norm2_gpu_order(x) == oracle.norm2(x)
            xr = rng.uniform(-1, 1, n).astype(dt); yr = rng.uniform(-1, 1, n).astype(dt)
            tol = (2e-4 if np.dtype(dt).itemsize in (4, 8) and np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else 1e-12) * max(1.0, float(np.sum(np.abs(xr * yr))))
            assert abs(oracle.conj_dot_gpu_order(xr, yr) - oracle.conj_dot(xr, yr)) <= tol
    # the solvers: same solution either way, and the mode is off unless asked for
    case = [c for c in G.load("solver_kat.json")["cases"] if c["name"] == "bench_laplacian_100"][0]
    p = G.solver_problem(case)
    a = oracle.bicgstab(p["indptr"], p["indices"], p["data"], p["rhs"], np.zeros_like(p["rhs"]), case["max_iter"], case["tol"], trace_cap=4)
    oracle.set_reduction_order("gpu", 512)
    try:
        b = oracle.bicgstab(p["indptr"], p["indices"], p["data"], p["rhs"], np.zeros_like(p["rhs"]), case["max_iter"], case["tol"], trace_cap=4)
    finally:
        oracle.set_reduction_order("reference")
    c = oracle.bicgstab(p["indptr"], p["indices"], p["data"], p["rhs"], np.zeros_like(p["rhs"]), case["max_iter"], case["tol"], trace_cap=4)
    assert a.status == b.status == oracle.OK and np.max(np.abs(a.x - b.x)) < 1e-9 and np.max(np.abs(b.x - p["exact"])) < 1e-9
    assert np.allclose(a.trace[0], b.trace[0], rtol=1e-12) and not np.array_equal(a.trace, b.trace)      # different order, same numbers
    assert np.array_equal(a.trace, c.trace) and np.array_equal(a.x, c.x) and a.its == c.its               # the default is untouched


# ------------------------------------------------------------------ special values: the oracle's side (tests/_special.py)
def _special_matrices(dtype):
    """A small 3-D Poisson matrix (lines of 9 rows) and a ragged random one (empty rows, rows longer than a wavefront, more columns
    than rows), each with one column no row references."""
    import _special as S
    from sprsolve_amd import gen
    ip, ix, d, _ = gen.poisson3d(9, 7, 5)
    d = d.astype(dtype)
    if np.dtype(dtype).kind == "c":
        d = d * (1 - 0.5j)
    n = ip.size - 1
    out = {"poisson3d": S.drop_column(ip, ix, d, n // 3) + (n, n, 9, n // 3)}
    ip, ix, d = S.ragged_csr(700, 31, dtype, ncols=760)
    out["ragged"] = S.drop_column(ip, ix, d, 333) + (700, 760, None, 333)
    return out


@pytest.mark.parametrize("name", ["poisson3d", "ragged"])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128, np.float32, np.complex64], ids=["f64", "c64", "f32", "c32"])
def test_oracle_spmv_depends_on_exactly_the_stored_columns(oracle, dtype, name):
    """The property tests/test_gpu_special_values.py holds every SpMV route to, on the reference side alone: y[i] depends on x[j] if
    and only if row i stores column j.  With x[S] = NaN / +Inf / -Inf (complex: either part, both) rows that store no column of S
    keep the bits of A x0 — the oracle's fold touches stored entries only; the share of (matrix, poison set) combinations where it
    does not must be zero, so every one is asserted — and the touched rows equal an independent numpy restatement of the fold (NaN
    by mask, bits elsewhere)."""
    import _special as S
    ip, ix, d, nrows, ncols, nx, free_col = _special_matrices(dtype)[name]
    x0 = S.rand_vec(ncols, dtype, 3)
    spmv = lambda x: oracle.spmv(ip, ix, d, x)
    ref = lambda x: S.fold_spmv(ip, ix, d, x)
    y0 = spmv(x0)
    S.assert_same_special(y0, ref(x0), "clean x")
    rng = np.random.default_rng(17)
    sets = [("random%d" % k, S.random_poison_set(rng, ip, ix, ncols), "random") for k in range(3)]
    sets += [(k, v, "structural") for k, v in S.structural_sets(ip, ix, nrows, ncols, nx).items()]
    sets.append(("unreferenced", np.array([free_col]), "unreferenced"))
    assert {"first", "last", "triple", "last_column"} <= {s[0] for s in sets}
    for sname, cols, kind in sets:
        for vname, value in S.poison_values(dtype):
            _, y, touched = S.check_poison(spmv, ref, ip, ix, ncols, x0, y0, cols, value, kind, label="%s/%s/%s" % (name, sname, vname))
            if kind != "unreferenced" and value[1] != value[1]:
                assert np.isnan(S.components(y[touched])).any()            # (the poison arrives where it should)


@pytest.mark.parametrize("name", ["poisson3d", "ragged"])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128, np.float32, np.complex64], ids=["f64", "c64", "f32", "c32"])
def test_oracle_spmv_signed_zero_subnormal_overflow(oracle, dtype, name):
    """The fold starts from +0.0 (oracle/krylov_tmpl.h): a row whose products are all -0.0 gives +0.0; subnormal products are kept,
    not flushed; a partial sum that overflows stays +-Inf and +Inf meeting -Inf is NaN; complex products follow (ac - bd) + (ad + bc) i
    through Inf and NaN.  The oracle against the independent numpy fold on every value variant of tests/_special.py."""
    import _special as S
    ip, ix, d, nrows, ncols, nx, free_col = _special_matrices(dtype)[name]
    seen = set()
    for vname, vals, x in S.special_variants(d, dtype, ncols, 5):
        y = oracle.spmv(ip, ix, vals, x)
        S.assert_same_special(y, S.fold_spmv(ip, ix, vals, x), "%s/%s" % (name, vname))
        yc = S.components(y)
        if vname in ("zeros_values_neg0_x", "neg0_x"):
            assert not np.signbit(yc).any() and not yc.any(), vname            # sums of -0.0 products on top of +0.0: +0.0
        if vname == "subnormal":
            tiny = np.finfo(yc.dtype).tiny
            assert ((yc != 0) & (np.abs(yc) < tiny)).any() and (np.abs(yc) == np.finfo(yc.dtype).smallest_subnormal).any()
        if vname == "overflow":
            assert np.isinf(yc).any() and np.isnan(yc).any() and np.isfinite(yc).any()
        if vname == "complex_inf":
            assert np.isnan(yc).any() and np.isfinite(yc).any()
        seen.add(vname)
    assert {"zeros_values", "neg0_x", "subnormal", "overflow"} <= seen


def test_special_helpers_catch_a_multiply_by_zero_and_a_seeded_accumulator():
    """The two assertion classes can fail: an SpMV that MULTIPLIES its padded slots by zero instead of selecting them away is
    bit-identical on finite data and goes red in the poison check (0 * NaN, 0 * Inf); one that seeds its accumulator with the first
    product goes red on the all -0.0 input (-0.0 where the reference gives +0.0).  assert_same_special itself: NaN by mask whatever
    its sign and payload, everything else by bits (+0.0 is not -0.0, +Inf is not -Inf)."""
    import _special as S
    ip, ix, d = S.ragged_csr(120, 7, np.float64, long_rows=False)
    ip, ix, d = S.drop_column(ip, ix, d, 40)
    n = 120
    x0 = S.rand_vec(n, np.float64, 1)
    good = lambda x: S.fold_spmv(ip, ix, d, x)
    wrong = lambda x: S.padded_spmv_multiplying_by_zero(ip, ix, d, x)
    lens = np.diff(ip)
    y0 = good(x0)
    assert np.array_equal(S.bits(wrong(x0)[lens > 0]), S.bits(y0[lens > 0]))          # finite data cannot tell them apart
    rng = np.random.default_rng(2)
    cols = S.random_poison_set(rng, ip, ix, n)
    for vname, value in S.poison_values(np.float64):
        S.check_poison(good, good, ip, ix, n, x0, y0, cols, value, "random", label=vname)
        with pytest.raises(AssertionError, match="untouched rows"):
            S.check_poison(wrong, good, ip, ix, n, x0, wrong(x0), cols, value, "random", label=vname)
    with pytest.raises(AssertionError):                                                  # a vacuous poison set is refused
        S.check_poison(good, good, ip, ix, n, x0, y0, np.array([40]), ("re", np.nan), "random")
    S.check_poison(good, good, ip, ix, n, x0, y0, np.array([40]), ("re", np.nan), "unreferenced")
    neg0 = np.full(n, -0.0)
    seeded = S.first_product_seeded_spmv(ip, ix, np.abs(d), neg0)
    S.assert_same_special(good(neg0), np.zeros(n))
    with pytest.raises(AssertionError, match="bits differ"):
        S.assert_same_special(seeded, good(neg0), "seeded accumulator")
    a = np.array([np.nan, 1.0, -0.0, np.inf])
    b = np.array([-np.nan, 1.0, -0.0, np.inf])
    b.view(np.uint64)[0] |= 0x1234                                                       # another payload, the other sign
    S.assert_same_special(a, b)
    for k, v in ((1, np.nan), (2, 0.0), (3, -np.inf), (0, 1.0)):
        c = b.copy(); c[k] = v
        with pytest.raises(AssertionError):
            S.assert_same_special(c, a)
    z = np.array([1 + 2j, np.nan + 1j], dtype=np.complex64)
    S.assert_same_special(z, z.copy())
    with pytest.raises(AssertionError):
        S.assert_same_special(np.array([1 + 2j, 1 + np.nan * 1j], dtype=np.complex64), z)
