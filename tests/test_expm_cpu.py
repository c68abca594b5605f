"""The Krylov propagator w = exp(tA) v without a GPU: the C ABI and the Python mirror exist, and the numpy checker of the GPU
tests (tests/_expm_ref.py) is checked independently of the library — its result against scipy.linalg.expm of the dense matrix,
its small exponential against scipy.linalg.expm on the projected matrices of the runs and on scaled random Hessenberg matrices,
its round2, its happy-breakdown rule on a diagonal matrix with five distinct entries, a finite input that reaches the tenth
rejection — and the sub-step, rejection and product counts the GPU tests quote are recorded here."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _expm_ref as ref  # noqa: E402

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
EPS64 = float(np.finfo(np.float64).eps)
NAMES = sorted(["sprs_expm_%s_%s" % (f, s) for f in ("create", "apply", "apply_dev") for s in "dzsc"] + ["sprs_expm_destroy"])

# (matrix, dtype, t, ncv, tau0, tol) -> (sub-steps, rejections, products) of the checker on the tests' start vector; tau0 = 0: chosen
# by the recurrence, tol = 0: sqrt(eps).  An oversized tau0 is the deterministic way into the reject loop: one such case per scalar
# type at least.  test_counts_and_truth holds them.
COUNTS = {
    ("cd9x8", "float64", 0.5, 10, 0.0, 0.0): (3, 0, 33),
    ("cd9x8", "float32", 0.5, 10, 0.0, 0.0): (2, 0, 22),
    ("cd9x8", "complex128", 0.5, 10, 0.0, 0.0): (3, 0, 33),
    ("cd9x8", "complex64", 0.5, 10, 0.0, 0.0): (2, 0, 22),
    ("heat12x11x10", "float64", 0.5, 10, 0.0, 0.0): (4, 0, 44),
    ("heat12x11x10", "float32", 0.5, 10, 0.0, 0.0): (2, 0, 22),
    ("schro700", "complex128", 0.5, 10, 0.0, 0.0): (4, 0, 44),
    ("schro700", "complex64", 0.5, 10, 0.0, 0.0): (2, 0, 22),
    ("schro700", "complex128", -0.25, 12, 0.0, 0.0): (2, 0, 26),
    ("schro700", "complex64", -0.25, 12, 0.0, 0.0): (2, 0, 26),
    ("cd40x33", "float64", 2.0, 10, 2.0, 0.0): (7, 2, 77),
    ("cd40x33", "float32", 2.0, 10, 2.0, 0.0): (3, 2, 33),
    ("heat12x11x10", "float64", 1.0, 12, 1.0, 0.0): (3, 1, 39),
    ("heat12x11x10", "float32", 1.0, 12, 1.0, 0.0): (2, 1, 26),
    ("schro700", "complex128", 1.0, 12, 1.0, 0.0): (4, 1, 52),
    ("schro700", "complex64", 1.0, 12, 1.0, 0.0): (2, 1, 26),
    ("cd9x8", "float64", 40.0, 8, 0.0, 1e-10): (37, 1, 333),
    ("diag5", "float64", 1.5, 12, 0.0, 0.0): (1, 0, 5),
    ("diag5", "float32", 1.5, 12, 0.0, 0.0): (1, 0, 5),
    ("diag5", "complex128", 1.5, 12, 0.0, 0.0): (1, 0, 5),
    ("diag5", "complex64", 1.5, 12, 0.0, 0.0): (1, 0, 5),
    # the ends of ncv: 3, and 48 (the full footprint of the small exponential)
    ("cd9x8", "float64", 0.05, 3, 0.0, 0.0): (47, 0, 188),
    ("cd9x8", "complex64", 0.05, 3, 0.0, 0.0): (3, 0, 12),
    ("cd40x33", "float64", 8.0, 48, 0.0, 0.0): (3, 0, 147),
    ("cd40x33", "complex64", 8.0, 48, 0.0, 0.0): (2, 0, 98),
}
CASES = list(COUNTS)
_id = lambda c: "%s-%s-t%g-m%d-tau%g-tol%g" % c
# a finite input that reaches the tenth rejection: a step size 1e5 times too long on a skew-Hermitian matrix, whose estimate stays
# of the order of |v| however long the step, so that every rejection shortens the step by (tau tol / err)^(1/48) ~ 0.6 only
TENTH_REJECTION = ("schro700", "complex128", 1e5, 48, 1e5, 0.0)


@functools.lru_cache(maxsize=None)
def _arrays(name):
    from sprsolve_amd import gen
    if name == "cd9x8":
        ip, ix, d = gen.convection_diffusion_2d(9, 8)[:3]
        d = -np.asarray(d)
    elif name == "cd40x33":
        ip, ix, d = gen.convection_diffusion_2d(40, 33)[:3]
        d = -np.asarray(d)
    elif name == "heat12x11x10":
        ip, ix, d = gen.poisson3d(12, 11, 10)[:3]
        d = -np.asarray(d)
    elif name == "schro700":
        ip, ix, d = gen.hermitian_banded(700)[:3]
        d = -1j * np.asarray(d)
    elif name == "diag5":
        ip, ix, d = np.arange(301), np.arange(300), -(1.0 + np.arange(300) % 5)
    else:
        raise KeyError(name)
    ip, ix, d = np.ascontiguousarray(ip, np.int32), np.ascontiguousarray(ix, np.int32), np.asarray(d)
    for a in (ip, ix, d):
        a.setflags(write=False)
    return ip, ix, d


def system(name, dt):
    """-> (indptr, indices, data in dt)."""
    ip, ix, d = _arrays(name)
    return ip, ix, d.astype(dt)


def wide(dt):
    return C64 if np.dtype(dt).kind == "c" else F64


@functools.lru_cache(maxsize=None)
def propagator(name, t):
    """scipy.linalg.expm(t A) of the dense matrix in double (shared, read-only)."""
    import scipy.linalg
    ip, ix, d = _arrays(name)
    E = scipy.linalg.expm(t * ref.dense(ip, ix, d.astype(wide(d.dtype))))
    E.setflags(write=False)
    return E


def truth(name, dt, t):
    n = _arrays(name)[0].size - 1
    return propagator(name, t) @ ref.start_vector(n, dt).astype(wide(dt))


def true_error(name, dt, t, w):
    """|w - exp(tA) v|_2 formed in double."""
    return float(np.linalg.norm(np.asarray(w).astype(wide(dt)) - truth(name, dt, t)))


def tol_of(case):
    return case[5] if case[5] != 0.0 else ref.default_tol(np.dtype(case[1]))


@functools.lru_cache(maxsize=None)
def checker(case, sums="blas"):
    """The restatement's result on a case (shared, read-only)."""
    name, dtname, t, ncv, tau0, tol = case
    dt = np.dtype(dtname).type
    ip, ix, d = system(name, dt)
    o = ref.expm_apply(ip, ix, d, t, ref.start_vector(ip.size - 1, dt), ncv, tol, 100000, tau0, keep_H=True, sums=sums)
    if o.w is not None:
        o.w.setflags(write=False)
    return o


@pytest.fixture(scope="module")
def L():
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_expm_abi_and_binding_exist(L):
    src = open(os.path.join(ROOT, "include", "sprsolve_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sprs_[a-z0-9_]+)\s*\(", src)) if n.startswith("sprs_expm_"))
    assert declared == NAMES
    assert re.search(r"typedef\s+struct\s+sprs_expm\s+sprs_expm\s*;", src)
    assert re.search(r"#define\s+SPRS_EXPM_MAX_NCV\s+48\b", src)
    for name in NAMES:
        assert hasattr(L, name), name
    out = C.c_void_p()
    for s in "dzsc":
        assert getattr(L, "sprs_expm_create_" + s)(None, 4, 0, C.byref(out)) == 7 and not out.value       # a null A
        for f in ("apply", "apply_dev"):
            assert getattr(L, "sprs_expm_%s_%s" % (f, s))(None, 1.0, None, 4, 0.0, 1, 0.0, None, 4, None, None, None, None, None, None) == 7
    assert L.sprs_expm_destroy(None) == 0
    import sprsolve_amd
    from sprsolve_amd import _lib
    assert sprsolve_amd.Expm.NAME == "expm" and _lib.EXPM_MAX_NCV == ref.MAX_NCV == 48
    assert callable(sprsolve_amd.Expm.apply) and callable(sprsolve_amd.Expm.new) and callable(sprsolve_amd.expm_multiply)


def test_round2():
    for x, want in ((1234.0, 1200.0), (1250.0, 1300.0), (12.44, 12.0), (12.46, 13.0), (99.6, 100.0), (10.0, 10.0), (7.0, 7.0), (0.5, 0.5)):
        assert ref.round2(x) == want, (x, ref.round2(x))
    for x, want in ((0.01234, 0.012), (0.0995, 0.1), (3.14159e-7, 3.1e-7), (2.71828e-300, 2.7e-300), (6.02e23, 6.0e23), (1.66e308, 1.7e308)):
        assert abs(ref.round2(x) - want) <= 1e-13 * want, (x, ref.round2(x))
    rng = np.random.default_rng(5)
    for x in np.exp(rng.uniform(-600.0, 600.0, 400)):
        r = ref.round2(x)
        assert 0.95 * x < r <= 1.055 * x                     # floor(y + 0.55) on y in [10, 100)
        assert abs(ref.round2(r) - r) <= 1e-13 * r           # two digits stay two digits
    assert ref.round2(0.0) == 0.0 and ref.round2(-3.0) == -3.0 and ref.round2(np.inf) == np.inf and np.isnan(ref.round2(np.nan))
    assert ref.round2(5e-324) > 0.0                          # the 330 steps reach past the smallest subnormal


def _smallexp_check(X):
    """|smallexp(X) - expm(X)|_1 against a bound from the algorithm.  The Taylor remainder of degree 18 at |Y|_1 <= 1/2 is below
    (1/2)^19 / 19! ~ 1.6e-23: nothing.  Each of the 18 + s products of M terms rounds by at most M eps relative to the product of
    its factors' norms, and every squaring doubles the relative error it inherits: 2^s (19 + s) M eps, relative to `grow`, the
    largest |exp(X 2^-k)|_1^(2^k) over k <= s — what the factors' norms can amount to on the way (1 for a contraction, far more than
    |exp(X)|_1 for a non-normal X), formed here from scipy's exponentials."""
    import scipy.linalg
    M = X.shape[0]
    F, s = ref.smallexp(X)
    assert F is not None and 0 <= s <= ref.MAX_SQUARINGS
    E = scipy.linalg.expm(X)
    grow = 1.0                                               # the largest |exp(X 2^-k)|_1^(2^k): what the squarings can amplify
    for k in range(s + 1):
        grow = max(grow, float(np.linalg.norm(scipy.linalg.expm(X * 2.0 ** -k), 1)) ** (2 ** k))
    err = float(np.linalg.norm(F - E, 1))
    bound = 2.0 ** s * (ref.HORNER + 1 + s) * M * EPS64 * grow
    assert err <= bound, (err, bound, s, M)
    return s


def test_smallexp_on_the_projected_matrices_of_the_runs():
    most, seen = 0, 0
    for case in CASES:
        o = checker(case)
        assert len(o.Hs) == o.steps
        for Hc, tau_s, sgn in o.Hs[:: max(1, len(o.Hs) // 4)]:
            most = max(most, _smallexp_check(Hc * (sgn * tau_s)))
            seen += 1
    assert seen >= len(CASES) and 1 <= most <= 12


@pytest.mark.parametrize("M", [1, 2, 5, 14, 32, 50])
@pytest.mark.parametrize("scale", [0.0, 1e-3, 0.4, 3.0, 40.0])
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_smallexp_on_scaled_random_hessenberg(M, scale, kind):
    rng = np.random.default_rng(100 * M + int(10 * scale) + (kind == "complex"))
    X = rng.uniform(-1.0, 1.0, (M, M))
    if kind == "complex":
        X = X + 1j * rng.uniform(-1.0, 1.0, (M, M))
    X = np.triu(X, -1)
    X = X * (scale / max(float(np.linalg.norm(X, 1)), 1e-300))
    s = _smallexp_check(X)
    assert s == (0 if scale <= 0.5 else int(np.ceil(np.log2(scale))) + 1)


def test_smallexp_refuses_what_it_cannot_scale():
    assert ref.smallexp(np.array([[np.nan, 0.0], [0.0, 1.0]]))[0] is None
    assert ref.smallexp(np.array([[np.inf, 0.0], [0.0, 1.0]]))[0] is None
    assert ref.smallexp(np.array([[2.0 ** 64, 0.0], [0.0, 1.0]]))[0] is None       # s would be 65
    F, s = ref.smallexp(np.array([[-(2.0 ** 63), 0.0], [0.0, 0.0]]))               # s = 64: the last one taken
    assert s == 64 and F[0, 0] == 0.0 and F[1, 1] == 1.0
    F, s = ref.smallexp(np.zeros((3, 3)))
    assert s == 0 and np.array_equal(F, np.eye(3))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_counts_and_truth(case):
    """The restatement takes the recorded numbers of sub-steps, rejections and products and its true error, formed in double
    against scipy.linalg.expm of the dense matrix, is within delta |t| tol: the sum the accept rule allows."""
    name, dtname, t, ncv, tau0, tol = case
    o = checker(case)
    assert o.status == ref.OK and o.t_done == float(np.dtype(ref.real_dtype(dtname)).type(t))
    assert (o.steps, o.rejects, o.matvecs) == COUNTS[case]
    assert o.matvecs == sum(me if me < ncv else ncv + 1 for me in o.m_effs)
    bound = 1.2 * abs(t) * tol_of(case)
    err = true_error(name, dtname, t, o.w)
    print("%s: true error %.3e, estimate %.3e, bound %.3e" % (_id(case), err, o.err, bound))
    assert err <= bound and 0.0 <= o.err <= bound
    assert o.hump >= float(np.linalg.norm(ref.start_vector(o.w.size, dtname).astype(wide(dtname)))) * (1 - 1e-6)
    p = checker(case, "pairwise")
    assert p.status == ref.OK and abs(p.steps - o.steps) <= 1 and abs(p.rejects - o.rejects) <= 1
    assert true_error(name, dtname, t, p.w) <= bound


@pytest.mark.parametrize("dt", [F64, F32, C64, C32], ids=lambda d: np.dtype(d).name)
def test_happy_breakdown_on_five_distinct_entries(dt):
    """diag5 has five distinct eigenvalues: the Krylov space of any vector is invariant after five steps, the fifth hn is rounding
    noise under 64 eps scale, and the projected exponential is exact up to rounding."""
    case = ("diag5", np.dtype(dt).name, 1.5, 12, 0.0, 0.0)
    o = checker(case)
    assert o.status == ref.OK and (o.steps, o.rejects, o.matvecs) == (1, 0, 5) and o.m_effs == [5] and o.err == 0.0
    n = o.w.size
    exact = np.exp(1.5 * _arrays("diag5")[2]) * ref.start_vector(n, dt).astype(wide(dt))
    assert np.linalg.norm(o.w.astype(wide(dt)) - exact) <= 64 * float(np.finfo(ref.real_dtype(dt)).eps) * np.linalg.norm(exact)


def test_zero_time_zero_vector_nan_and_one_step():
    ip, ix, d = system("heat12x11x10", F64)
    n = ip.size - 1
    v = ref.start_vector(n, F64)
    o = ref.expm_apply(ip, ix, d, 0.0, v, 10)
    assert o.status == ref.OK and np.array_equal(o.w, v) and (o.steps, o.rejects, o.matvecs, o.err, o.hump, o.t_done) == (0, 0, 0, 0, 0, 0)
    o = ref.expm_apply(ip, ix, d, 0.5, np.zeros(n), 10)
    assert o.status == ref.OK and not np.any(o.w) and o.matvecs == 0
    bad = v.copy(); bad[17] = np.nan
    o = ref.expm_apply(ip, ix, d, 0.5, bad, 10)
    assert o.status == ref.BREAKDOWN and o.w is None and o.matvecs == 0
    o = ref.expm_apply(ip, ix, d, 0.5, v, 10, max_steps=1)
    assert o.status == ref.INSUFFICIENT_ITER and o.steps == 1 and 0.0 < o.t_done < 0.5 and o.matvecs == 11
    assert np.linalg.norm(o.w - propagator("heat12x11x10", o.t_done) @ v) <= 1.2 * 0.5 * ref.default_tol(F64)


def test_a_finite_input_reaches_the_tenth_rejection():
    o = checker(TENTH_REJECTION)
    assert o.status == ref.BREAKDOWN and o.w is None
    assert (o.steps, o.rejects, o.matvecs, o.t_done) == (0, ref.MAX_REJECTS - 1, 49, 0.0)
