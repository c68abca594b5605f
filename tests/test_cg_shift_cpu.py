"""Multi-shift CG without a GPU: the C ABI and the Python mirror exist, null handles are refused, and the checker of the GPU
tests (tests/_cg_shift_ref.py) gives per shift what tests/_cg_ref.py gives on the matrix with the shift added to its diagonal.

The iteration counts of tests/_cg_ref.py on A + sigma I (gen.symmetric_banded(2000) / gen.hermitian_banded(1500, 3), the
generator's rhs, x0 = 0) for sigma = 0, 1/32, 1/4, 1, 4, 16, 64, 1024:
    f64 (tol 1e-10) 26 26 25 22 16 10 7 4        c64 (1e-10) 26 26 24 21 16 10 7 4
    f32 (tol 1e-5)  14 14 13 11  8  5 4 2        c32 (1e-5)  13 13 12 11  8  5 4 2"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cg_ref as ref  # noqa: E402
import _cg_shift_ref as shift  # noqa: E402

NAMES = sorted(["sprs_cgshift_%s_%s" % (f, s) for f in ("create", "solve", "solve_dev") for s in "dzsc"] + ["sprs_cgshift_destroy"])
SHIFTS = [0.0, 1.0 / 32, 0.25, 1.0, 4.0, 16.0, 64.0, 1024.0]
F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
COUNTS = {"float64": [26, 26, 25, 22, 16, 10, 7, 4], "complex128": [26, 26, 24, 21, 16, 10, 7, 4],
          "float32": [14, 14, 13, 11, 8, 5, 4, 2], "complex64": [13, 13, 12, 11, 8, 5, 4, 2]}


@pytest.fixture(scope="module")
def L():
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _system(dt):
    from sprsolve_amd import gen
    ip, ix, d, rhs = gen.hermitian_banded(1500, 3) if np.dtype(dt).kind == "c" else gen.symmetric_banded(2000)
    return ip, ix, d.astype(dt), rhs.astype(dt)


def _tol(dt):
    return 1e-5 if np.dtype(dt) in (np.dtype(F32), np.dtype(C32)) else 1e-10


def test_abi_and_binding_exist(L):
    src = open(os.path.join(ROOT, "include", "sprsolve_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sprs_[a-z0-9_]+)\s*\(", src))
    assert len(NAMES) == 13 and sorted(n for n in declared if n.startswith("sprs_cgshift_")) == NAMES
    assert re.search(r"typedef\s+struct\s+sprs_cg_shift\s+sprs_cg_shift\s*;", src)
    from sprsolve_amd import _lib
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
    import sprsolve_amd
    assert callable(sprsolve_amd.CGShift.new) and callable(sprsolve_amd.CGShift.solve)


def test_null_handles_are_rejected(L):
    out = C.c_void_p()
    for s in "dzsc":
        assert getattr(L, "sprs_cgshift_create_" + s)(None, 4, 2, C.byref(out)) == 7 and not out.value
        for f in ("solve_", "solve_dev_"):
            assert getattr(L, "sprs_cgshift_" + f + s)(None, None, 2, None, 4, None, 8, 10, 1e-8, None, None, None) == 7
    assert L.sprs_cgshift_destroy(None) == 0


@pytest.mark.parametrize("dt", [F64, C64, F32, C32], ids=lambda d: np.dtype(d).name)
def test_checker_of_checkers(dt):
    ip, ix, d, rhs = _system(dt)
    n = rhs.size
    tol = _tol(dt)
    its, res, status, X = shift.cg_shift(ip, ix, d, rhs, SHIFTS, 80, tol)
    assert its.shape == res.shape == status.shape == (8,) and X.shape == (8, n) and X.dtype == np.dtype(dt)
    single = np.dtype(dt) in (np.dtype(F32), np.dtype(C32))
    for j, sg in enumerate(SHIFTS):
        o = ref.cg(ip, ix, shift.shifted(ip, ix, d, sg), rhs.copy(), np.zeros(n, dt), 80, tol)
        err = np.max(np.abs(X[j] - o.x)) / max(1.0, np.max(np.abs(o.x)))
        print("%s sigma %g: its %d (CG alone %d, tabulated %d) res %.3e (%.3e) max|x - x_cg| %.3e"
              % (np.dtype(dt).name, sg, its[j], o.its, COUNTS[np.dtype(dt).name][j], res[j], o.res, err))
        assert status[j] == ref.OK and o.status == ref.OK
        assert o.its == COUNTS[np.dtype(dt).name][j]
        assert abs(int(its[j]) - o.its) <= 1
        assert res[j] <= tol
        assert err <= (1e-5 if single else 1e-12)


def test_events_of_the_checker():
    ip, ix, d, rhs = _system(F64)
    n = rhs.size
    full = shift.cg_shift(ip, ix, d, rhs, SHIFTS, 80, 1e-10)
    # -A: not positive definite along the first direction, every column breaks down at once
    its, res, status, X = shift.cg_shift(ip, ix, -d, rhs, SHIFTS, 80, 1e-10)
    assert np.all(status == ref.BREAKDOWN) and not np.any(its) and not np.any(X)
    # a zero right-hand side
    its, res, status, X = shift.cg_shift(ip, ix, d, np.zeros(n), SHIFTS, 80, 1e-10)
    assert np.all(status == ref.OK) and not np.any(its) and not np.any(X)
    # max_iter = 12: the columns that need more stop there, the others are untouched by their neighbours' fate
    its, res, status, X = shift.cg_shift(ip, ix, d, rhs, SHIFTS, 12, 1e-10)
    for j, c in enumerate(COUNTS["float64"]):
        if c > 12:
            assert status[j] == ref.INSUFFICIENT_ITER and its[j] == 12
        else:
            assert status[j] == ref.OK and its[j] == full[0][j] and res[j] == full[1][j] and np.array_equal(X[j], full[3][j])
