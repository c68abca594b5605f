"""SpMM and batched CG without a GPU: the C ABI and the Python mirror exist, null handles are refused, and the checker of the
GPU tests (tests/_cg_many_ref.py) gives per column what tests/_cg_ref.py gives for that column alone."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cg_many_ref as many  # noqa: E402
import _cg_ref as ref  # noqa: E402

NAMES = sorted(["sprs_%s_%s" % (f, s) for f in ("mul_mat", "mul_mat_dev", "cgmany_create", "cgmany_solve", "cgmany_solve_dev") for s in "dzsc"]
               + ["sprs_cgmany_destroy"])


@pytest.fixture(scope="module")
def L():
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_abi_and_binding_exist(L):
    src = open(os.path.join(ROOT, "include", "sprsolve_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sprs_[a-z0-9_]+)\s*\(", src))
    assert sorted(n for n in declared if n.startswith(("sprs_cgmany_", "sprs_mul_mat_"))) == NAMES
    assert re.search(r"typedef\s+struct\s+sprs_cg_many\s+sprs_cg_many\s*;", src)
    from sprsolve_amd import _lib
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
    import sprsolve_amd
    assert callable(sprsolve_amd.HipCsr.mul_mat) and callable(sprsolve_amd.CGMany.new)
    assert callable(sprsolve_amd.CGMany.solve) and callable(sprsolve_amd.CGMany.precond_solve)


def test_null_handles_are_rejected(L):
    out = C.c_void_p()
    for s in "dzsc":
        assert getattr(L, "sprs_mul_mat_dev_" + s)(None, None, None, 2) == 7
        assert getattr(L, "sprs_mul_mat_" + s)(None, None, 8, None, 8, 2) == 7
        assert getattr(L, "sprs_cgmany_create_" + s)(None, 4, 2, C.byref(out)) == 7 and not out.value
        assert getattr(L, "sprs_cgmany_solve_dev_" + s)(None, None, None, 8, None, 8, 2, 10, 1e-8, None, None, None) == 7
    assert L.sprs_cgmany_destroy(None) == 0


def test_checker_of_checkers():
    from sprsolve_amd import gen
    ip, ix, d, rhs = gen.symmetric_banded(2000)
    n = rhs.size
    B = np.stack([rhs, gen.uniform(gen.SEED + 1, n), np.zeros(n), np.eye(1, n, n // 2)[0]], axis=1)
    dg = d[np.repeat(np.arange(n), np.diff(ip)) == ix]
    for diag in (None, dg):
        its, res, status, X = many.cg_many(ip, ix, d, B, np.zeros_like(B), 80, 1e-10, precond_diag=diag)
        assert its.shape == res.shape == status.shape == (4,) and X.shape == B.shape
        for j in range(4):
            o = ref.cg(ip, ix, d, B[:, j].copy(), np.zeros(n), 80, 1e-10, precond_diag=diag)
            assert (its[j], status[j]) == (o.its, o.status) and res[j] == o.res and np.array_equal(X[:, j], o.x)
        assert list(status) == [0, 0, 0, 0] and its[2] == 0 and not np.any(X[:, 2]) and 0 < its[3] < its[0]
    # a column that runs out of iterations does not disturb its neighbours' report
    its, res, status, X = many.cg_many(ip, ix, d, B, np.zeros_like(B), 21, 1e-10)
    assert list(status) == [ref.INSUFFICIENT_ITER, ref.INSUFFICIENT_ITER, ref.OK, ref.OK] and list(its[:2]) == [21, 21]
