"""Batched CG's checker: tests/_cg_ref.py's conjugate-gradient recurrence applied to each column of an (n, k) block on its
own — what sprs_cgmany_* must report per column.  Nothing is compared bit for bit against it (see _cg_ref.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cg_ref as ref  # noqa: E402


def cg_many(indptr, indices, data, RHS, X0, max_iter, tol, precond_diag=None):
    """-> (its, res, status, X): arrays of k entries and the (n, k) block of solutions; RHS / X0 are (n, k)."""
    RHS = np.asarray(RHS); X0 = np.asarray(X0)
    k = RHS.shape[1]
    its = np.zeros(k, np.int64); status = np.zeros(k, np.int32)
    res = np.zeros(k, np.float32 if np.dtype(data.dtype) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)
    X = np.array(X0, dtype=data.dtype)
    for j in range(k):
        o = ref.cg(indptr, indices, data, np.ascontiguousarray(RHS[:, j]), np.ascontiguousarray(X0[:, j]), max_iter, tol, precond_diag=precond_diag)
        its[j], res[j], status[j], X[:, j] = o.its, o.res, o.status, o.x
    return its, res, status, X
