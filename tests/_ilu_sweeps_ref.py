"""The Jacobi-sweep triangular solves of include/sprsolve_hip.h (sprs_ilu0_create_sweeps), restated with plain loops over
tests/_ilu_ref.py's Scalar: the checker of tests/test_ilu_sweeps_cpu.py and tests/test_gpu_ilu_sweeps.py.  Every sweep reads only
the previous sweep's vector, every sigma is folded from +0 over the row's stored entries in ascending column order, so the results
can be compared BIT FOR BIT with the library's."""
import numpy as np

import _ilu_ref as ref


class Sweeps(ref.Applier):
    """ref.Applier with each fold replaced by k sweeps.  solve(which, v): 0 = the upper sweeps on the lower sweeps' output,
    1 = the lower sweeps, 2 = the upper sweeps."""

    def __init__(self, indptr, indices, val, k):
        super().__init__(indptr, indices, val)
        assert k >= 1
        self.k = int(k)

    def _lower(self, r):
        S, ix, a = self.S, self.ix, self.a
        y = list(r)                                          # y(1) = in
        for _ in range(self.k - 1):
            new = [None] * self.n
            for i in range(self.n):
                sigma = S.zero()
                for p in range(self.ip[i], self.dpos[i]):
                    sigma = S.add(sigma, S.mul(a[p], y[ix[p]]))
                new[i] = S.sub(r[i], sigma)
            y = new
        return y

    def _upper(self, y):
        S, ix, a = self.S, self.ix, self.a
        z = [S.div(y[i], a[self.dpos[i]]) for i in range(self.n)]   # z(1)
        for _ in range(self.k - 1):
            new = [None] * self.n
            for i in range(self.n):
                sigma = S.zero()
                for p in range(self.dpos[i] + 1, self.ip[i + 1]):
                    sigma = S.add(sigma, S.mul(a[p], z[ix[p]]))
                new[i] = S.div(S.sub(y[i], sigma), a[self.dpos[i]])
            z = new
        return z


class Columns(ref.Scalar):
    """ref.Scalar whose scalars are numpy vectors (a complex one a pair of them): the unchanged loops of an applier then run on
    many right-hand sides at once, every element with the operations and roundings of the scalar path."""

    def _div(self, a, b):
        with np.errstate(all="ignore"):
            return self.R(a) / self.R(b)

    def vec_load(self, V):
        V = np.asarray(V, dtype=self.T)
        return [(r.real.astype(self.R), r.imag.astype(self.R)) if self.cx else r.astype(self.R) for r in V]

    def vec_store(self, s):
        return np.array([(e[0] + 1j * e[1]) if self.cx else e for e in s], dtype=self.T)


def dense_operator(applier, which=0):
    """The n x n matrix of applier.solve(which, .), column by column (all columns in one pass of the applier's own loops)."""
    scalar, applier.S = applier.S, Columns(applier.S.T)
    try:
        return applier.solve(which, np.eye(applier.n, dtype=scalar.T))
    finally:
        applier.S = scalar
