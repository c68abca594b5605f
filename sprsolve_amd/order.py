"""Orderings on the host side: what turns `HipCsr.color`'s colours into the permutation `HipCsr.permute` and
`ILU0.new(order=...)` take (include/sprsolve_hip.h, "orderings").  Permutations are int32, new -> old: `perm[p]` is the row
of A that becomes row p of P A P^T, i.e. scipy's `A[perm][:, perm]`."""
import numpy as np


def color_order(colors):
    """(perm, color_ptr): the stable sort of the rows by colour.  Rows of colour c are perm[color_ptr[c]:color_ptr[c + 1]],
    ascending; under this permutation every colour is a diagonal block of P A P^T."""
    colors = np.asarray(colors, dtype=np.int64)
    perm = np.argsort(colors, kind="stable").astype(np.int32)
    ncolors = int(colors.max()) + 1 if colors.size else 0
    color_ptr = np.zeros(ncolors + 1, np.int64)
    np.cumsum(np.bincount(colors, minlength=ncolors), out=color_ptr[1:])
    return perm, color_ptr


def inverse_permutation(perm):
    """ord with ord[perm[p]] = p: the new index of every old row."""
    perm = np.asarray(perm, dtype=np.int32)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size, dtype=np.int32)
    return inv
