"""The orderings as include/sprsolve_hip.h states them (sprs_csr_color, sprs_csr_permute, sprs_ilu0_create_ordered), restated
with plain loops: the checker of tests/test_order_cpu.py and tests/test_gpu_order.py.  The colouring twice — the greedy rule and
the Jones-Plassmann rounds the device runs, which must agree — the permutation over (indptr, indices, data), and the ordered
ILU(0) as tests/_ilu_ref.py's loops on the permuted matrix with the values mapped back to A's positions."""
import numpy as np

import _ilu_ref as ref

MASK = (1 << 64) - 1


def weight(seed, i):
    """w(i) of the header = gen.splitmix64_keys(seed, i), on Python integers."""
    z = ((seed & MASK) + (i + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def neighbours(indptr, indices):
    """i ~ j iff i != j and (i, j) or (j, i) is stored -> a list of sets."""
    n = indptr.size - 1
    nb = [set() for _ in range(n)]
    for i in range(n):
        for p in range(indptr[i], indptr[i + 1]):
            j = int(indices[p])
            if j != i:
                nb[i].add(j); nb[j].add(i)
    return nb


def _first_fit(i, nb, colour):
    used = {colour[j] for j in nb[i] if colour[j] >= 0}
    c = 0
    while c in used:
        c += 1
    return c


def greedy(indptr, indices, seed=0):
    """Greedy first-fit in decreasing (w(i), i) -> (colours int32, ncolours)."""
    n = indptr.size - 1
    nb = neighbours(indptr, indices)
    colour = [-1] * n
    for i in sorted(range(n), key=lambda v: (weight(seed, v), v), reverse=True):
        colour[i] = _first_fit(i, nb, colour)
    return np.array(colour, np.int32), (max(colour) + 1 if n else 0)


def jones_plassmann(indptr, indices, seed=0):
    """Round by round: the uncoloured vertices that beat every uncoloured neighbour take their first-fit colour against the
    colours of the rounds before -> (colours int32, ncolours, rounds)."""
    n = indptr.size - 1
    nb = neighbours(indptr, indices)
    key = [(weight(seed, i), i) for i in range(n)]
    colour = [-1] * n
    left, rounds = set(range(n)), 0
    while left:
        chosen = [i for i in left if all(colour[j] >= 0 or key[j] < key[i] for j in nb[i])]
        assert chosen
        new = {i: _first_fit(i, nb, colour) for i in chosen}   # all against the state before the round
        for i, c in new.items():
            colour[i] = c
        left -= set(chosen)
        rounds += 1
    return np.array(colour, np.int32), (max(colour) + 1 if n else 0), rounds


def is_proper(indptr, indices, colours):
    return all(colours[i] != colours[j] for i, s in enumerate(neighbours(indptr, indices)) for j in s)


def color_order(colours):
    """The stable sort of the rows by colour (new -> old)."""
    return np.array(sorted(range(len(colours)), key=lambda i: (colours[i], i)), np.int32)


def inverse(perm):
    inv = np.empty(len(perm), np.int32)
    for p, i in enumerate(perm):
        inv[i] = p
    return inv


def permute(indptr, indices, data, perm):
    """B = P A P^T, B[p, q] = A[perm[p], perm[q]] -> (indptr, indices, data, src): columns ascending by a stable sort (the rows
    of A in any stored order; duplicate columns stay, in their stored order), values bit copies, src[q] = the position in A's
    arrays of B's entry q."""
    n = indptr.size - 1
    inv = inverse(perm)
    ip = np.zeros(n + 1, np.int32)
    ix, src = [], []
    for p in range(n):
        i = int(perm[p])
        row = sorted((int(inv[indices[k]]), k) for k in range(indptr[i], indptr[i + 1]))
        ix += [c for c, _ in row]; src += [k for _, k in row]
        ip[p + 1] = len(ix)
    src = np.array(src, np.int64)
    return ip, np.array(ix, np.int32), data[src] if src.size else data[:0].copy(), src


class OrderedIlu:
    """The header's ordered ILU(0): tests/_ilu_ref.py's ilu0 and Applier on B = P A P^T.  status / row as ref.ilu0, the row in
    A's numbering; val: the factor values at A's CSR positions; solve(which, v) = P^T . Applier.solve(which, P v)."""

    def __init__(self, indptr, indices, data, perm):
        self.perm = np.asarray(perm, np.int32)
        self.bp, self.bx, bd, src = permute(indptr, indices, data, self.perm)
        f = ref.ilu0(self.bp, self.bx, bd)
        self.status = f.status
        self.row = int(self.perm[f.row]) if f.row >= 0 else -1
        self.val = None
        if f.status == ref.OK:
            self.val = np.empty_like(f.val)
            self.val[src] = f.val
            self.ap = ref.Applier(self.bp, self.bx, f.val)

    def levels(self):
        return ref.level_counts(self.bp, self.bx)

    def solve(self, which, v):
        v = np.asarray(v)
        out = np.empty_like(v)
        out[self.perm] = self.ap.solve(which, v[self.perm])
        return out

    def __call__(self, v):
        return self.solve(0, v)
