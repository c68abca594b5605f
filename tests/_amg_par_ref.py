"""The parallel aggregation rule of sprs_amg_create_dev as include/sprsolve_hip.h states it: the checker of
tests/test_amg_par_cpu.py and tests/test_gpu_amg_device_setup.py.  The rule is restated twice as plain Python loops — the greedy
loop in decreasing (splitmix64(seed, i), i), and the rounds the device runs — and everything else of a level (the products, the
transpose, omega, the LU, the cycle) is tests/_amg_ref.py's, so a hierarchy built here differs from the host rule's in its
aggregates alone."""
from collections import namedtuple

import numpy as np

import _amg_ref as amg

# as _amg_ref.Hierarchy (Applier takes either), plus the pass-1 rounds of every aggregated level
Hierarchy = namedtuple("Hierarchy", "status row levels lu dtype rounds")


def keys(seed, n):
    from sprsolve_amd import gen
    return [int(v) for v in gen.splitmix64_keys(seed, np.arange(n))]


def graph(op, ip, ix, val, diag, theta):
    """nb[i] = {j: w(i, j)}: i ~ j when (i, j) or (j, i) is a strong stored entry, w the largest |a|^2 among those of the two
    that are strong."""
    n = ip.size - 1
    R = op.R.type
    rows = np.repeat(np.arange(n), np.diff(ip))
    md = op.mod(diag)
    sq = op.sq(val)
    th2 = R(theta) * R(theta)
    strong = (ix != rows) & (sq >= th2 * (md[rows] * md[ix]))
    nb = [dict() for _ in range(n)]
    for i, j, w in zip(rows[strong].tolist(), ix[strong].tolist(), sq[strong].tolist()):
        for a, b in ((i, j), (j, i)):
            if nb[a].get(b, -1.0) < w:
                nb[a][b] = w
    return nb


def pass1_greedy(nb, key):
    """root[i] = the root of i's aggregate after pass 1, or -1."""
    n = len(nb)
    root = [-1] * n
    for i in sorted(range(n), key=lambda v: (key[v], v), reverse=True):
        if root[i] < 0 and all(root[j] < 0 for j in nb[i]):
            root[i] = i
            for j in nb[i]:
                root[j] = i
    return root


def pass1_rounds(nb, key):
    """The device form -> (root, rounds)."""
    n = len(nb)
    root = [-1] * n
    undecided = [True] * n
    rounds = 0
    while True:
        for i in range(n):
            if undecided[i] and (root[i] >= 0 or any(root[j] >= 0 for j in nb[i])):
                undecided[i] = False
        if not any(undecided):
            return root, rounds
        assert rounds < n
        rounds += 1
        none = (-1, -1)
        m1 = [max([(key[j], j) for j in list(nb[k]) + [k] if undecided[j]], default=none) for k in range(n)]
        winners = [i for i in range(n) if undecided[i] and max(m1[k] for k in list(nb[i]) + [i]) == (key[i], i)]
        assert winners, "a round without a winner"
        for i in winners:
            root[i] = i
            for j in nb[i]:
                root[j] = i


def pass2(nb, root):
    """Against the snapshot `root`: a free vertex joins the aggregate of its aggregated neighbour of largest w, ties to the
    smallest index.  A vertex without such a neighbour keeps -1."""
    out = list(root)
    for i in range(len(nb)):
        if root[i] >= 0:
            continue
        best = max([(w, -j) for j, w in nb[i].items() if root[j] >= 0], default=None)
        if best is not None:
            out[i] = root[-best[1]]
    return out


def number(root):
    """Aggregates numbered by ascending root index -> (agg, count)."""
    r = np.asarray(root, np.int64)
    roots = np.nonzero(r == np.arange(r.size))[0]
    ids = np.full(r.size, -1, np.int64)
    ids[roots] = np.arange(roots.size)
    return ids[r], int(roots.size)


def aggregate(op, ip, ix, val, diag, theta, seed):
    """-> (agg, count, rounds); every row is placed (asserted: the header's argument)."""
    nb = graph(op, ip, ix, val, diag, theta)
    root, rounds = pass1_rounds(nb, keys(seed, len(nb)))
    root = pass2(nb, root)
    assert min(root, default=0) >= 0
    agg, nc = number(root)
    return agg, nc, rounds


def build(indptr, indices, data, theta=0.08, coarse_max=256, max_levels=16, seed=0, ncols=None):
    """_amg_ref.build with the parallel rule in place of the three serial passes."""
    op = amg.Ops(data.dtype)
    n = indptr.size - 1
    fail = lambda st, row=-1: Hierarchy(st, row, None, None, op.T, None)
    if ncols is not None and ncols != n:
        return fail(amg.NOT_SQUARE)
    if not (theta >= 0) or coarse_max < 1 or coarse_max > amg.COARSE_LIMIT or max_levels < 1 or max_levels > amg.LEVELS_LIMIT:
        return fail(amg.INVALID_ARGUMENT)
    ip = np.asarray(indptr, np.int64); ix = np.asarray(indices, np.int64); val = np.asarray(data)
    for i in range(n):
        if np.any(np.diff(ix[ip[i]:ip[i + 1]]) <= 0):
            return fail(amg.INVALID_ARGUMENT, i)
    levels, rounds = [], []
    lvl = 0
    while True:
        rows = np.repeat(np.arange(n), np.diff(ip))
        on = rows == ix
        bad = np.ones(n, bool)
        bad[rows[on]] = op.bad_pivot(val[on])
        if bad.any():
            return fail(amg.ZERO_DIAGONAL, int(np.nonzero(bad)[0][0]))
        diag = val[on]
        omega = amg._omega(op, ip, val, diag)
        if n <= coarse_max or lvl + 1 >= max_levels:
            break
        agg, nc, rnd = aggregate(op, ip, ix, val, diag, op.R.type(theta) * op.R.type(2.0 ** -lvl), seed)
        if 2 * nc > n:
            break
        tip = np.arange(n + 1, dtype=np.int64)
        aip, aix, av = amg.spgemm(op, nc, ip, ix, val, tip, agg, np.ones(n, op.T))
        arow = np.repeat(np.arange(n), np.diff(aip))
        t = (aix == agg[arow]).astype(op.T)
        pv = op.sub(t, op.div(op.mulr(av, omega), diag[arow]))
        P = (aip, aix, pv)
        Rm = amg.transpose_conj(op, nc, *P)
        apip, apix, apv = amg.spgemm(op, nc, ip, ix, val, *P)
        cip, cix, cv = amg.spgemm(op, nc, *Rm, apip, apix, apv)
        levels.append(amg.Level(n, ip, ix, val, diag, omega, agg, P, Rm))
        rounds.append(rnd)
        ip, ix, val, n = cip, cix, cv, nc
        lvl += 1
    levels.append(amg.Level(n, ip, ix, val, diag, omega, None, None, None))
    lu = None
    if n <= coarse_max:
        M = np.zeros((n, n), op.T); M[np.repeat(np.arange(n), np.diff(ip)), ix] = val
        st, row, lu = amg.dense_lu(op, M)
        if st != amg.OK:
            return fail(st, row)
    return Hierarchy(amg.OK, -1, levels, lu, op.T, rounds)
