"""The parallel aggregation rule of sprs_amg_create_dev (tests/_amg_par_ref.py) checked on the CPU: the rounds the device runs
against the greedy loop they stand for, on every level of every system the GPU file uses; what the rule must give (a partition,
nothing left after pass 2, an operator complexity no larger than the serial rule's); the level sizes, round counts and
iteration counts as constants; the symmetry of the cycle; the exported symbols.  The extra systems of the GPU file (a hub row, isolated rows, a one-sided strength
pattern) are built here."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _amg_par_ref as par  # noqa: E402
import _amg_ref as amg  # noqa: E402
import _ilu_ref as ref  # noqa: E402
from test_amg_cpu import (CG_COUNTS, COARSE_MAX, GMRES_COUNTS, GMRES_RESTART, MAX_LEVELS, THETA, _complex_rhs, hierarchy_of,  # noqa: E402
                          system_of)
from test_ilu_cpu import C64, F64  # noqa: E402

SEEDS = (0, 1)
NAMED = ("p3_12x11x10", "p3_24x22x20", "cd24x20", "cd64x64", "tri300", "ragged1000", "p3_64x64x8")
EXTRA = ("hub600", "isolated400", "onesided400")
# Hubs whose wavefront holds undecided vertices of larger key that are NOT their neighbours: a whole-wavefront walk that let a
# helping lane's own vertex into the hub's maximum would delay winners and count more rounds (seed 7: 4 for 3, and 3 for 2).
WIDE_HUBS = {"hub600_at70": (70, 100, 400), "hub600_at130": (130, 200, 500)}
WIDE_SEED = 7
WIDE_ROUNDS = {"hub600_at70": [3], "hub600_at130": [2]}


def _csr(M):
    R, Cc = np.nonzero(M)
    ip = np.zeros(M.shape[0] + 1, np.int32); np.cumsum(np.bincount(R, minlength=M.shape[0]), out=ip[1:])
    return ip, Cc.astype(np.int32), M[R, Cc]


def hub_matrix(n=600, hub=17, lo=100, hi=400):
    """A chain (4 on the diagonal, -1 beside it) with one hub: row and column `hub` hold -1 at lo .. hi - 1 and 30 on the
    diagonal, so all 300 couplings are strong (1 >= 0.08^2 * 30 * 4) and the hub's neighbour list is longer than a wavefront."""
    M = np.zeros((n, n))
    i = np.arange(n)
    M[i, i] = 4.0
    M[i[:-1], i[:-1] + 1] = -1.0; M[i[:-1] + 1, i[:-1]] = -1.0
    M[hub, lo:hi] = -1.0; M[lo:hi, hub] = -1.0
    M[hub, hub] = 30.0
    return M


def isolated_matrix(n=400):
    """The chain with every row i = 3 (mod 7) cut out of it: such a row stores its diagonal alone and no other row stores its
    column, so it has no neighbour in G and founds a singleton."""
    M = np.zeros((n, n))
    i = np.arange(n)
    M[i[:-1], i[:-1] + 1] = -1.0; M[i[:-1] + 1, i[:-1]] = -1.0
    cut = i % 7 == 3
    M[cut, :] = 0.0; M[:, cut] = 0.0
    M[i, i] = 2.0
    return M


def onesided_matrix(n=400):
    """Strength that is not symmetric: (i, i + 1) = -1 is strong while (i + 1, i) = -0.05 is stored and weak
    (0.0025 < 0.08^2 * 16), and (i, i + 5) = -0.5 is strong with nothing stored at (i + 5, i)."""
    M = np.zeros((n, n))
    i = np.arange(n)
    M[i, i] = 4.0
    M[i[:-1], i[:-1] + 1] = -1.0; M[i[:-1] + 1, i[:-1]] = -0.05
    M[i[:-5], i[:-5] + 5] = -0.5
    return M


@functools.lru_cache(maxsize=None)
def par_system_of(name, dtname):
    """test_amg_cpu.system_of, extended by the three systems above (real values in every scalar type)."""
    if name not in EXTRA and name not in WIDE_HUBS:
        return system_of(name, dtname)
    if name in WIDE_HUBS:
        hub, lo, hi = WIDE_HUBS[name]
        ip, ix, d = _csr(hub_matrix(600, hub, lo, hi))
    else:
        ip, ix, d = _csr({"hub600": hub_matrix, "isolated400": isolated_matrix, "onesided400": onesided_matrix}[name]())
    d = d.astype(dtname); rhs = _complex_rhs(ip.size - 1, np.dtype(dtname).type)
    for a in (ip, ix, d, rhs):
        a.setflags(write=False)
    return ip, ix, d, rhs


@functools.lru_cache(maxsize=None)
def par_hierarchy_of(name, dtname, seed, coarse_max=COARSE_MAX):
    ip, ix, d, _ = par_system_of(name, dtname)
    H = par.build(ip, ix, d, THETA, coarse_max, MAX_LEVELS, seed)
    assert H.status == amg.OK, (name, H.status, H.row)
    return H


# f64, the defaults of AMG.new: rows per level and pass-1 rounds per aggregated level, by seed
ROWS = {
    "p3_12x11x10": ([1320, 135], [1320, 135]),
    "p3_24x22x20": ([10560, 1007, 98], [10560, 998, 100]),
    "cd24x20": ([480, 70], [480, 71]),
    "cd64x64": ([4096, 585, 54], [4096, 586, 53]),
    "tri300": ([300, 85], [300, 86]),
    "ragged1000": ([1000, 75], [1000, 81]),
    "p3_64x64x8": ([32768, 3136, 319, 48], [32768, 3121, 303, 38]),
    "hub600": ([600, 84], [600, 80]),
    "isolated400": ([400, 172], [400, 172]),
    "onesided400": ([400, 54], [400, 56]),
}
ROUNDS = {
    "p3_12x11x10": ([4], [5]),
    "p3_24x22x20": ([5, 5], [5, 5]),
    "cd24x20": ([5], [4]),
    "cd64x64": ([4, 3], [5, 4]),
    "tri300": ([3], [3]),
    "ragged1000": ([7], [6]),
    "p3_64x64x8": ([6, 5, 4], [6, 4, 4]),
    "hub600": ([3], [3]),
    "isolated400": ([2], [2]),
    "onesided400": ([3], [4]),
}
# iterations of the checker's solvers at tol 1e-10 with the hierarchy of seed 0 / seed 1
CG_PAR_COUNTS = (17, 17)                                      # system "cg", f64 = poisson3d(12, 11, 10)
CG_PAR_COUNTS_24 = (18, 18)                                   # poisson3d(24, 22, 20)
GMRES_PAR_COUNTS = (19, 20)                                   # cd24x20, GMRES(10)
CG_JACOBI_COUNT = 63                                          # system "cg", f64, Jacobi


def _complexity(H):
    nnz = [int(L.ip[-1]) for L in H.levels]
    return sum(nnz) / nnz[0]


# ------------------------------------------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", NAMED + EXTRA)
def test_rounds_are_the_greedy_loop_and_the_aggregates_partition_the_rows(name, seed):
    ip, ix, d, _ = par_system_of(name, "float64")
    H = par_hierarchy_of(name, "float64", seed)
    op = amg.Ops(F64)
    assert len(H.levels) >= 2 and len(H.rounds) == len(H.levels) - 1
    for l, L in enumerate(H.levels[:-1]):
        nb = par.graph(op, L.ip, L.ix, L.val, L.diag, op.R.type(THETA) * op.R.type(2.0 ** -l))
        key = par.keys(seed, L.n)
        greedy = par.pass1_greedy(nb, key)
        sim, rounds = par.pass1_rounds(nb, key)
        assert sim == greedy and rounds == H.rounds[l], (l, rounds)
        # pass 1 is maximal: every free vertex has an aggregated neighbour, so pass 2 leaves no row
        placed = par.pass2(nb, sim)
        assert min(placed) >= 0
        agg, nc = par.number(placed)
        assert np.array_equal(agg, L.agg) and nc == H.levels[l + 1].n
        assert np.array_equal(np.unique(agg), np.arange(nc))                     # a partition, every aggregate inhabited
        roots = np.nonzero(np.asarray(sim) == np.arange(L.n))[0]
        assert np.array_equal(agg[roots], np.arange(nc))                         # numbered by ascending root
    print(name, seed, "rows", [L.n for L in H.levels], "rounds", H.rounds, "sum nnz / nnz0 = %.3f" % _complexity(H))
    assert [L.n for L in H.levels] == ROWS[name][seed]
    assert H.rounds == ROUNDS[name][seed]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", NAMED)
def test_operator_complexity_is_no_larger_than_the_serial_rules(name, seed):
    c_par, c_host = _complexity(par_hierarchy_of(name, "float64", seed)), _complexity(hierarchy_of(name, "float64"))
    print(name, seed, "%.3f against %.3f" % (c_par, c_host))
    assert c_par <= c_host


def _rounds_with_leaking_wavefront(nb, key, wave=64):
    """par.pass1_rounds as a whole-wavefront walk would run it if each helping lane started its partial maximum from ITS OWN
    vertex: for a vertex of more than `wave` neighbours, m1 and the win test also see the undecided vertices (and their m1) of the
    64 consecutive vertices it shares a wavefront with.  The roots stay right (the test only gets stricter); winners are delayed."""
    n = len(nb)
    root = [-1] * n
    undecided = [True] * n
    rounds = 0
    none = (-1, -1)
    mates = lambda k: range(wave * (k // wave), min(wave * (k // wave) + wave, n)) if len(nb[k]) > wave else [k]
    while True:
        for i in range(n):
            if undecided[i] and (root[i] >= 0 or any(root[j] >= 0 for j in nb[i])):
                undecided[i] = False
        if not any(undecided):
            return root, rounds
        rounds += 1
        m1 = [max([(key[j], j) for j in list(nb[k]) + list(mates(k)) if undecided[j]], default=none) for k in range(n)]
        seen = lambda i: [m1[k] for k in nb[i]] + [m1[k] for k in mates(i) if undecided[k]]
        winners = [i for i in range(n) if undecided[i] and max(seen(i)) == (key[i], i)]
        assert winners
        for i in winners:
            root[i] = i
            for j in nb[i]:
                root[j] = i


@pytest.mark.parametrize("name", sorted(WIDE_HUBS))
def test_round_counts_of_the_hubs_that_share_a_wavefront_with_larger_keys(name):
    """The cases of the GPU file that tell a correct whole-wavefront walk from one whose helping lanes bring their own vertices
    along: the same roots either way, one round more with the leak."""
    H = par_hierarchy_of(name, "float64", WIDE_SEED)
    hub = WIDE_HUBS[name][0]
    key = par.keys(WIDE_SEED, 600)
    L = H.levels[0]
    nb = par.graph(amg.Ops(F64), L.ip, L.ix, L.val, L.diag, amg.Ops(F64).R.type(THETA))
    assert len(nb[hub]) > 64 and H.rounds == WIDE_ROUNDS[name]
    root, rounds = par.pass1_rounds(nb, key)
    assert root == par.pass1_greedy(nb, key) and [rounds] == WIDE_ROUNDS[name]
    leaky_root, leaky_rounds = _rounds_with_leaking_wavefront(nb, key)
    assert leaky_root == root and leaky_rounds == rounds + 1
    for seed in SEEDS:                                       # the hub of the other cases does not tell them apart
        nb0 = par.graph(amg.Ops(F64), *par_system_of("hub600", "float64")[:3], par_hierarchy_of("hub600", "float64", seed).levels[0].diag,
                        amg.Ops(F64).R.type(THETA))
        assert _rounds_with_leaking_wavefront(nb0, par.keys(seed, 600))[1] == ROUNDS["hub600"][seed][0]


def test_seeds_give_different_aggregates():
    a, b = (par_hierarchy_of("p3_12x11x10", "float64", s).levels[0].agg for s in SEEDS)
    assert not np.array_equal(a, b)


def test_hub_isolated_and_onesided_systems_are_what_they_claim():
    op = amg.Ops(F64)
    th = op.R.type(THETA)
    ip, ix, d, _ = par_system_of("hub600", "float64")
    diag = d[np.repeat(np.arange(600), np.diff(ip)) == ix]
    nb = par.graph(op, ip, ix, d, diag, th)
    assert len(nb[17]) == 302                                 # longer than four wavefronts' lanes: the whole-wavefront walk
    agg = par_hierarchy_of("hub600", "float64", 0).levels[0].agg
    assert np.bincount(agg).max() >= 200                      # aggregate sizes are unbounded under a hub
    ip, ix, d, _ = par_system_of("isolated400", "float64")
    diag = d[np.repeat(np.arange(400), np.diff(ip)) == ix]
    nb = par.graph(op, ip, ix, d, diag, th)
    lone = [i for i in range(400) if not nb[i]]
    assert lone == list(range(3, 400, 7))
    agg = par_hierarchy_of("isolated400", "float64", 0).levels[0].agg
    assert all(np.count_nonzero(agg == agg[i]) == 1 for i in lone)
    ip, ix, d, _ = par_system_of("onesided400", "float64")
    rows = np.repeat(np.arange(400), np.diff(ip))
    diag = d[rows == ix]
    strong = (ix != rows) & (d * d >= th * th * (np.abs(diag)[rows] * np.abs(diag)[ix]))
    S = set(zip(rows[strong].tolist(), ix[strong].tolist()))
    assert (0, 1) in S and (1, 0) not in S and (0, 5) in S and (5, 0) not in S
    nb = par.graph(op, ip, ix, d, diag, th)
    assert 0 in nb[5] and 5 in nb[0] and nb[5][0] == 0.25     # G is symmetric all the same


# ------------------------------------------------------------------------------------------------ 2. the cycle
@pytest.mark.parametrize("dt", [F64, C64], ids=lambda d: np.dtype(d).name)
def test_cycle_is_hermitian(dt):
    name = np.dtype(dt).name
    ip, ix, d, _ = par_system_of("p3_12x11x10", name)
    H = par_hierarchy_of("p3_12x11x10", name, 0)
    assert len(H.levels) == 2
    ap = amg.Applier(H)
    n = ip.size - 1
    M = np.array([ap(e) for e in np.eye(n, dtype=dt)]).T
    assert np.max(np.abs(M - M.conj().T)) <= 1e-15 * n * np.max(np.abs(M))
    assert np.linalg.eigvalsh((M + M.conj().T) / 2).min() > 0


# ------------------------------------------------------------------------------------------------ 3. iteration counts
def test_amg_cg_counts():
    ip, ix, d, rhs = system_of("cg", "float64")
    n = rhs.size
    ilu_count, host_count = CG_COUNTS["float64"]
    oj = ref.cg(ip, ix, d, rhs, np.zeros(n), 2 * CG_JACOBI_COUNT, 1e-10, prec=ref.jacobi(ip, ix, d))
    assert (oj.status, oj.its) == (ref.OK, CG_JACOBI_COUNT)
    for seed in SEEDS:
        H = par.build(ip, ix, d, THETA, COARSE_MAX, MAX_LEVELS, seed)
        o = ref.cg(ip, ix, d, rhs, np.zeros(n), 2 * CG_PAR_COUNTS[seed], 1e-10, prec=amg.Applier(H))
        print("cg seed %d: %d iterations (host rule %d, ILU(0) %d, Jacobi %d)" % (seed, o.its, host_count, ilu_count, oj.its))
        assert (o.status, o.its) == (ref.OK, CG_PAR_COUNTS[seed])
        assert o.its < ilu_count == 21 and o.its < oj.its == 63


def test_amg_cg_count_is_flat_in_the_grid():
    ip, ix, d, rhs = system_of("p3_24x22x20", "float64")
    for seed in SEEDS:
        o = ref.cg(ip, ix, d, rhs, np.zeros(rhs.size), 2 * CG_PAR_COUNTS_24[seed], 1e-10,
                   prec=amg.Applier(par_hierarchy_of("p3_24x22x20", "float64", seed)))
        assert (o.status, o.its) == (ref.OK, CG_PAR_COUNTS_24[seed])
        assert abs(o.its - CG_PAR_COUNTS[seed]) <= 3


def test_amg_gmres_needs_fewer_steps_than_jacobi():
    ip, ix, d, rhs = system_of("cd24x20", "float64")
    jacobi_count = GMRES_COUNTS["float64"][0]
    for seed in SEEDS:
        o = ref.gmres(ip, ix, d, rhs, np.zeros(rhs.size), 2 * GMRES_PAR_COUNTS[seed], 1e-10, restart=GMRES_RESTART,
                      prec=amg.Applier(par_hierarchy_of("cd24x20", "float64", seed)))
        assert (o.status, o.its) == (ref.OK, GMRES_PAR_COUNTS[seed])
        assert o.its < jacobi_count == 107


# ------------------------------------------------------------------------------------------------ 4. errors, symbols
def test_creation_errors_are_the_serial_rules():
    ip = np.array([0, 2, 4], np.int32); ix = np.array([0, 1, 0, 1], np.int32)
    assert par.build(ip, ix, np.ones(4), ncols=3).status == amg.NOT_SQUARE
    H = par.build(ip, ix, np.ones(4))
    assert (H.status, H.row) == (amg.ZERO_DIAGONAL, 1)        # the coarse LU: u_11 = 1 - 1*1
    ip3 = np.array([0, 2, 3, 5, 6], np.int32); ix3 = np.array([0, 1, 0, 1, 2, 2], np.int32)
    assert par.build(ip3, ix3, np.ones(6))[:2] == (amg.ZERO_DIAGONAL, 1)
    assert par.build(ip, np.array([1, 0, 0, 1], np.int32), np.ones(4))[:2] == (amg.INVALID_ARGUMENT, 0)
    assert par.build(ip, np.array([0, 1, 1, 1], np.int32), np.ones(4))[:2] == (amg.INVALID_ARGUMENT, 1)
    for kw in (dict(theta=-1.0), dict(coarse_max=0), dict(coarse_max=amg.COARSE_LIMIT + 1), dict(max_levels=0),
               dict(max_levels=amg.LEVELS_LIMIT + 1)):
        assert par.build(ip, ix, np.array([2.0, 1.0, 1.0, 2.0]), **kw).status == amg.INVALID_ARGUMENT


def test_library_exports_the_device_setup_and_the_binding_lists_it():
    from sprsolve_amd import AMG, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    for name, nargs in (("sprs_amg_create_dev", 7), ("sprs_amg_setup_info", 4), ("sprs_amg_setup_stage_ms", 3)):
        assert hasattr(L, name) and name in _lib.all_symbols() and len(_lib.PROTOTYPES[name]) == nargs
    assert L.sprs_amg_create_dev(None, 0.08, 256, 16, 0, None, None) == _lib.INVALID_ARGUMENT    # null handles never reach the device
    assert L.sprs_amg_setup_info(None, None, None, 0) == _lib.INVALID_ARGUMENT
    import inspect
    assert {"setup", "seed"} <= set(inspect.signature(AMG.new).parameters)
