"""Knob bicg_k5 (csrc/bicgstab.hip "K5 on the chains", csrc/spmv_chain.hip UPD): BiCGStab's last update walks the chains.

Flavour 1 ("recompute"): K4 keeps its two dots and stores no t; K5 stages s in its windows as K4 did and folds t = A s again for its
own rows.  Flavour 2 ("stored"): K4 stores t, K5 walks the chains all the same and loads t.  The two share one walk and one grouping
of K5's dots, and the fold over the same window contents gives K4's bits, so they must agree BIT FOR BIT over whole solves — that
pins the recomputation.  Against flavour 0 (the vector-kernel K5) only the grouping of |r'|^2 and r0.r' differs: alpha and w of an
iteration come from K2's / K4's unchanged dots, so x after ONE iteration is bit-identical, and longer solves agree the way the chain
and tile plans do (test_gpu_dict_stream.py::test_plane_streaming_chains_bit_identical).

Shapes: the smallest at which the chain kernel can go wrong — _chain_cases()'s three 3-D grids (no drift; cfg 5's line length with
seams in every block and an 80-row drift; an 8-row drift) and three seeded random grids of test_fused_spmv_input_randomised's
ranges.  Each case's solves run once (module cache) and serve every test."""
import numpy as np
import pytest

from _special import assert_same_special, bits

pytestmark = pytest.mark.gpu

_KNOBS = ("spmv_chain", "spmv_tile", "spmv_fuse", "bicg_k5")


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


def _grids():
    rng = np.random.default_rng(31)
    out = {"p3_160x128x24": (160, 128, 24), "p3_500x100x14_seams_drift": (500, 100, 14), "p3_250x84x20_drift": (250, 84, 20)}
    for k in range(3):
        nx = int(rng.integers(75, 126)) * 2; ny = int(rng.integers(60, 91)); nz = int(rng.integers(18, 27))
        out["random%d_%dx%dx%d" % (k, nx, ny, nz)] = (nx, ny, nz)
    return out


CASES = _grids()

# (right-hand side, initial guess, max_iter, tol): _fused_against_five_launches' list (test_gpu_dict_stream.py)
SOLVES = (("rhs", None, 3000, 1e-10), ("rhs2", "x0", 3000, 1e-9), ("rhs2", None, 37, 0.0), ("rhs", None, 1, 0.0),
          ("rhs2", None, 2, 0.0), ("rhs", None, 3000, 0.5), ("rhs", None, 700, 0.0))
CONVERGING = (0, 1, 5)          # positions in SOLVES of the solves with tol > 0
ONE_ITERATION = 3
RESTART_POLLS = (16, 5, 2)      # ... and the 700-iteration run again untraced at these poll intervals


def _solve(sa, A, n, b, start, max_iter, tol, trace):
    s = sa.BiCGStab.new(A, n); s.set_profile(True)
    if trace:
        s.set_trace(64)
    x = np.zeros(n) if start is None else start.copy()
    try:
        its, rr = s.solve(b, x, max_iter, tol); st = "ok"
    except sa.error.InsufficientIterNum as e:
        its, rr, st = e.iters, None, "insufficient"
    except sa.error.BreakDown as e:
        its, rr, st = e.its, None, "breakdown"
    return dict(st=st, its=its, rr=rr, x=x, trace=s.trace().copy() if trace else np.zeros((0, 8)), prof=s.profile())


_cache = {}


def _runs(sa, name):
    """{flavour: [result per solve]} for flavours 1 and 2 (every solve) and 0 under spmv_fuse = 1 (the one-iteration and the
    converging solves; None elsewhere), plus the problem."""
    if name in _cache:
        return _cache[name]
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    nx, ny, nz = CASES[name]
    ip, ix, d, rhs = gen.poisson3d(nx, ny, nz)
    n = rhs.size
    rng = np.random.default_rng(5)
    vec = {"rhs": rhs, "rhs2": rng.uniform(-1, 1, n), "x0": rng.uniform(-1, 1, n), None: None}
    out = {}
    try:
        ctx.set("spmv_chain", 1); ctx.set("spmv_tile", 1); ctx.set("spmv_fuse", 1)
        A = sa.HipCsr.new((n, n), ip, ix, d)
        assert A.chain_plan()[0] >= 64, (name, A.chain_plan())
        for k5 in (1, 2, 0):
            ctx.set("bicg_k5", k5)
            res = []
            for pos, (b, start, max_iter, tol) in enumerate(SOLVES):
                if k5 == 0 and pos != ONE_ITERATION and pos not in CONVERGING:
                    res.append(None)
                    continue
                res.append(_solve(sa, A, n, vec[b], vec[start], max_iter, tol, True))
            if k5 != 0:
                for poll in RESTART_POLLS:
                    ctx.set("poll", poll)
                    res.append(_solve(sa, A, n, rhs, None, 700, 0.0, False))
                ctx.set("poll", 16)
            out[k5] = res
    finally:
        for k in _KNOBS:
            ctx.set(k, -1)
        ctx.set("poll", 16)
    _cache[name] = (out, (ip, ix, d, vec))
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_recomputed_t_is_bit_identical_to_stored_t(sa, name):
    """Flavour 1 against flavour 2: outcome, iteration count, residual, x and every traced scalar bit for bit — to convergence,
    x0 != 0, fixed iteration counts (37, 1, 2), a loose tolerance, 700 iterations at tol = 0 through the restart branch, and that run
    untraced at poll 16, 5 and 2 (odd and even numbers of idle iterations behind a restart request: the r / r' rotation)."""
    out, _ = _runs(sa, name)
    assert len(out[1]) == len(SOLVES) + len(RESTART_POLLS) == len(out[2])
    for pos, (a, b) in enumerate(zip(out[1], out[2])):
        assert (a["st"], a["its"], a["rr"]) == (b["st"], b["its"], b["rr"]), (name, pos, a["st"], a["its"], a["rr"], b["st"], b["its"], b["rr"])
        assert np.array_equal(bits(a["x"]), bits(b["x"])), (name, pos, "x differs between recomputed and stored t")
        assert np.array_equal(bits(a["trace"]), bits(b["trace"])), (name, pos, "a traced scalar differs")
        for r in (a, b):
            assert r["prof"]["chain_k5"] >= 1 and r["prof"]["fused_k4"] >= 1, (name, pos, r["prof"])
            assert r["prof"]["fused_k4"] == r["prof"]["chain_k5"], (name, pos, r["prof"])       # every K4 has its K5 on the chains
        assert a["prof"]["spmv_launches"] == b["prof"]["spmv_launches"] or a["trace"].size == 0, (name, pos)
    assert out[1][0]["st"] == "ok"


@pytest.mark.parametrize("name", list(CASES))
def test_chain_k5_against_the_vector_kernel_k5(sa, name):
    """Flavour 1 against today's three-launch flow (bicg_k5 = 0, spmv_fuse = 1).  One iteration at tol = 0: x and trace row 0 bit for
    bit (alpha and w come from unchanged dots; x after one iteration does not depend on K5's dots).  The converging solves: what the
    project asks between chains and tiles, whose dots also differ in grouping only — iteration counts within max(3, its // 4), the
    first four trace rows to rtol 1e-9 / atol 1e-12, |x - exact| < 1e-6 where the exact solution is known (rhs of gen.poisson3d: 1)."""
    out, _ = _runs(sa, name)
    a, b = out[1][ONE_ITERATION], out[0][ONE_ITERATION]
    assert b["prof"]["chain_k5"] == 0 and b["prof"]["fused_k4"] >= 1 and a["prof"]["chain_k5"] == 1, (a["prof"], b["prof"])
    assert (a["st"], a["its"]) == (b["st"], b["its"]) == ("insufficient", 1)
    assert np.array_equal(bits(a["x"]), bits(b["x"])), (name, "x after one iteration")
    assert a["trace"].shape[0] >= 1 and np.array_equal(bits(a["trace"][0]), bits(b["trace"][0])), (name, a["trace"][:1], b["trace"][:1])
    for pos in CONVERGING:
        a, b = out[1][pos], out[0][pos]
        print(name, pos, "its", a["its"], b["its"], "rr", a["rr"], b["rr"])
        assert a["st"] == b["st"] == "ok", (name, pos, a["st"], b["st"])
        assert abs(a["its"] - b["its"]) <= max(3, b["its"] // 4), (name, pos, a["its"], b["its"])
        rows = min(4, a["trace"].shape[0], b["trace"].shape[0])
        assert rows >= 1 and np.allclose(a["trace"][:rows], b["trace"][:rows], rtol=1e-9, atol=1e-12), (name, pos)
        if SOLVES[pos][0] == "rhs" and SOLVES[pos][3] <= 1e-9:
            err = float(np.max(np.abs(a["x"] - 1.0)))
            print(name, pos, "max |x - exact|", err)
            assert err < 1e-6, (name, pos, err)


@pytest.mark.parametrize("name", list(CASES))
def test_chain_k5_against_the_oracle(sa, oracle, name):
    """Where the tol = 1e-10 solve converges, x is within 1e-7 max(1, |x_ref|_inf) of the oracle's BiCGStab
    (test_fused_spmv_input_randomised's bound)."""
    out, (ip, ix, d, vec) = _runs(sa, name)
    a = out[1][0]
    assert a["st"] == "ok", (name, a["st"], a["its"])
    ref = oracle.bicgstab(ip, ix, d, vec["rhs"], np.zeros(vec["rhs"].size), SOLVES[0][2], SOLVES[0][3])
    assert ref.status == oracle.OK
    err = float(np.max(np.abs(a["x"] - ref.x)))
    print(name, "its", a["its"], "oracle", ref.its, "max |x - x_ref|", err)
    assert err <= 1e-7 * max(1.0, float(np.max(np.abs(ref.x)))), (name, err)


def test_bicg_k5_zero_is_inert(sa):
    """With the knob at 0 nothing of this flow runs: spmv_fuse 1 and 0 are bit-identical to each other, as the existing tests of the
    fused input assume, and no K5 walks the chains."""
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = gen.poisson3d(*CASES["p3_250x84x20_drift"])
    n = rhs.size
    try:
        ctx.set("spmv_chain", 1); ctx.set("spmv_tile", 1); ctx.set("bicg_k5", 0)
        assert ctx.get("bicg_k5") == 0
        A = sa.HipCsr.new((n, n), ip, ix, d)
        assert A.chain_plan()[0] >= 64
        got = []
        for fuse in (1, 0):
            ctx.set("spmv_fuse", fuse)
            got.append(_solve(sa, A, n, rhs, None, 40, 0.0, True))
        a, b = got
        assert (a["st"], a["its"], a["rr"]) == (b["st"], b["its"], b["rr"])
        assert np.array_equal(bits(a["x"]), bits(b["x"])) and np.array_equal(bits(a["trace"]), bits(b["trace"]))
        assert a["prof"]["chain_k5"] == 0 and b["prof"]["chain_k5"] == 0
        assert a["prof"]["fused_k4"] >= 1 and b["prof"]["fused_k4"] == 0
    finally:
        for k in _KNOBS:
            ctx.set(k, -1)


def test_automatic_setting_follows_spmv_fuse(sa):
    """bicg_k5 = -1: K5 walks the chains while spmv_fuse is automatic too; once a caller has set spmv_fuse = 1 — the flow that is
    bit-identical to spmv_fuse = 0 — the automatic setting means 0."""
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = gen.poisson3d(*CASES["p3_250x84x20_drift"])
    n = rhs.size
    try:
        ctx.set("spmv_chain", 1); ctx.set("spmv_tile", 1)
        A = sa.HipCsr.new((n, n), ip, ix, d)
        assert A.chain_plan()[0] >= 64
        assert ctx.get("bicg_k5") == -1 and ctx.get("spmv_fuse") == -1
        auto = _solve(sa, A, n, rhs, None, 5, 0.0, False)
        assert auto["prof"]["chain_k5"] == 5 and auto["prof"]["fused_k4"] == 5, auto["prof"]
        ctx.set("spmv_fuse", 1)
        pinned = _solve(sa, A, n, rhs, None, 5, 0.0, False)
        assert pinned["prof"]["chain_k5"] == 0 and pinned["prof"]["fused_k4"] == 5, pinned["prof"]
        ctx.set("spmv_fuse", 0)
        off = _solve(sa, A, n, rhs, None, 5, 0.0, False)
        assert off["prof"]["chain_k5"] == 0 and off["prof"]["fused_k4"] == 0, off["prof"]
    finally:
        for k in _KNOBS:
            ctx.set(k, -1)


def test_knob_range(sa):
    ctx = sa.default_ctx(0)
    try:
        for v in (0, 1, 2, -1):
            ctx.set("bicg_k5", v)
            assert ctx.get("bicg_k5") == v
        with pytest.raises(Exception):
            ctx.set("bicg_k5", 3)
    finally:
        ctx.set("bicg_k5", -1)


def test_recomputed_and_stored_t_agree_on_special_values(sa):
    """A right-hand side with a NaN, an Inf and signed zeros, 8 iterations (the style of
    test_gpu_special_values.py::test_fused_input_flows_agree_on_nan_and_inf): flavours 1 and 2 agree in outcome, iteration count and
    x bit for bit, NaN mask included — a t folded again must carry the same non-finite and zero rows as the t K4 stored."""
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = gen.poisson3d(*CASES["p3_160x128x24"])
    n = rhs.size
    rhs = rhs.copy()
    rhs[n // 3] = np.nan
    rhs[n // 2 + 7] = np.inf
    rhs[5:400:7] = -0.0
    rhs[6:400:7] = 0.0
    try:
        ctx.set("spmv_chain", 1); ctx.set("spmv_tile", 1); ctx.set("spmv_fuse", 1)
        A = sa.HipCsr.new((n, n), ip, ix, d)
        assert A.chain_plan()[0] >= 64 and A.spmv_route()["kernel"] == "Chain"
        got = {}
        for k5 in (1, 2):
            ctx.set("bicg_k5", k5)
            got[k5] = _solve(sa, A, n, rhs, None, 8, 1e-10, True)
            assert got[k5]["prof"]["chain_k5"] >= 1, got[k5]["prof"]
        a, b = got[1], got[2]
        assert (a["st"], a["its"]) == (b["st"], b["its"]), (a["st"], a["its"], b["st"], b["its"])
        assert_same_special(a["x"], b["x"], "x with t folded again against x with t stored")
        assert_same_special(a["trace"], b["trace"], "traced scalars")
    finally:
        for k in _KNOBS:
            ctx.set(k, -1)
