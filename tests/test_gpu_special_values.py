"""Non-finite, signed-zero, subnormal and overflowing data through every SpMV route and through the vector kernels.

Every other parity test feeds the kernels finite random data, on which "y is bit-identical to the oracle" cannot tell a lane or
slot that is SELECTED away from one that is multiplied by zero (0 * Inf and 0 * NaN are NaN), nor a fold that starts from +0.0
from one seeded with its first product (a row of -0.0 products).  Here each kernel `spmv_route` (csrc/spmv.hip) can return is
held to the exact data dependence of an SpMV — y[i] depends on x[j] if and only if row i stores column j — and to the oracle's
bits on zeros, subnormals and overflow; the solvers and the stand-alone vector kernels to the oracle's NaN masks and bits.
NaN is compared by MASK everywhere (tests/_special.py assert_same_special): sign and payload of a generated NaN differ
legitimately between x86 and the GPU."""
import fractions
import os
import re

import numpy as np
import pytest

import _special as S
from _special import assert_same_special, bits

pytestmark = pytest.mark.gpu
F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = (F64, C64, F32, C32)
NAME = {F64: "f64", C64: "c64", F32: "f32", C32: "c32"}

_KNOBS = ("spmv_dict", "spmv_wide", "spmv_wideload", "spmv_uniform", "spmv_triple", "spmv_seam", "spmv_period", "spmv_tile",
          "spmv_chain", "spmv_fuse", "stream_nt")

# ---------------------------------------------------------------------------------------------------- the route table
# (id, SpmvKernel, scalar types, matrix, knobs set before the handle is created, what else the handle must report)
# How a route is asserted (_assert_route): the handle's spmv_route() reports what csrc/spmv.hip's spmv_route decides for the next
# launch under the knobs in force — the kernel by name, whether the blocks are walked through an order list, whether y is stored
# non-temporally — and is cross-checked against the older reports (chain_plan / tile_plan non-zero exactly for those routes,
# wide_blocks()[0] == ceil(nrows / 128) exactly for the 128-row kernels).
# "uniform": "none" / "some" = wide_blocks()[1] == 0 / > 0; "ordered": the walk goes through an order list (XCD-period order).
ROUTES = [
    ("csr-ragged",          "Csr",      ALL,    "ragged",            dict(spmv_dict=0, spmv_wideload=0), {}),
    ("csr-rectangular",     "Csr",      ALL,    "ragged_rect",       dict(spmv_dict=0, spmv_wideload=0), {}),
    ("csr-csc-ingest",      "Csr",      (C64,), "ragged_csc",        dict(spmv_dict=0), {}),
    ("csrwide-odd-nnz",     "CsrWide",  (F64,), "ragged_odd",        dict(spmv_dict=0, spmv_wideload=1), {}),
    ("csrwide-even-nnz",    "CsrWide",  (F64,), "ragged_even",       dict(spmv_dict=0, spmv_wideload=1), {}),
    ("csrwide-csc-ingest",  "CsrWide",  (F64,), "ragged_csc",        dict(spmv_dict=0, spmv_wideload=1), {}),
    ("dict-offset-codes",   "Dict",     ALL,    "p3_random_values",  dict(spmv_dict=1, spmv_wideload=0), {"uniform": "some"}),
    ("dict-offsets-ragged", "Dict",     ALL,    "banded_ragged_random", dict(spmv_dict=1, spmv_wideload=0), {}),
    ("dict-pair-codes",     "Dict",     ALL,    "grid_pairs",        dict(spmv_dict=2, spmv_wide=0), {}),
    ("dictwide",            "DictWide", (F64,), "p3_random_values",  dict(spmv_dict=1, spmv_wideload=1), {"uniform": "some"}),
    ("dictwide-ragged",     "DictWide", (F64,), "banded_ragged_random", dict(spmv_dict=1, spmv_wideload=1), {}),
    ("pair2-plain",         "Pair2",    (F64,), "banded_ragged",     dict(spmv_dict=2, spmv_wide=1, spmv_uniform=0), {"uniform": "none"}),
    ("pair2-uniform",       "Pair2",    (F64,), "p3_300x4x3",        dict(spmv_dict=2, spmv_wide=1, spmv_uniform=1, spmv_triple=0, spmv_seam=0), {"uniform": "some"}),
    ("pair2-triple",        "Pair2",    (F64,), "p3_300x4x3",        dict(spmv_dict=2, spmv_wide=1, spmv_uniform=1, spmv_triple=1, spmv_seam=0), {"uniform": "some"}),
    ("pair2-seam",          "Pair2",    (F64,), "p3_300x6x5",        dict(spmv_dict=2, spmv_wide=1, spmv_uniform=1, spmv_seam=1), {"uniform": "more_than_without_seams"}),
    ("pair2-period-order",  "Pair2",    (F64,), "p3_160x128x12",     dict(spmv_dict=2, spmv_wide=1, spmv_period=1, spmv_tile=0), {"uniform": "some", "ordered": True}),
    ("tilepair",            "TilePair", (F64,), "p3_160x128x12",     dict(spmv_dict=2, spmv_tile=1, spmv_chain=0), {}),
    ("tilepair-seams",      "TilePair", (F64,), "p3_500x100x8",      dict(spmv_dict=2, spmv_tile=1, spmv_chain=0), {}),
    ("tilepair-window1536", "TilePair", (F64,), "p3_800x64x8",       dict(spmv_dict=2, spmv_tile=1, spmv_chain=0), {}),
    ("tileoff",             "TileOff",  (F64,), "p3_160x128x12_random", dict(spmv_dict=1, spmv_tile=1), {}),
    ("chain",               "Chain",    (F64,), "p3_160x128x24",     dict(spmv_dict=2, spmv_tile=1, spmv_chain=1), {}),
]
_CASES = [(r, dt) for r in ROUTES for dt in r[2]]
_CASE_IDS = ["%s-%s" % (r[0], NAME[dt]) for r, dt in _CASES]


def _enumerators():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sprsolve_amd", "csrc", "internal.hpp")).read()
    body = re.search(r"enum\s+class\s+SpmvKernel\s*\{(.*?)\};", src, re.S).group(1)
    return [m.group(1) for m in re.finditer(r"^\s*(\w+)\s*,", body, re.M)]


def test_route_table_names_every_spmv_kernel():
    """The table is checked against the enumerators of SpmvKernel (csrc/internal.hpp): a ninth kernel without a row fails here."""
    names = _enumerators()
    assert len(names) >= 8 and {"Csr", "Chain"} <= set(names), names
    assert {r[1] for r in ROUTES} == set(names)
    from sprsolve_amd.mat import HipCsr
    assert list(HipCsr.SPMV_KERNELS) == names            # the names spmv_route() reports are the enumerators, in their order
    for k in ("Csr", "Dict"):
        assert {dt for r in ROUTES if r[1] == k for dt in r[2]} == set(ALL), k            # all four scalar types


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


@pytest.fixture(autouse=True)
def _restore_knobs(sa):
    ctx = sa.default_ctx(0)
    grid, poll = ctx.get("grid"), ctx.get("poll")
    yield
    for k in _KNOBS:
        ctx.set(k, -1)
    ctx.set("grid", grid); ctx.set("poll", poll)


def _cast(d, dtype):
    d = d.astype(dtype)
    return d * (1 - 0.5j) if np.dtype(dtype).kind == "c" else d


def _with_nnz_parity(ip, ix, d, odd):
    if (ix.size % 2 == 1) == odd:
        return ip, ix, d
    r = int(np.flatnonzero(np.diff(ip) >= 2)[0])
    keep = np.ones(ix.size, bool); keep[ip[r]] = False
    ip = ip.copy(); ip[r + 1:] -= 1
    return ip, ix[keep], d[keep]


def _banded_ragged(n, seed, values):
    """Ragged rows inside a +-20 band, four values (pair codes) or a value per entry (offset codes) — test_wide_kernel_irregular_rows."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 13, n)
    lens[::97] = 0
    lens[5::211] = 34
    rows = []
    for r, l in enumerate(lens):
        c = r + rng.choice(np.arange(-20, 21), l, replace=False)
        rows.append(np.sort(c[(c >= 0) & (c < n)]))
    ip = np.zeros(n + 1, dtype=np.int32); np.cumsum([len(c) for c in rows], out=ip[1:])
    ix = np.concatenate(rows).astype(np.int32)
    d = rng.choice(np.array([1.0, -2.0, 0.5, 4.0]), ix.size) if values == "few" else rng.uniform(-1, 1, ix.size)
    return ip, ix, d


def _matrix(name, dtype):
    """-> dict(ip, ix, d, nrows, ncols, nx, free_col, storage) — every matrix with one column that no row references."""
    from sprsolve_amd import gen
    from test_gpu_dict_stream import _chain_cases, _tile_cases
    nx = None
    storage = "CSR"
    if name in ("ragged", "ragged_odd", "ragged_even", "ragged_csc"):
        ip, ix, d = S.ragged_csr(5000, 41, dtype, long_rows=name != "ragged_csc")
        nrows = ncols = 5000
        storage = "CSC" if name == "ragged_csc" else "CSR"
    elif name == "ragged_rect":
        ip, ix, d = S.ragged_csr(3000, 43, dtype, ncols=3300)
        nrows, ncols = 3000, 3300
    elif name == "banded_ragged":
        ip, ix, d = _banded_ragged(3001, 31, "few"); d = _cast(d, dtype); nrows = ncols = 3001
    elif name == "banded_ragged_random":
        ip, ix, d = _banded_ragged(3001, 33, "random"); d = _cast(d, dtype); nrows = ncols = 3001
    elif name == "grid_pairs":
        if np.dtype(dtype).kind == "c":
            ip, ix, d, _, _ = gen.complex_symmetric_grid(40, 50); d = d.astype(dtype); nx = 50        # the row-value slot (code 255)
        else:
            ip, ix, d, _ = gen.poisson3d(13, 11, 9); d = d.astype(dtype); nx = 13
        nrows = ncols = ip.size - 1
    else:
        m = re.match(r"p3_(\d+)x(\d+)x(\d+)", name) if name.startswith("p3_") and name[3].isdigit() else None
        if name == "p3_random_values":
            dims = (150, 9, 7)
        else:
            dims = tuple(int(v) for v in m.groups())
        key = [k for k in list(_tile_cases()) + list(_chain_cases()) if k.startswith("p3_%dx%dx%d" % dims)]
        if key:                                                   # the tile / chain tests' own generator
            ip, ix, d = ({**_tile_cases(), **_chain_cases()})[key[0]]()[:3]
        else:
            ip, ix, d, _ = gen.poisson3d(*dims)
        if name.endswith("random") or name == "p3_random_values":
            d = d * np.random.default_rng(11).uniform(0.5, 1.5, d.size)
        d = _cast(d, dtype); nx = dims[0]; nrows = ncols = ip.size - 1
    free_col = (ncols // 3) | 1
    ip, ix, d = S.drop_column(ip, ix, d, free_col)
    if name == "ragged_odd":
        ip, ix, d = _with_nnz_parity(ip, ix, d, True)
    if name == "ragged_even":
        ip, ix, d = _with_nnz_parity(ip, ix, d, False)
    return dict(ip=ip, ix=ix, d=d, nrows=nrows, ncols=ncols, nx=nx, free_col=free_col, storage=storage)


def _assert_route(A, kernel, label, ordered=None, y_nt=None):
    r = A.spmv_route()
    rep = (label, r, A.stream_format(), A.wide_blocks(), A.tile_plan(), A.chain_plan())
    assert r["kernel"] == kernel, rep
    assert r["format"] == A.stream_format()[0], rep
    assert (A.chain_plan()[0] > 0) == (kernel == "Chain"), rep
    assert (A.tile_plan()[0] > 0) == (kernel in ("TilePair", "TileOff")), rep
    if r["format"] == 2:
        assert (A.wide_blocks()[0] == (A.rows() + 127) // 128) == (kernel in ("Pair2", "TilePair", "Chain")), rep
    if ordered is not None:
        assert r["ordered"] == ordered, rep
    if y_nt is not None:
        assert r["y_nt"] == y_nt, rep
    return r


def _handle(sa, M, d, knobs, kernel, dtype, expect, label):
    """A handle of the pattern M with values d under `knobs`, its route asserted."""
    ctx = sa.default_ctx(0)
    for k, v in knobs.items():
        ctx.set(k, v)
    if M["storage"] == "CSC":
        import scipy.sparse as sp
        C = sp.csr_matrix((d, M["ix"], M["ip"]), shape=(M["nrows"], M["ncols"])).tocsc()
        A = sa.HipCsr.new((M["nrows"], M["ncols"]), C.indptr, C.indices, C.data, storage="CSC")
    else:
        A = sa.HipCsr.new((M["nrows"], M["ncols"]), M["ip"], M["ix"], d)
    _assert_route(A, kernel, label, ordered=expect.get("ordered"))
    if kernel in ("TilePair", "TileOff"):
        assert A.tile_plan()[0] >= 8, A.tile_plan()
    if kernel == "Chain":
        assert A.chain_plan()[0] >= 64, A.chain_plan()
    uni = expect.get("uniform")
    if uni == "none":
        assert A.wide_blocks()[1] == 0
    elif uni == "some":
        assert A.wide_blocks()[1] > 0, A.wide_blocks()
    elif uni == "more_than_without_seams":
        nu = A.wide_blocks()[1]
        ctx.set("spmv_seam", 0)
        B = sa.HipCsr.new((M["nrows"], M["ncols"]), M["ip"], M["ix"], d)
        assert nu > B.wide_blocks()[1], (nu, B.wide_blocks())
        ctx.set("spmv_seam", knobs["spmv_seam"])
    return A


def _ref_spmv(oracle, M, d):
    if M["storage"] == "CSC":
        # the reference multiplies a CSC matrix by scattering column after column (mat.rs:130-142): per row the same products in
        # column order — the order of the sorted CSR rows
        import scipy.sparse as sp
        C = sp.csr_matrix((d, M["ix"], M["ip"]), shape=(M["nrows"], M["ncols"])).tocsc()
        return lambda x: oracle.spmv_csc(M["nrows"], C.indptr, C.indices, C.data, x)
    return lambda x: oracle.spmv(M["ip"], M["ix"], d, x)


def _loose(oracle, M, kernel, dtype):
    """Rows of more than 96 entries take the plain kernels' wavefront-per-row path, which re-associates the sum
    (test_spmv_random_ragged): their finite values agree to that test's tolerance, RED_RTOL * sum |val * x|."""
    lens = np.diff(M["ip"])
    if kernel not in ("Csr", "CsrWide") or not (lens > 96).any():
        return None, None
    absA = oracle.spmv(M["ip"], M["ix"], np.abs(M["d"]).astype(dtype), np.ones(M["ncols"], dtype=dtype))
    rtol = 2e-5 if np.dtype(dtype) in (np.dtype(F32), np.dtype(C32)) else 1e-13
    return lens > 96, rtol * np.abs(absA) * 2.0          # (|x| <= sqrt 2 on the clean entries)


@pytest.mark.parametrize("case,dtype", _CASES, ids=_CASE_IDS)
def test_spmv_depends_on_exactly_the_stored_columns(sa, oracle, case, dtype):
    """§1, the "poison" test.  y0 = A x0 on clean random x0 is the oracle's, bit for bit (rows on the re-associating
    wavefront-per-row path: to the existing tolerance).  Then x[S] = quiet NaN / +Inf / -Inf (complex: the real part, the
    imaginary part, both) for seeded random sets S that touch 1 % - 60 % of the rows and for the structural sets of
    _special.structural_sets (x[0], x[n - 1], just outside the tile / chain x windows of half-width 512 and 1536, line seams,
    both neighbours of a triple centre, the last stored column, columns >= nrows, a column no row references):
    rows that store no column of S keep the bits of y0; the others have NaN where the oracle has NaN and its bits elsewhere;
    the fused-dot launch gives the same y and a dot that is NaN exactly when the oracle's is.  f64 routes run a second time with
    stream_nt = 1 (the non-temporal y-store flavours, at test sizes)."""
    cid, kernel, _, mname, knobs, expect = case
    ctx = sa.default_ctx(0)
    M = _matrix(mname, dtype)
    ip, ix, d, ncols = M["ip"], M["ix"], M["d"], M["ncols"]
    A = _handle(sa, M, d, knobs, kernel, dtype, expect, cid)
    ref = _ref_spmv(oracle, M, d)
    loose, ltol = _loose(oracle, M, kernel, dtype)
    x0 = S.rand_vec(ncols, dtype, 7)
    rng = np.random.default_rng(23)
    sets = [("random%d" % k, S.random_poison_set(rng, ip, ix, ncols), "random") for k in range(2)]
    sets += [(k, v, "structural") for k, v in S.structural_sets(ip, ix, M["nrows"], ncols, M["nx"]).items()]
    sets.append(("unreferenced", np.array([M["free_col"]]), "unreferenced"))
    names = {s[0] for s in sets}
    assert {"first", "last", "triple", "last_column", "unreferenced"} <= names
    if M["nx"]:
        assert {"seam_first_of_line", "seam_last_of_line"} <= names
    if M["nrows"] >= 100000:
        assert {"window_512_4096_before", "window_512_4096_after", "window_1536_4096_after", "window_512_2048_before"} <= names
    if ncols > M["nrows"]:
        assert "beyond_rows" in names
    if mname == "ragged_odd":
        assert ix.size % 2 == 1
    if mname == "ragged_even":
        assert ix.size % 2 == 0

    def spmv(x):
        y = np.full(M["nrows"], 3.0, dtype=dtype)
        if M["nrows"] == ncols:
            A.mul_vec(x, y)
            return y
        # (the checked mul_vec wants len(x) == len(y), as the reference's does, mat.rs:49-56: a rectangular matrix goes through
        # the unchecked entry point on device vectors)
        dx = sa.DevVec.from_numpy(x); dy = sa.DevVec.from_numpy(y)
        A.mul_vec_unchecked(dx, dy)
        return dy.to_numpy()

    for nt in ((0, 1) if np.dtype(dtype) == np.dtype(F64) else (-1,)):
        ctx.set("stream_nt", nt)
        _assert_route(A, kernel, cid, y_nt=(nt == 1) if nt >= 0 else None)
        y0 = spmv(x0)
        r0 = ref(x0)
        if loose is None:
            assert np.array_equal(bits(y0), bits(r0)), (cid, nt)
        else:
            assert np.array_equal(bits(y0[~loose]), bits(r0[~loose])), (cid, nt)
            assert np.all(np.abs(y0[loose] - r0[loose]) <= ltol[loose])
        for sname, cols, kind in (sets if nt != 1 else sets[1:]):
            for vname, value in S.poison_values(dtype):
                label = "%s/%s/%s/nt=%d" % (cid, sname, vname, nt)
                x, y, touched = S.check_poison(spmv, ref, ip, ix, ncols, x0, y0, cols, value, kind, label=label,
                                               loose_rows=loose, loose_tol=ltol)
                # the fused-dot epilogue: the same y, and conj(x).y NaN exactly when the oracle's is (component by component;
                # a sum that holds +Inf and -Inf, or a NaN, is NaN in any order)
                y2 = np.zeros(M["nrows"], dtype=dtype)
                if M["nrows"] == ncols:
                    dot = A.mul_vec_dot(x, y2)
                    assert_same_special(y2, y, label + ": y of mul_vec_dot")
                    want = oracle.conj_dot(x, ref(x))
                    g = S.components(np.array([dot], dtype=dtype)); w = S.components(np.array([want], dtype=dtype))
                    assert np.array_equal(np.isnan(g), np.isnan(w)), (label, "fused dot", dot, want)


@pytest.mark.parametrize("case,dtype", _CASES, ids=_CASE_IDS)
def test_spmv_signed_zero_subnormal_overflow(sa, oracle, case, dtype):
    """§2.  The same routes on the same patterns with the value variants of _special.special_variants: all-zero values and all
    -0.0 / +0.0 x (every fold is a sum of zeros on top of the reference's +0.0 start: a -0.0 anywhere means a seeded accumulator
    or a stray term), values and x at the subnormal boundary (products that stay subnormal, land exactly on the smallest subnormal,
    underflow), values near the largest finite number (partial sums overflow in the middle of a row and stay; +Inf meets -Inf:
    NaN exactly where the oracle's is), complex values Inf + 0i, 0 + Inf i, NaN + 1i.  Bit for bit, NaN by mask; rows on the
    re-associating wavefront-per-row path are compared bit for bit on the all-zero variants, by NaN mask, Inf and the existing
    tolerance on the subnormal and complex variants, and left out of the overflow variant alone (there the order of the additions
    decides whether a partial sum overflows, so even the NaN mask legitimately depends on it).  The new value of an entry is a function of its (offset, old value) pair, so a pattern of
    few pairs keeps its uniform blocks, tiles and chains: the route is asserted for every handle."""
    cid, kernel, _, mname, knobs, expect = case
    M = _matrix(mname, dtype)
    loose, _ = _loose(oracle, M, kernel, dtype)
    handles = {}
    offsets = M["ix"].astype(np.int64) - np.repeat(np.arange(M["nrows"]), np.diff(M["ip"]))
    for vname, vals, x in S.special_variants(M["d"], dtype, M["ncols"], 5, keys=offsets):
        key = id(vals) if vals is not M["d"] else 0
        if key not in handles:
            # (a pattern whose values are all +-0.0 or the same few subnormals may qualify for pair codes where the random values
            # did not, and the other way round: the knobs force the stream, and the route is asserted for every handle)
            handles[key] = _handle(sa, M, vals, knobs, kernel, dtype, {}, "%s/%s" % (cid, vname))
        A = handles[key]
        y = np.full(M["nrows"], 3.0, dtype=dtype)
        if M["nrows"] == M["ncols"]:
            A.mul_vec(x, y)
        else:
            dx = sa.DevVec.from_numpy(x); dy = sa.DevVec.from_numpy(y)
            A.mul_vec_unchecked(dx, dy)
            y = dy.to_numpy()
        want = _ref_spmv(oracle, M, vals)(x)
        label = "%s/%s" % (cid, vname)
        if loose is not None:
            # wavefront-per-row rows (more than 96 entries): the same products added in another order
            assert_same_special(y[~loose], want[~loose], label)
            if vname.startswith("zeros") or vname.endswith("0_x"):
                assert_same_special(y[loose], want[loose], label + " (long rows)")                  # a sum of zeros: any order
            elif vname != "overflow":
                # subnormal / complex_inf: whether a sum is NaN, +Inf or -Inf does not depend on the order (no finite partial sum
                # overflows here); finite sums to test_spmv_random_ragged's tolerance, rtol * sum |val x|, plus half a smallest
                # subnormal for every product and addition of the row (the rounding unit at the bottom of the range)
                fi = np.finfo(S.real_dtype(dtype))
                absA = _ref_spmv(oracle, M, np.abs(vals).astype(dtype))(np.abs(x).astype(dtype))
                absA = np.where(np.isfinite(np.abs(absA)), np.abs(absA), 0.0)
                rtol = 2e-5 if fi.bits == 32 else 1e-13
                tol = rtol * 2.0 * absA + np.diff(M["ip"]) * 4.0 * float(fi.smallest_subnormal)
                S.assert_close_special(y[loose], want[loose], tol[loose], label + " (long rows)")
        else:
            assert_same_special(y, want, label)
        if vname in ("zeros_values_neg0_x", "neg0_x"):
            assert not np.signbit(S.components(y)).any(), label


# ---------------------------------------------------------------------------------------------------- split operator
def test_split_operator_interior_and_boundary_parts(sa, oracle):
    """The Interior and Boundary launches of an operator split at creation, on one GPU through the in-process self-halo plan of
    tests/test_gpu_dist.py (a world-1 communicator; the columns above n - 3R are declared remote, so only the last row blocks
    touch the halo: "interior/boundary overlap").  Poisoned one element at a time: an owned entry that is SENT into the halo (the
    exchange overwrites the halo tail, so a halo entry is poisoned through its owner), an interior entry next to the boundary, an
    owned entry that only boundary rows read, and a halo TAIL entry before the exchange (must be overwritten: y = y0 everywhere).
    With the 64-row kernels (Dict on both parts) and with the two-rows-per-lane kernel (Pair2 on both parts) on the subsets.  The
    split is made at creation only under the context knob halo_overlap = 1 (csrc/dist.hip), which is set here and restored; that
    the handle did split, and which kernel each part takes, is asserted through spmv_route(part): both parts exist, walk their
    blocks through an order list, and together cover every row block.  Nothing here spawns a process; plans over several ranks
    are left to tests/test_gpu_dist_multirank.py."""
    import torch
    from sprsolve_amd import dist as sdist, gen
    from test_gpu_dist import _self_halo_plan
    ctx = sa.default_ctx(0)
    dev = torch.device("cuda", 0)
    comm = sdist.Comm(ctx, 0, 1)
    overlap0 = ctx.get("halo_overlap")
    try:
        ctx.set("halo_overlap", 1)
        R = 96
        ip, ix, d = gen.grid_laplacian_dirichlet(R, R)
        n = R * R
        ref = lambda x: oracle.spmv(ip, ix, d, x)
        x0 = S.rand_vec(n, F64, 3)
        for wide in (0, 1):
            ctx.set("spmv_wide", wide)
            plan = _self_halo_plan(torch, dev, n, ix, lambda c: c > n - 3 * R)
            assert plan["n_ext"] > n
            A = sdist.DistCsr.from_plan(comm, plan, int(ip[-1]), torch.from_numpy(ip).to(dev), torch.from_numpy(d).to(dev),
                                        adopt=True, to_device=lambda a: torch.from_numpy(a).to(dev))
            assert A.stream_format()[0] == 2                       # few (offset, value) pairs survive the halo renumbering
            ri, rb = A.spmv_route(1), A.spmv_route(2)
            assert ri is not None and rb is not None, "the operator was not split into interior and boundary launches"
            want_kernel = "Pair2" if wide else "Dict"
            assert ri["kernel"] == want_kernel and rb["kernel"] == want_kernel, (wide, ri, rb)
            assert ri["ordered"] and rb["ordered"] and ri["n_blocks"] > 0 and rb["n_blocks"] > 0, (ri, rb)
            assert ri["n_blocks"] + rb["n_blocks"] == (n + (127 if wide else 63)) // (128 if wide else 64), (wide, ri, rb)

            def spmv(x, tail=0.0):
                x_ext = torch.zeros(plan["n_ext"], dtype=torch.float64, device=dev)
                x_ext[:n] = torch.from_numpy(x).to(dev)
                x_ext[n:] = tail
                y = torch.full((n,), 3.0, dtype=torch.float64, device=dev)
                A.mul_vec_ext(x_ext, y)
                return y.cpu().numpy()

            y0 = spmv(x0)
            assert np.array_equal(bits(y0), bits(ref(x0)))
            for tail in (float("nan"), float("inf")):
                assert np.array_equal(bits(spmv(x0, tail)), bits(y0)), "a stale halo tail entry reaches y"
            first_remote = n - 3 * R + 1
            singles = {"sent into the halo": first_remote + R + 5, "first halo column": first_remote,
                       "interior, next to the boundary": first_remote - 1, "interior, one line before": first_remote - R,
                       "read by boundary rows only": n - R - 2, "last owned": n - 2, "x[0]": 1}
            for sname, col in singles.items():
                for vname, value in S.poison_values(F64):
                    S.check_poison(spmv, ref, ip, ix, n, x0, y0, np.array([col]), value, "structural",
                                   label="split/wide=%d/%s/%s" % (wide, sname, vname))
            rng = np.random.default_rng(5)
            cols = S.random_poison_set(rng, ip, ix, n)
            for vname, value in S.poison_values(F64):
                S.check_poison(spmv, ref, ip, ix, n, x0, y0, cols, value, "random", label="split/wide=%d/random/%s" % (wide, vname))
    finally:
        ctx.set("halo_overlap", overlap0)
        comm.close()


# ---------------------------------------------------------------------------------------------------- solvers
def _outcome(sa, fn):
    try:
        its, res = fn()
        return ("ok", its)
    except sa.error.InsufficientIterNum as e:
        return ("insufficient", e.iters)
    except sa.error.BreakDown as e:
        return ("breakdown", e.its)
    except sa.error.InvalidPreconditioner:
        return ("invalid_precond", None)


def _oracle_outcome(oracle, r):
    name = {oracle.OK: "ok", oracle.INSUFFICIENT_ITER: "insufficient", oracle.BREAKDOWN: "breakdown",
            oracle.INVALID_PRECOND: "invalid_precond"}[r.status]
    return (name, None if name == "invalid_precond" else r.its)


def _solver_problems():
    from sprsolve_amd import gen
    out = {}
    ip, ix, d, rhs = gen.minres_grid_laplacian(24, 24)
    out["f64"] = (ip, ix, d, rhs, np.abs(d[np.flatnonzero(ix == np.repeat(np.arange(rhs.size), np.diff(ip)))]) + 1.0)
    ip, ix, d, rhs, diag = gen.complex_symmetric_grid(20, 24)
    out["c64"] = (ip, ix, d, rhs, np.abs(diag) + 1.0 if diag is not None else np.full(rhs.size, 4.0))
    ip, ix, d, rhs = gen.minres_grid_laplacian(20, 20)
    out["f32"] = (ip, ix, d.astype(F32), rhs.astype(F32), None)
    return out


@pytest.mark.parametrize("what", ["nan_in_rhs", "inf_in_matrix"])
@pytest.mark.parametrize("mode", ["fused", "literal"])
@pytest.mark.parametrize("solver", ["bicgstab", "minres", "csminres"])
def test_solvers_follow_the_oracle_through_nan_and_inf(sa, oracle, solver, mode, what):
    """§3.  One NaN in the right-hand side, or one Inf in a matrix value; max_iter = 12 on a few hundred rows.  Every `res < tol`
    comparison against NaN is false on both sides, so both run to max_iter or leave through the same breakdown branch: the outcome
    (Ok / InsufficientIterNum / BreakDown / InvalidPreconditioner), the iteration count and the NaN mask of the returned x must be
    the oracle's under set_reduction_order("gpu", grid).  f64 and c64, plain and Jacobi-preconditioned (real diagonal; CSMINRES
    has no preconditioned form), plus one f32 case."""
    ctx = sa.default_ctx(0)
    cls = {"bicgstab": sa.BiCGStab, "minres": sa.MinRes, "csminres": sa.CSMinRes}[solver]
    orc = getattr(oracle, solver)
    oracle.set_reduction_order("gpu", ctx.get("grid"))
    try:
        for tname, (ip, ix, d, rhs, diag) in _solver_problems().items():
            n = rhs.size
            d = d.copy(); rhs = rhs.copy()
            if what == "nan_in_rhs":
                rhs[n // 3] = np.nan
            else:
                d[int(ip[n // 2])] = np.inf
            A = sa.HipCsr.new((n, n), ip, ix, d)
            for jac in ((False, True) if (diag is not None and solver != "csminres") else (False,)):
                x = np.zeros(n, dtype=d.dtype)
                s = cls.new(A, n); s.set_mode(mode)
                if jac:
                    P = sa.DiagPrecond.new(diag.astype(S.real_dtype(d.dtype)), t_dtype=d.dtype)
                    got = _outcome(sa, lambda: s.precond_solve(P, rhs, x, 12, 1e-10))
                    r = orc(ip, ix, d, rhs, np.zeros(n, dtype=d.dtype), 12, 1e-10, precond_diag=diag.astype(S.real_dtype(d.dtype)))
                else:
                    got = _outcome(sa, lambda: s.solve(rhs, x, 12, 1e-10))
                    r = orc(ip, ix, d, rhs, np.zeros(n, dtype=d.dtype), 12, 1e-10)
                want = _oracle_outcome(oracle, r)
                label = (solver, mode, what, tname, jac)
                assert got == want, (label, got, want)
                assert np.array_equal(np.isnan(S.components(x)), np.isnan(S.components(r.x))), (label, "NaN mask of x")
    finally:
        oracle.set_reduction_order("reference")


@pytest.mark.parametrize("dtype", [C64, C32], ids=["c64", "c32"])
def test_csminres_three_iterations_from_a_poisoned_guess(sa, oracle, dtype):
    """CSMINRES multiplies by conj(q) through the conjugated gather (conj_x = true) — the only launches with it.  Three iterations
    from an initial guess with poisoned entries (NaN in a real part, Inf in an imaginary part): outcome, iteration count and the
    NaN mask of x as the oracle's; plain stream, offset codes and pair codes."""
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs, _ = gen.complex_symmetric_grid(20, 24)
    d = d.astype(dtype); rhs = rhs.astype(dtype)
    n = rhs.size
    x0 = np.zeros(n, dtype=dtype)
    S.components(x0)[n // 4, 0] = np.nan
    S.components(x0)[n // 2, 1] = np.inf
    oracle.set_reduction_order("gpu", ctx.get("grid"))
    try:
        r = oracle.csminres(ip, ix, d, rhs, x0, 3, 1e-10)
        want = _oracle_outcome(oracle, r)
        for knob in (0, 1, 2):
            ctx.set("spmv_dict", knob)
            A = sa.HipCsr.new((n, n), ip, ix, d)
            assert A.stream_format()[0] == knob
            for mode in ("fused", "literal"):
                x = x0.copy()
                s = sa.CSMinRes.new(A, n); s.set_mode(mode)
                got = _outcome(sa, lambda: s.solve(rhs, x, 3, 1e-10))
                assert got == want, (knob, mode, got, want)
                assert np.array_equal(np.isnan(S.components(x)), np.isnan(S.components(r.x))), (knob, mode)
    finally:
        oracle.set_reduction_order("reference")


@pytest.mark.parametrize("what", ["nan_in_rhs", "inf_in_matrix"])
def test_fused_input_flows_agree_on_nan_and_inf(sa, oracle, what):
    """The fused-input chain flow of BiCGStab (K2f / K4f, spmv_fuse = 1) against the five-launch flow (spmv_fuse = 0) on the chain
    matrix of test_fused_spmv_input_is_bit_identical, and MINRES / CSMINRES with "M3 deferred" (the dict_scaled launch) on and
    off on the matrices of test_minres_m3_inside_m1_is_bit_identical: outcome, iteration count and x (assert_same_special) agree,
    8 iterations.  The only place these launches see non-finite data, so that they ARE the launches taken is asserted from the
    solver's profile on the fused side of every case (fused_k2 / fused_k4 > 0; none on the unfused side), and that the chain
    plan is still there with the Inf among the values (one new (offset, value) pair; the row's block leaves its tile)."""
    from test_gpu_dict_stream import _chain_cases, _m3_cases
    ctx = sa.default_ctx(0)

    def run(cls, A, n, rhs, dtype):
        out = {}
        for fuse in (1, 0):
            ctx.set("spmv_fuse", fuse)
            s = cls.new(A, n); s.set_profile(True)
            x = np.zeros(n, dtype=dtype)
            got = _outcome(sa, lambda: s.solve(rhs, x, 8, 1e-10))
            out[fuse] = (got, x, s.profile())
        assert out[1][0] == out[0][0], (out[1][0], out[0][0])
        assert_same_special(out[1][1], out[0][1], "x of the fused flow against the unfused one")
        return out

    def spoil(ip, d, rhs):
        d = d.copy(); rhs = rhs.copy()
        n = rhs.size
        if what == "nan_in_rhs":
            rhs[n // 3] = np.nan
        else:
            d[int(ip[n // 2]) + 1] = np.inf
        return d, rhs

    ip, ix, d, rhs, _ = _chain_cases()["p3_160x128x24"]()
    d, rhs = spoil(ip, d, rhs)
    n = rhs.size
    ctx.set("spmv_chain", 1); ctx.set("spmv_tile", 1)
    A = sa.HipCsr.new((n, n), ip, ix, d)
    assert A.chain_plan()[0] >= 64 and A.spmv_route()["kernel"] == "Chain", (what, A.chain_plan(), A.spmv_route())
    out = run(sa.BiCGStab, A, n, rhs, F64)
    assert out[1][2]["fused_k4"] >= 1 and out[1][2]["fused_k2"] >= 1, out[1][2]
    assert out[0][2]["fused_k4"] == 0 and out[0][2]["fused_k2"] == 0, out[0][2]
    ctx.set("spmv_chain", -1); ctx.set("spmv_tile", -1)
    for name in ("banded_f64_offsets", "complex_symmetric_offsets"):
        kind, ip, ix, d, rhs, knob = _m3_cases()[name]()
        d, rhs = spoil(ip, d, rhs)
        n = rhs.size
        ctx.set("spmv_dict", knob)
        A = sa.HipCsr.new((n, n), ip, ix, d)
        assert A.stream_format()[0] in (1, 2)
        out = run(sa.MinRes if kind == "minres" else sa.CSMinRes, A, n, rhs, d.dtype)
        assert out[1][2]["fused_k2"] > 0, (name, what, "M3 was not deferred into the scaled SpMV", out[1][2])
        assert out[0][2]["fused_k2"] == 0
        ctx.set("spmv_dict", -1)


# ---------------------------------------------------------------------------------------------------- vector kernels
BLOCK = 256          # threads per workgroup: csrc/internal.hpp:19
RED_UNROLL = 4       # packs a reduction thread loads per trip: csrc/blas1.hip:140


def _pk(dtype):
    """Elements per 16-byte pack, pack_width<T> (csrc/device.hpp:236): f64 2, c64 1, f32 4, c32 2."""
    return 16 // np.dtype(dtype).itemsize


def _special_list(dtype):
    fi = np.finfo(S.real_dtype(dtype))
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.tiny, -fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal,
                     fi.max, -fi.max, 1.0, -2.5], dtype=fi.dtype)


def _cycled(dtype, n, rot):
    """The special list cycled over n elements, rotated by `rot`; complex: each component cycles, the imaginary one shifted by
    one more for every pass through the list, so that every pair of values occurs."""
    v = _special_list(dtype)
    i = np.arange(n)
    re = v[(i + rot) % v.size]
    if np.dtype(dtype).kind != "c":
        return re.astype(dtype)
    out = np.empty(n, dtype=dtype)
    c = S.components(out); c[:, 0] = re; c[:, 1] = v[(i + i // v.size + rot + 3) % v.size]
    return out


class _View:
    """A device vector that starts `off` bytes into an allocation (off = 8: the element-wise kernels' scalar-access path)."""

    def __init__(self, sa, host, off):
        self.off, self.n, self.np_dtype = off, host.size, host.dtype
        raw = np.zeros((off + host.nbytes + 23) // 8 * 8, dtype=np.uint8)
        raw[off:off + host.nbytes] = host.view(np.uint8)
        self.base = sa.DevVec.from_numpy(raw.view(np.float64))
        self.is_cuda, self.dtype = True, str(host.dtype)

    def data_ptr(self):
        return self.base.ptr.value + self.off

    def numel(self):
        return self.n

    def get(self):
        raw = self.base.to_numpy().view(np.uint8)
        return raw[self.off:self.off + self.n * self.np_dtype.itemsize].view(self.np_dtype).copy()


def _scalars(dtype):
    fi = np.finfo(S.real_dtype(dtype))
    reals = [0.0, -0.0, 1.0, -1.0, float("inf"), float("nan"), float(fi.tiny), float(S.rand_vec(1, S.real_dtype(dtype), 77)[0])]
    if np.dtype(dtype).kind != "c":
        return reals
    return [complex(r, 0.0) for r in reals] + [complex(0.0, float("inf")), complex(float("nan"), 1.0), complex(-0.0, -0.0),
                                               complex(S.rand_vec(1, dtype, 78)[0])]


@pytest.mark.parametrize("off", [0, 8], ids=["aligned", "offset8"])
@pytest.mark.parametrize("dtype", ALL, ids=S.ALL_IDS)
def test_elementwise_kernels_on_special_values(sa, oracle, dtype, off):
    """§4, element-wise: axpy (and the real-scalar-on-complex form), axpby, scale, rscale, conj and the Jacobi apply on a vector
    that cycles through +-0.0, +-Inf, NaN, +-tiny, +-smallest subnormal, +-max, 1.0, -2.5 (complex: in each component), with
    the scalars +-0.0, 1, -1, Inf, NaN, tiny and a random one, on 16-byte aligned device vectors and on views 8 bytes into an
    allocation (the scalar-access kernels).  Against the oracle's element-wise functions through assert_same_special.

    Length: n = 3 * BLOCK * PK + 1 with BLOCK = 256 (csrc/internal.hpp:19) and PK = the 16-byte pack width of the type
    (csrc/device.hpp:236) — three workgroups' worth of full packs and a pack tail of one element (ew_kernel, csrc/blas1.hip:80-86,
    walks n / PK packs and then the n % PK tail elements one per thread).  The list has 13 values; instead of relying on how 13
    falls against 256 * PK, the vector is ROTATED through all 13 phases, so that every value lands on every position: the tail
    element, the first and last element of every pack and of every workgroup's block."""
    va = sa.vecalg
    pk = _pk(dtype)
    n = 3 * BLOCK * pk + 1
    nvals = _special_list(dtype).size
    cx = np.dtype(dtype).kind == "c"
    rdt = S.real_dtype(dtype)

    def dev(h):
        return _View(sa, h, off) if off else sa.DevVec.from_numpy(h)

    def host(v):
        return v.get() if off else v.to_numpy()

    for rot in range(nvals):
        x = _cycled(dtype, n, rot)
        y = _cycled(dtype, n, (rot * 5 + 2) % nvals)[::-1].copy()
        label = "%s/off%d/rot%d" % (NAME[dtype], off, rot)
        dx = dev(x)
        out = dev(np.zeros(n, dtype=dtype)); va.conj(dx, out)
        assert_same_special(host(out), oracle.conj(x), label + "/conj")
        for a in _scalars(dtype):
            dy = dev(y); va.axpy(a, dx, dy)
            assert_same_special(host(dy), oracle.axpy(a, x, y.copy()), "%s/axpy a=%r" % (label, a))
            b = _scalars(dtype)[(rot + 3) % len(_scalars(dtype))]
            dy = dev(y); va.axpby(a, dx, b, dy)
            assert_same_special(host(dy), oracle.axpby(a, x, b, y.copy()), "%s/axpby a=%r b=%r" % (label, a, b))
            dz = dev(x); va.scale(a, dz)
            assert_same_special(host(dz), oracle.scale(a, x.copy()), "%s/scale a=%r" % (label, a))
        for a in _scalars(rdt):
            dz = dev(x); va.rscale(a, dz)
            assert_same_special(host(dz), oracle.rscale(a, x.copy()), "%s/rscale a=%r" % (label, a))
            if cx:
                dy = dev(y); va.axpy(float(a), dx, dy)                  # S = Real, T = Complex
                assert_same_special(host(dy), oracle.axpy(float(a), x, y.copy()), "%s/axpy real a=%r" % (label, a))
        # Jacobi: set-up (1 / d: 1/0, 1/subnormal -> Inf, 1/max -> subnormal, 1/Inf, 1/NaN) and apply
        diags = [y.real.astype(rdt).copy() if cx else y.copy()] + ([y.copy()] if cx else [])
        for dg in diags:
            P = sa.DiagPrecond.new(dg, t_dtype=dtype)
            dinv = oracle.diag_inv(dg)
            dout = dev(np.zeros(n, dtype=dtype))
            P.mul_vec_unchecked(dx, dout)
            assert_same_special(host(dout), oracle.diag_apply(dinv, x), "%s/jacobi %s" % (label, dg.dtype))
            if not cx:
                ones = np.ones(n, dtype=dtype); P.mul_vec_unchecked(dev(ones), dout)
                assert_same_special(host(dout), dinv, "%s/1 / d" % label)      # 1 * (1 / d): the set-up kernel's own bits


def _red_grid(n, pk, g0):
    """balanced_grid (csrc/internal.hpp) of a reduction over n elements in packs of pk."""
    work = (n // pk + BLOCK - 1) // BLOCK
    if work <= g0:
        return max(work, 1)
    trips = (work + g0 - 1) // g0
    return min(((work + trips - 1) // trips + 7) & ~7, g0)


def _reduction_sizes(pk, g0):
    """{name: n}: (a) three grid-stride trips — the remainder loop only; (b) exactly 2 unrolled trips of RED_UNROLL packs;
    (c) one unrolled trip + two remainder trips, the last one partial, + a pack tail."""
    st = g0 * BLOCK
    return {"remainder_only": (3 * st - 5) * pk + (pk - 1), "two_unrolled_trips": 2 * RED_UNROLL * st * pk,
            "unrolled_remainder_tail": ((RED_UNROLL + 2) * st - 3) * pk + (pk - 1)}


def _positions(n, pk, g0):
    g = _red_grid(n, pk, g0)
    st = g * BLOCK
    npk = n // pk
    k = 0
    while k * RED_UNROLL * st + (RED_UNROLL - 1) * st < npk:      # trips the first thread makes through the unrolled loop
        k += 1
    unrolled = k * RED_UNROLL * st                                # packs below this index: handled by unrolled trips of SOME thread
    p = {0, pk - 1, pk, (npk - 1) * pk, npk * pk - 1, n - 1,
         BLOCK * pk, 2 * BLOCK * pk - 1, st * pk - 1, st * pk}     # a workgroup's first stride: first / last element; the grid's
    p |= {npk * pk + t for t in range(n % pk)}                      # every element of the pack tail
    if k:
        p |= {(RED_UNROLL - 1) * st * pk, min(unrolled, npk) * pk - 1}      # unrolled loop: its 4th pack of thread 0, its last element
    if unrolled < npk:
        p |= {unrolled * pk, (npk - 1) * pk}                        # remainder loop: first and last pack
    return sorted(q for q in p if 0 <= q < n)


@pytest.mark.parametrize("dtype", ALL, ids=S.ALL_IDS)
def test_reductions_single_element_sensitivity(sa, oracle, dtype):
    """§4, reductions, exact: x = 0 but x[p] = 1, y = seeded small integers: dot(x, y) and conj_dot(x, y) must be y[p] and norm2(x)
    1.0 EXACTLY, for p at 0, PK - 1, PK, the last full pack, every element of the pack tail, the first / last element of a
    workgroup's first stride, the first / last element the 4-way unrolled loop (RED_UNROLL, csrc/blas1.hip:140) and the remainder
    loop handle, and n - 1 — an element a loop bound drops, or counts twice, cannot hide.  Sizes from the context's "grid" knob:
    three trips (remainder loop only), exactly two unrolled trips, one unrolled + two remainder trips + a pack tail; each with
    stream_nt 0 and 1 (the NT = true instantiations of dot_kernel / nrm2sq_kernel without 72 MB operands), and one size of 72 MB
    with the knob at -1 (the automatic choice)."""
    import torch
    ctx = sa.default_ctx(0)
    va = sa.vecalg
    dev = torch.device("cuda", 0)
    tdt = {F64: torch.float64, C64: torch.complex128, F32: torch.float32, C32: torch.complex64}[dtype]
    pk = _pk(dtype)
    g0 = ctx.get("grid")
    sizes = dict(_reduction_sizes(pk, g0))
    sizes["72MB_automatic"] = (72 << 20) // np.dtype(dtype).itemsize + pk + 1
    cx = np.dtype(dtype).kind == "c"
    for sname, n in sizes.items():
        rng = np.random.default_rng(n % 1000)
        yh = rng.integers(-8, 9, n).astype(dtype)
        if cx:
            yh = yh + 1j * rng.integers(-8, 9, n).astype(dtype)
            yh = yh.astype(dtype)
        y = torch.from_numpy(yh).to(dev)
        x = torch.zeros(n, dtype=tdt, device=dev)
        pos = _positions(n, pk, g0)
        if sname == "unrolled_remainder_tail":
            assert n % pk == pk - 1 and len(pos) >= 10 + (pk - 1)
        for nt in ((-1,) if sname == "72MB_automatic" else (0, 1)):
            ctx.set("stream_nt", nt)
            assert va.norm2(x) == 0.0 and va.dot(x, y) == 0
            for p in pos:
                x[p] = 1.0
                torch.cuda.synchronize()
                label = (NAME[dtype], sname, n, nt, p)
                assert va.dot(x, y) == yh[p], label
                assert va.conj_dot(x, y) == yh[p], label
                assert va.dot(y, x) == yh[p], label
                assert va.norm2(x) == 1.0, label
                x[p] = 0.0
        del x, y
    ctx.set("stream_nt", -1)


@pytest.mark.parametrize("dtype", ALL, ids=S.ALL_IDS)
def test_reductions_on_special_values(sa, oracle, dtype):
    """§4, reductions, special values.  With the "grid" knob at 64 (smaller vectors for the oracle's emulation; the sizes are
    derived from it as above) one NaN, then one Inf at each structural position: dot, conj_dot and norm2 must be what
    oracle.*_gpu_order says (NaN by mask, Inf by bits), with stream_nt 0 and 1.  norm2 of a vector whose squares overflow is Inf;
    norm2 of a vector with a single subnormal equals the oracle's bit for bit; conj_dot of an all -0.0 x with a positive y has the
    oracle's sign of zero."""
    ctx = sa.default_ctx(0)
    va = sa.vecalg
    g0 = 64
    ctx.set("grid", g0)
    oracle.set_reduction_order("gpu", g0)
    pk = _pk(dtype)
    rdt = S.real_dtype(dtype)
    fi = np.finfo(rdt)
    one = lambda v, dt: np.array([v], dtype=dt)
    try:
        for sname, n in _reduction_sizes(pk, g0).items():
            x0 = S.rand_vec(n, dtype, 5); y0 = S.rand_vec(n, dtype, 6)
            dx = sa.DevVec.from_numpy(x0); dy = sa.DevVec.from_numpy(y0)
            for p in _positions(n, pk, g0):
                for special in (np.nan, np.inf):
                    x = x0.copy(); x[p] = special
                    dx.upload(x)
                    wd = oracle.conj_dot_gpu_order(x, y0); wn = oracle.norm2_gpu_order(x)
                    # dot(x, y) = conj_dot(conj(x), y) term by term: conj(conj(x)) is x bit for bit, so the oracle's fold of
                    # conj(x) in the kernels' order is the unconjugated dot's
                    wu = oracle.conj_dot_gpu_order(np.conj(x), y0)
                    for nt in (0, 1):
                        ctx.set("stream_nt", nt)
                        label = "%s/%s/p=%d/%r/nt=%d" % (NAME[dtype], sname, p, special, nt)
                        assert_same_special(one(va.conj_dot(dx, dy), dtype), one(wd, dtype), label + "/conj_dot")
                        assert_same_special(one(va.dot(dx, dy), dtype), one(wu, dtype), label + "/dot")
                        assert_same_special(one(va.norm2(dx), rdt), one(wn, rdt), label + "/norm2")
            dx.free(); dy.free()
        ctx.set("stream_nt", -1)
        n = 5 * g0 * BLOCK * pk + 3
        big = np.full(n, fi.max / 4, dtype=dtype)
        assert va.norm2(big) == np.inf and oracle.norm2_gpu_order(big) == np.inf
        big[::2] = 1.0                                         # overflow in some partials only
        assert_same_special(one(va.norm2(big), rdt), one(oracle.norm2_gpu_order(big), rdt), "norm2 overflow")
        for v in (fi.smallest_subnormal, fi.tiny, np.sqrt(fi.tiny) * 1.5, np.sqrt(fi.smallest_subnormal) * 2):
            sub = np.zeros(n, dtype=dtype); sub[n // 3] = v
            assert_same_special(one(va.norm2(sub), rdt), one(oracle.norm2_gpu_order(sub), rdt), "norm2 of a single %r" % v)
        neg = np.full(n, -0.0, dtype=dtype); pos = np.full(n, 2.0, dtype=dtype)
        assert_same_special(one(va.conj_dot(neg, pos), dtype), one(oracle.conj_dot_gpu_order(neg, pos), dtype), "dot of -0.0")
        if np.dtype(dtype).kind != "c":                        # (real scalars: dot is conj_dot)
            assert_same_special(one(va.dot(neg, pos), dtype), one(oracle.conj_dot_gpu_order(neg, pos), dtype), "dot of -0.0")
    finally:
        oracle.set_reduction_order("reference")


def _exact_conj_dot(x, y):
    """sum conj(x_i) y_i in exact rational arithmetic, rounded once to double components."""
    F = fractions.Fraction
    if x.dtype.kind != "c":
        return float(sum(F(float(a)) * F(float(b)) for a, b in zip(x, y)))
    xr, xi, yr, yi = [[F(float(v)) for v in arr] for arr in (x.real, x.imag, y.real, y.imag)]
    re = sum(a * c + b * d for a, b, c, d in zip(xr, xi, yr, yi))
    im = sum(a * d - b * c for a, b, c, d in zip(xr, xi, yr, yi))
    return complex(float(re), float(im))


@pytest.mark.parametrize("dtype", ALL, ids=S.ALL_IDS)
def test_conj_dot_accuracy_on_an_ill_conditioned_sum(sa, oracle, dtype):
    """§4, accuracy.  The oracle is a same-precision fold, so agreeing with it says nothing about accuracy.  An ill-conditioned dot
    product — a seeded vector, its permuted copy against the negated partner (these cancel exactly) and a small remainder:
    sum |x_i y_i| / |sum x_i y_i| about 1e8 — against the exact value (rational arithmetic on the inputs, rounded once).  No
    invented tolerance: the error of the GPU's tree sum must be at most twice the error of oracle.conj_dot, the reference's serial
    fold, on the same data (the margin is there because the tree is expected to be the MORE accurate side, as
    test_vecalg_random_vs_oracle notes for f32 — not to excuse a worse result).
    Measured on an MI355X, absolute errors (GPU tree, serial fold), condition number in brackets:
    f64 1.0e-14, 7.7e-14 (7e7); c64 2.4e-14, 2.4e-13 (2e8); f32 6.1e-6, 1.3e-4 (7e7); c32 1.5e-5, 3.9e-5 (2e8)."""
    rng = np.random.default_rng(1234)
    m = 12000
    a = S.rand_vec(m, dtype, 1); b = S.rand_vec(m, dtype, 2)
    perm = rng.permutation(m)
    r = 64
    xr = S.rand_vec(r, dtype, 3); yr = (S.rand_vec(r, dtype, 4) * 2e-5).astype(dtype)
    x = np.concatenate([a, a[perm], xr]).astype(dtype)
    y = np.concatenate([b, -b[perm], yr]).astype(dtype)
    mix = rng.permutation(x.size)
    x, y = x[mix].copy(), y[mix].copy()
    exact = _exact_conj_dot(x, y)
    mag = float(np.sum(np.abs(x).astype(np.float64) * np.abs(y).astype(np.float64)))
    cond = mag / abs(exact)
    assert 1e6 < cond < 1e10, cond
    gpu = sa.vecalg.conj_dot(x, y)
    ser = oracle.conj_dot(x, y)
    e_gpu, e_ser = abs(gpu - exact), abs(ser - exact)
    print("conj_dot accuracy %s: cond %.3g, GPU error %.3e, serial-fold error %.3e (of sum|x y| = %.3e)" % (NAME[dtype], cond, e_gpu, e_ser, mag))
    assert e_gpu <= 2.0 * e_ser, "GPU error %.3e, serial-fold (oracle.conj_dot) error %.3e, exact %r" % (e_gpu, e_ser, exact)


def test_spmv_fuzz_with_special_values(oracle):
    """scripts/fuzz_spmv.py with its opt-in special_prob: random structured matrices through the full knob product, 3 % of the
    entries of x and of the values replaced by zeros, infinities, NaN, subnormals and the largest finite numbers: y as the oracle's
    (NaN by mask).  The committed fuzz slice (tests/test_gpu_fuzz_slice.py) keeps its calls and its data."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_spmv", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "fuzz_spmv.py"))
    F = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(F)
    r = F.run(budget=2.0, seed=21, big_prob=0.05, special_prob=0.03)
    assert r["mismatch"] is None, r["mismatch"] and r["mismatch"]["text"]
    assert r["combos"] >= 50, r
