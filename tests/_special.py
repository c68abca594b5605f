"""Helpers of the special-value tests (tests/test_gpu_special_values.py on the GPU, their oracle-only twins in
tests/test_oracle_golden.py): NaN-aware comparison, poison values and poison sets, the exact-data-dependence check of
an SpMV, and the matrices / value variants both files multiply.  Pure numpy: nothing here needs a GPU."""
import numpy as np

ALL_DTYPES = [np.float64, np.complex128, np.float32, np.complex64]
ALL_IDS = ["f64", "c64", "f32", "c32"]

# a randomly poisoned case must touch between 1 % and 60 % of the rows: below, the touched-row assertion is (nearly) vacuous;
# above, the untouched-row one is
TOUCHED_MIN, TOUCHED_MAX = 0.01, 0.60


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def real_dtype(dtype):
    return np.dtype(dtype).type(0).real.dtype


def components(a):
    """A real view of `a`: a complex array becomes (..., 2) real components."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        return a.view(real_dtype(a.dtype)).reshape(a.shape + (2,))
    return a


def assert_same_special(got, want, label=""):
    """`got` equals `want` component by component: NaN exactly where `want` has NaN (compared by MASK — sign and payload of a
    generated NaN differ legitimately between x86 and the GPU), bit-identical everywhere else (so +-0.0, +-Inf, subnormals and
    every finite value are compared by bit pattern)."""
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    g, w = components(got), components(want)
    gn, wn = np.isnan(g), np.isnan(w)
    if not np.array_equal(gn, wn):
        k = np.argwhere(gn != wn)[0]
        raise AssertionError("%s: NaN mask differs at %s: got %r, want %r (%d components differ)"
                             % (label, tuple(k), g[tuple(k)], w[tuple(k)], int(np.sum(gn != wn))))
    ui = np.dtype("u%d" % g.dtype.itemsize)
    gb, wb = g.view(ui), w.view(ui)
    bad = (gb != wb) & ~wn
    if bad.any():
        k = np.argwhere(bad)[0]
        raise AssertionError("%s: bits differ at %s: got %r (%#x), want %r (%#x) (%d components differ)"
                             % (label, tuple(k), g[tuple(k)], int(gb[tuple(k)]), w[tuple(k)], int(wb[tuple(k)]), int(bad.sum())))


def assert_close_special(got, want, tol, label=""):
    """For sums the kernel re-associates: NaN exactly where `want` has NaN, +-Inf exactly where it has them (same sign), finite
    components within tol (one tolerance per element)."""
    g, w = components(got), components(want)
    assert np.array_equal(np.isnan(g), np.isnan(w)), (label, "NaN mask")
    inf = np.isinf(w)
    assert np.array_equal(np.isinf(g), inf) and np.array_equal(g[inf], w[inf]), (label, "Inf")
    fin = np.isfinite(w)
    t = np.broadcast_to(np.asarray(tol, dtype=np.float64).reshape((-1,) + (1,) * (g.ndim - 1)), g.shape)
    err = np.abs(g[fin].astype(np.float64) - w[fin].astype(np.float64))
    assert np.all(err <= t[fin]), (label, "finite values", float(err.max()) if err.size else 0.0)


def rand_vec(n, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "c":
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(dtype)
    return rng.uniform(-1, 1, n).astype(dtype)


def poison_values(dtype):
    """[(name, value)]: quiet NaN, +Inf, -Inf; complex: in the real part only, the imaginary part only, and both."""
    out = []
    for name, p in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        if np.dtype(dtype).kind == "c":
            out += [(name + ".re", ("re", p)), (name + ".im", ("im", p)), (name + ".both", ("both", p))]
        else:
            out.append((name, ("re", p)))
    return out


def poisoned(x0, cols, value):
    """x0 with x[cols] poisoned; `value` = (part, p) of poison_values()."""
    part, p = value
    x = x0.copy()
    cols = np.asarray(cols, dtype=np.int64)
    if x.dtype.kind != "c":
        x[cols] = p
    elif part == "re":
        x[cols] = p + 1j * x0[cols].imag
    elif part == "im":
        x[cols] = x0[cols].real + 1j * p
    else:
        xv = components(x)              # (writing p + 1j * p would compute inf * 1j: a NaN real part)
        xv[cols, 0] = p; xv[cols, 1] = p
    return x


def touched_rows(indptr, indices, cols, ncols):
    """Boolean mask of the rows that store at least one column of `cols`."""
    hit = np.zeros(ncols, dtype=bool)
    hit[np.asarray(cols, dtype=np.int64)] = True
    per_entry = hit[np.asarray(indices, dtype=np.int64)]
    cnt = np.zeros(per_entry.size + 1, dtype=np.int64)
    np.cumsum(per_entry, out=cnt[1:])
    ip = np.asarray(indptr, dtype=np.int64)
    return (cnt[ip[1:]] - cnt[ip[:-1]]) > 0


def random_poison_set(rng, indptr, indices, ncols, share=0.10):
    """A seeded set of columns that touches about `share` of the rows (between TOUCHED_MIN and TOUCHED_MAX: asserted)."""
    nrows = len(indptr) - 1
    nnz = max(1, len(indices))
    per_col = nnz / float(ncols)                                # rows a column touches on average
    k = int(min(ncols, max(1, round(share * nrows / max(per_col, 1e-9)))))
    for _ in range(50):
        cols = np.sort(rng.choice(ncols, size=k, replace=False))
        frac = touched_rows(indptr, indices, cols, ncols).mean()
        if TOUCHED_MIN <= frac <= TOUCHED_MAX:
            return cols
        k = max(1, int(k * (0.5 if frac > TOUCHED_MAX else 2.0)))
    raise AssertionError("no poison set touches between 1 %% and 60 %% of the rows (last: %.3f)" % frac)


def check_poison(spmv, ref_spmv, indptr, indices, ncols, x0, y0, cols, value, kind, label="", loose_rows=None, loose_tol=None):
    """The exact-data-dependence property for one poison set: with x = x0 but x[cols] = poison,
      * rows that store no column of `cols` give the bits of y0 = A x0 (a `0 * poison` anywhere in their fold would be NaN),
      * rows that do give what `ref_spmv` gives: NaN where it has NaN, its bits elsewhere.
    kind: "random" (the touched share must lie within [1 %, 60 %]), "structural" (>= 1 row touched) or "unreferenced"
    (no row touched: y is y0 everywhere).  loose_rows: rows whose sum the kernel re-associates (the plain CSR kernel's
    wavefront-per-row path) — there finite values are compared to loose_tol[row] instead of bit for bit; NaN and Inf as usual.
    Returns (x, y, touched)."""
    x = poisoned(x0, cols, value)
    touched = touched_rows(indptr, indices, cols, ncols)
    frac = touched.mean() if touched.size else 0.0
    if kind == "random":
        assert TOUCHED_MIN <= frac <= TOUCHED_MAX, (label, "touched share", frac)
    elif kind == "structural":
        assert touched.any(), (label, "a structural poison set must touch a row", cols[:8])
    else:
        assert not touched.any(), (label, "the unreferenced column is referenced")
    y = spmv(x)
    assert_same_special(y[~touched], y0[~touched], "%s: untouched rows" % label)
    if touched.any():
        want = ref_spmv(x)
        if loose_rows is not None and (loose_rows & touched).any():
            exact = touched & ~loose_rows
            assert_same_special(y[exact], want[exact], "%s: touched rows" % label)
            lr = np.flatnonzero(touched & loose_rows)
            assert_close_special(y[lr], want[lr], loose_tol[lr], "%s: touched re-associated rows" % label)
        else:
            assert_same_special(y[touched], want[touched], "%s: touched rows" % label)
    return x, y, touched


# ------------------------------------------------------------------------------------------------ matrices
def drop_column(indptr, indices, data, col):
    """The same matrix without the entries of column `col`: a column no row references."""
    keep = np.asarray(indices) != col
    kept = np.zeros(keep.size + 1, dtype=np.int64)
    np.cumsum(keep, out=kept[1:])
    ip = kept[np.asarray(indptr, dtype=np.int64)].astype(np.int32)
    return ip, np.asarray(indices)[keep].astype(np.int32), np.asarray(data)[keep]


def ragged_csr(n, seed, dtype, ncols=None, long_rows=True):
    """Ragged random rows: empty rows, rows of 1..9 entries, a few longer than a wavefront (97..399 entries, one of min(n, 3000))."""
    rng = np.random.default_rng(seed)
    ncols = n if ncols is None else ncols
    cnt = rng.integers(0, 10, n)
    cnt[rng.integers(0, n, max(1, n // 50))] = 0
    if long_rows and n > 400:
        for r in rng.integers(0, n, 6):
            cnt[r] = rng.integers(97, 400)
        cnt[n // 2] = min(ncols, 3000)
        cnt[n // 2 + 1] = 130
    indptr = np.zeros(n + 1, dtype=np.int64); np.cumsum(cnt, out=indptr[1:])
    indices = np.concatenate([np.sort(rng.choice(ncols, c, replace=False)) for c in cnt]) if indptr[-1] else np.zeros(0, int)
    data = rand_vec(int(indptr[-1]), dtype, seed + 1)
    return indptr.astype(np.int32), indices.astype(np.int32), data


def structural_sets(indptr, indices, nrows, ncols, nx=None):
    """{name: columns}: the poison sets that sit where the kernels clamp, mask and stage windows.
      ends            x[0] and x[ncols - 1] (one set each)
      window_*        the element just before (b - hw - 1) and just after (b + span + hw) the x window of a run of rows that starts
                      at row b, for the window half-widths hw = 512 and 1536 of the LDS-window tiles (span 4096 rows) and the
                      plane-streaming chains (span 2048): tiles and chain tiles start on 128-row block boundaries, so b runs over
                      block starts at a stride that is odd in blocks (every phase against the 32-block tiles occurs)
      seam_*          with lines of nx rows: the first / last element of a line — the column the last row of the line before
                      (the first row of the line after) lacks, its missing +1 (-1) neighbour
      triple          both neighbours c - 1, c + 1 of centre columns c, not c itself
      last_column     the last stored column (when nnz is odd the plain wide kernel's 16-byte tail group is half padding)
      beyond_rows     rectangular matrices: columns >= nrows
    Every set is a valid poison set whatever the kernels' layout: the property is checked from the pattern alone.  Only the AIM of
    the window sets is approximate — where a plan's tiles really start is not read from tile_plan / chain_plan (which report
    counts), so the candidates are spread over block starts instead."""
    sets = {"first": np.array([0]), "last": np.array([ncols - 1])}
    starts = np.arange(0, nrows, 128 * 7)
    for hw in (512, 1536):
        for span in (4096, 2048):
            lo = starts - hw - 1
            hi = starts + span + hw
            lo = lo[(lo >= 0) & (lo < ncols)]; hi = hi[(hi >= 0) & (hi < ncols)]
            if lo.size:
                sets["window_%d_%d_before" % (hw, span)] = lo
            if hi.size:
                sets["window_%d_%d_after" % (hw, span)] = hi
    if nx is not None and nx < ncols:
        line = np.arange(nx, ncols, nx)
        sets["seam_first_of_line"] = line[::3]
        sets["seam_last_of_line"] = (line - 1)[1::3]
    c = np.arange(5, ncols - 5, 257)
    if c.size:
        sets["triple"] = np.unique(np.concatenate([c - 1, c + 1]))
    if len(indices):
        sets["last_column"] = np.array([int(indices[-1])])
    if ncols > nrows:
        sets["beyond_rows"] = np.arange(nrows, ncols)[::3]
    referenced = np.zeros(ncols, dtype=bool); referenced[np.asarray(indices, dtype=np.int64)] = True
    return {k: v for k, v in sets.items() if referenced[v].any()}


# ------------------------------------------------------------------------------------------------ value variants (signed zero,
# subnormals, overflow): the SAME pattern with other values, and the x to multiply it by
def special_variants(data, dtype, ncols, seed, keys=None):
    """[(name, values, x)] on a pattern whose values are `data`.  keys (one integer per entry, e.g. column - row): the new value of an
    entry is then a function of (key, old value) alone, so that a pattern of few (offset, value) pairs keeps that structure
    (uniform blocks, tiles, chains); without keys it is drawn per entry.

      zeros_*        every value +-0.0 (the sign of `data`'s components kept) times a finite random x, an all -0.0 x and an all +0.0
                     x; the original values times all -0.0 / all +0.0: every row's fold is a sum of zeros, and the reference starts
                     its fold from +0.0
      subnormal      values cycling over +-tiny, +-tiny / 2, +-smallest subnormal, x cycling over 1, 0.5, eps, tiny, -1, 2, 0.25:
                     products that stay subnormal, land exactly on the smallest subnormal (tiny * eps), round to it or to zero
                     (tiny / 2 * eps) and underflow to zero (tiny * tiny)
      overflow       values of magnitude max / 2 and max (signs of `data`) times x of +-1 and +-2: partial sums overflow to +-Inf in
                     the middle of a row and stay there; rows where +Inf and -Inf meet are NaN
      complex_inf    (complex only) values salted with Inf + 0i, 0 + Inf i and NaN + 1i times a finite x"""
    dtype = np.dtype(dtype)
    fi = np.finfo(real_dtype(dtype))
    rng = np.random.default_rng(seed)
    cx = dtype.kind == "c"
    nnz = data.size

    def pick(k, salt):
        if keys is None:
            return rng.integers(0, k, nnz)
        h = np.ascontiguousarray(data).view(np.dtype("u%d" % (dtype.itemsize // (2 if cx else 1)))).astype(np.uint64)
        h = h.reshape(nnz, -1).sum(axis=1, dtype=np.uint64) if cx else h
        h = (h ^ (h >> np.uint64(29))) * np.uint64(0x9E3779B97F4A7C15) + (np.asarray(keys).astype(np.int64).astype(np.uint64) + np.uint64(salt)) * np.uint64(0xBF58476D1CE4E5B9)
        return ((h >> np.uint64(33)) % np.uint64(k)).astype(np.int64)

    def cplx(re, im):
        out = np.empty(re.shape, dtype=dtype)
        v = components(out); v[..., 0] = re; v[..., 1] = im
        return out

    def sign_of(a):
        return np.where(np.signbit(a), -1.0, 1.0)

    re_s = sign_of(data.real if cx else data)
    im_s = sign_of(data.imag) if cx else None
    x_fin = rand_vec(ncols, dtype, seed + 1)
    zeros = cplx(re_s * 0.0, im_s * 0.0) if cx else (re_s * 0.0).astype(dtype)
    neg0 = cplx(np.full(ncols, -0.0), np.full(ncols, -0.0)) if cx else np.full(ncols, -0.0, dtype=dtype)
    pos0 = np.zeros(ncols, dtype=dtype)
    out = [("zeros_values", zeros, x_fin), ("zeros_values_neg0_x", zeros, neg0), ("zeros_values_pos0_x", zeros, pos0),
           ("neg0_x", data, neg0), ("pos0_x", data, pos0)]
    sub = np.array([fi.tiny, -fi.tiny, fi.tiny / 2, -fi.tiny / 2, fi.smallest_subnormal, -fi.smallest_subnormal], dtype=fi.dtype)
    xs = np.array([1.0, 0.5, fi.eps, fi.tiny, -1.0, 2.0, 0.25], dtype=fi.dtype)
    vsub = sub[pick(sub.size, 1)]; xsub = xs[rng.integers(0, xs.size, ncols)]
    if cx:
        vsub = cplx(vsub, sub[pick(sub.size, 2)]); xsub = cplx(xsub, xs[rng.integers(0, xs.size, ncols)])
    out.append(("subnormal", vsub, xsub))
    big = np.array([fi.max / 2, fi.max], dtype=fi.dtype)
    xo = np.array([1.0, -1.0, 2.0, 1.0, 1.0], dtype=fi.dtype)
    vbig = (big[pick(2, 3)] * re_s).astype(fi.dtype); xbig = xo[rng.integers(0, xo.size, ncols)]
    if cx:
        vbig = cplx(vbig, (big[pick(2, 4)] * im_s * (pick(2, 5) == 0)).astype(fi.dtype))
        xbig = cplx(xbig, xo[rng.integers(0, xo.size, ncols)] * (rng.uniform(size=ncols) < 0.5))
    out.append(("overflow", vbig, xbig))
    if cx:
        v = np.array(data, dtype=dtype, copy=True)
        vv = components(v)
        salted = rng.choice(nnz, size=max(3, nnz // 40), replace=False)
        for j, (re, im) in enumerate(((np.inf, 0.0), (0.0, np.inf), (np.nan, 1.0))):
            vv[salted[j::3], 0] = re; vv[salted[j::3], 1] = im
        out.append(("complex_inf", v, x_fin))
    return out


def padded_spmv_multiplying_by_zero(indptr, indices, data, x, width=None):
    """A deliberately WRONG SpMV, the kind the poison test exists to catch: every row is padded to `width` slots whose column is
    clamped into range and whose value is zero, and the padding is MULTIPLIED (0 * x[j]) instead of selected away.  Bit-identical
    to the reference fold on finite x (but for the sign of a zero row); NaN wherever a padded slot reads a poisoned element."""
    n = len(indptr) - 1
    lens = np.diff(indptr)
    width = int(lens.max()) + 1 if width is None else width
    y = np.zeros(n, dtype=data.dtype)
    with np.errstate(all="ignore"):
        for r in range(n):
            acc = data.dtype.type(0)
            for s in range(width):
                k = indptr[r] + s
                if s < lens[r]:
                    acc = acc + data[k] * x[indices[k]]
                else:
                    acc = acc + data.dtype.type(0) * x[min(r + s, len(x) - 1)]      # the clamped neighbour's element, times zero
            y[r] = acc
    return y


def first_product_seeded_spmv(indptr, indices, data, x):
    """Another deliberately wrong SpMV: the accumulator is seeded with the row's first product instead of +0.0 — identical on
    every row but one whose products are all -0.0, which comes out -0.0 where the reference gives +0.0."""
    n = len(indptr) - 1
    y = np.zeros(n, dtype=data.dtype)
    with np.errstate(all="ignore"):
        for r in range(n):
            a, b = indptr[r], indptr[r + 1]
            if b > a:
                acc = data[a] * x[indices[a]]
                for k in range(a + 1, b):
                    acc = acc + data[k] * x[indices[k]]
                y[r] = acc
    return y


def fold_spmv(indptr, indices, data, x):
    """The reference's per-row fold restated in numpy, slot by slot over all rows at once: acc = +0.0, then acc += val * x[col]
    left to right over the STORED entries only; a complex product is (ac - bd) + (ad + bc) i with every operation rounded on its
    own in the component type (oracle/scalar.h).  An independent statement of what the oracle's SpMV computes."""
    indptr = np.asarray(indptr, dtype=np.int64); indices = np.asarray(indices, dtype=np.int64)
    n = indptr.size - 1
    lens = np.diff(indptr)
    cx = data.dtype.kind == "c"
    d, xv = components(data), components(np.ascontiguousarray(x, dtype=data.dtype))
    acc = np.zeros((n, 2) if cx else (n,), dtype=d.dtype)
    with np.errstate(all="ignore"):
        for s in range(int(lens.max()) if n else 0):
            rows = np.flatnonzero(lens > s)
            k = indptr[rows] + s
            a, b = d[k], xv[indices[k]]
            if cx:
                acc[rows, 0] = acc[rows, 0] + (a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1])
                acc[rows, 1] = acc[rows, 1] + (a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0])
            else:
                acc[rows] = acc[rows] + a * b
    return acc.view(data.dtype).reshape(n) if cx else acc
