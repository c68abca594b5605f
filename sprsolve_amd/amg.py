"""Smoothed-aggregation AMG preconditioner (no reference analogue; include/sprsolve_hip.h, sprs_amg_*)."""
import ctypes as C

import numpy as np

from . import _lib
from .device import dev_len, dev_ptr, is_device_array, pre_sync, sfx
from .error import DimensionMismatch, ZeorDiagonalElem, check
from .mat import MatVecMul


class AMG(MatVecMul):
    """`AMG.new(A, theta=0.08, coarse_max=256, max_levels=16, setup="host", seed=0)`: a smoothed-aggregation hierarchy of a
    square single-GPU `HipCsr`, built at creation.  `setup="host"`: the serial aggregation on the host, the sparse products on the
    device.  `setup="device"`: the parallel aggregation rule of `sprs_amg_create_dev` (greedy in decreasing splitmix64(seed, i))
    and every other step of a level in HBM; other aggregates, so another hierarchy, in the same handle.  As a `MatVecMul` it
    applies one V(1,1) cycle with damped Jacobi (csrc/amg.hip); `precond_solve` of `CG`, `GMRES`, `BiCGStab`, `MinRes` and `IDRS`
    and `Lobpcg.solve` take it in place of a `DiagPrecond`.  The handle owns its hierarchy: A may be closed afterwards."""

    STAGES = ("diag", "graph", "rounds", "pass2", "AT", "prolongator", "adjoint", "AP", "RAP", "packing", "LU")

    def __init__(self, handle, ctx, dtype, n):
        self.h, self.ctx, self.dtype, self.n = handle, ctx, np.dtype(dtype), int(n)
        self.s = sfx(self.dtype)

    @classmethod
    def new(cls, A, theta=0.08, coarse_max=256, max_levels=16, setup="host", seed=0):
        """Raises IncompatibleMatrixFormat (not square), ValueError (distributed A, unsorted or duplicate columns, a parameter out
        of range, a `setup` that is neither "host" nor "device") or ZeorDiagonalElem(row): a missing, zero or non-finite diagonal
        entry of the level being built, or such a pivot of the coarse LU.  `seed` orders the device aggregation; the host one
        ignores it."""
        if setup not in ("host", "device"):
            raise ValueError("sprsolve_hip: invalid argument: setup must be \"host\" or \"device\", not %r" % (setup,))
        h = C.c_void_p(); row = C.c_int64(-1)
        if setup == "device":
            st = _lib.lib().sprs_amg_create_dev(A.h, float(theta), int(coarse_max), int(max_levels), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                C.byref(h), C.byref(row))
        else:
            st = _lib.lib().sprs_amg_create(A.h, float(theta), int(coarse_max), int(max_levels), C.byref(h), C.byref(row))
        if st == _lib.ZERO_DIAGONAL:
            raise ZeorDiagonalElem(row.value)
        if st == _lib.INVALID_ARGUMENT:
            raise ValueError("sprsolve_hip: invalid argument: " + (_lib.lib().sprs_last_error(A.ctx.h) or b"").decode(errors="replace"))
        check(st, A.ctx.h)
        return cls(h, A.ctx, A.dtype, A.rows())

    @property
    def info(self):
        """dict(levels, launches, tail_level, lu_rows, rows, nnz, p_nnz, omega, setup, rounds): the number of levels, the kernel
        launches of one application, the first level that runs inside the one-workgroup tail kernel (== levels: none), the rows
        of the coarse LU (0: Jacobi sweeps), per level the rows, nnz(A_l), nnz(P_l) and the Jacobi weight, how the hierarchy was
        built ("host" / "device") and per aggregated level the pass-1 rounds of the device aggregation (zeros for "host")."""
        L = _lib.lib()
        v = [C.c_int64() for _ in range(4)]
        check(L.sprs_amg_info(self.h, *[C.byref(x) for x in v]), self.ctx.h)
        out = dict(zip(("levels", "launches", "tail_level", "lu_rows"), (x.value for x in v)))
        per = []
        for l in range(out["levels"]):
            r, z, p, w = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
            check(L.sprs_amg_level_info(self.h, l, C.byref(r), C.byref(z), C.byref(p), C.byref(w)), self.ctx.h)
            per.append((r.value, z.value, p.value, w.value))
        out.update(rows=[p[0] for p in per], nnz=[p[1] for p in per], p_nnz=[p[2] for p in per], omega=[p[3] for p in per])
        how = C.c_int64()
        rounds = np.zeros(max(out["levels"] - 1, 0), np.int64)
        check(L.sprs_amg_setup_info(self.h, C.byref(how), rounds.ctypes.data_as(C.c_void_p), rounds.size), self.ctx.h)
        out.update(setup=("host", "device")[how.value], rounds=rounds.tolist())
        return out

    @property
    def setup_ms(self):
        """Milliseconds of the device set-up per stage (`AMG.STAGES`): a diagnostic, taken only when the environment variable
        SPRS_CREATE_TRACE was set at creation (the set-up then drains the stream at every stage boundary); zeros otherwise and
        for a host-built handle."""
        ms = np.zeros(len(self.STAGES))
        check(_lib.lib().sprs_amg_setup_stage_ms(self.h, ms.ctypes.data_as(C.c_void_p), ms.size), self.ctx.h)
        return dict(zip(self.STAGES, ms.tolist()))

    def level(self, l, which="A"):
        """(indptr, indices, data) of A_l, P_l or R_l (which = "A" / "P" / "R")."""
        w = {"A": 0, "P": 1, "R": 2}[which]
        inf = self.info
        if not 0 <= l < inf["levels"] - (w > 0):
            raise ValueError("sprsolve_hip: invalid argument: level %d has no %s (levels: %d; the coarsest has neither P nor R)"
                             % (l, which, inf["levels"]))
        rows = inf["rows"][l] if w < 2 else inf["rows"][l + 1]
        nnz = inf["nnz"][l] if w == 0 else inf["p_nnz"][l]
        ip = np.zeros(rows + 1, np.int32); ix = np.zeros(nnz, np.int32); v = np.zeros(nnz, self.dtype)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(_lib.lib().sprs_amg_level_read(self.h, l, w, vp(ip), vp(ix), vp(v), None), self.ctx.h)
        return ip, ix, v

    def aggregates(self, l):
        """The aggregate of every row of level l (not the coarsest)."""
        inf = self.info
        if not 0 <= l < inf["levels"] - 1:
            raise ValueError("sprsolve_hip: invalid argument: level %d has no aggregates (levels: %d)" % (l, inf["levels"]))
        agg = np.zeros(inf["rows"][l], np.int32)
        check(_lib.lib().sprs_amg_level_read(self.h, l, 1, None, None, None, agg.ctypes.data_as(C.c_void_p)), self.ctx.h)
        return agg

    def _apply(self, v_in, v_out, checked=True):
        L = _lib.lib()
        if is_device_array(v_in):
            if checked and (self.n != dev_len(v_in) or self.n != dev_len(v_out)):
                raise DimensionMismatch("Dimension mismatch")
            pre_sync(v_in, v_out)
            check(getattr(L, "sprs_amg_mul_vec_dev_" + self.s)(self.h, dev_ptr(v_in), dev_ptr(v_out)), self.ctx.h)
            self.ctx.sync()
            return
        x = np.ascontiguousarray(v_in, dtype=self.dtype)
        if not (isinstance(v_out, np.ndarray) and v_out.dtype == self.dtype and v_out.flags.c_contiguous):
            raise TypeError("v_out must be a contiguous %s ndarray" % self.dtype)
        check(getattr(L, "sprs_amg_mul_vec_" + self.s)(self.h, x.ctypes.data_as(C.c_void_p), x.size,
                                                       v_out.ctypes.data_as(C.c_void_p), v_out.size), self.ctx.h)

    def mul_vec(self, v_in, v_out):
        """v_out = one V-cycle on v_in; host arrays or device vectors (v_in may be v_out)."""
        self._apply(v_in, v_out)

    def mul_vec_unchecked(self, v_in, v_out):
        self._apply(v_in, v_out, checked=False)

    def mul_vec_dot(self, v_in, v_out):
        raise NotImplementedError("a preconditioner has no fused dot product (as DiagPrecond)")

    def mul_vec_dot_unchecked(self, v_in, v_out):
        raise NotImplementedError("a preconditioner has no fused dot product (as DiagPrecond)")

    def close(self):
        if self.h:
            _lib.lib().sprs_amg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
