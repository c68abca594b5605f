"""Shared plumbing of the solver mirrors: the handle's life, the one solve call of the linear solvers, and what the eigen / SVD
solvers and the per-column solvers have in common."""
import ctypes as C

import numpy as np

from . import _lib, gen
from .amg import AMG
from .bjacobi import BlockJacobi
from .device import DevVec, dev_len, dev_ptr, is_device_array, pre_sync, sfx
from .error import BreakDown, IncompatibleMatrixFormat, InsufficientIterNum, check, solve_result
from .fsai import FSAI
from .ilu import ILU0

_ARG_ERRORS = (_lib.INCOMPATIBLE_RHS_SIZE, _lib.INCOMPATIBLE_X_SIZE, _lib.DIM_MISMATCH, _lib.INVALID_ARGUMENT)


def _invalid_argument(ctx_h):
    """The ValueError of an argument the library refused with a text: it says which."""
    return ValueError("sprsolve_hip: invalid argument: " + (_lib.lib().sprs_last_error(ctx_h) or b"").decode(errors="replace"))


class _Handle:
    """A solver handle over a borrowed operator: A, dtype, s (the entry points' suffix) and h, from sprs_<NAME>_create_<s> to
    sprs_<NAME>_destroy."""
    NAME = None         # "bicgstab" | "minres" | ... : the entry points are sprs_<NAME>_*
    SAYS_WHY = False    # the library writes a text for every argument its create refuses: the ValueError carries it
    h = None            # until creation has succeeded: close() and __del__ of a failed `new` are no-ops

    def _create(self, A, *create_args):
        self.A = A                      # borrowed, like `A: &'data M` (bicg_stab.rs:18)
        self.dtype = A.dtype
        self.s = sfx(self.dtype)
        h = C.c_void_p()
        st = getattr(_lib.lib(), "sprs_%s_create_%s" % (self.NAME, self.s))(A.h, *create_args, C.byref(h))
        if st == _lib.INVALID_ARGUMENT and self.SAYS_WHY:
            raise _invalid_argument(A.ctx.h)
        check(st, A.ctx.h)
        self.h = h

    def close(self):
        if self.h:
            getattr(_lib.lib(), "sprs_%s_destroy" % self.NAME)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def applied_prefix(precond):
    """"ilu0" / "amg" / "fsai" / "bjacobi" for such a handle: the solves it preconditions are sprs_<prefix>_<solver>_solve[_dev]_*.  None for
    anything else."""
    for cls, prefix in ((ILU0, "ilu0"), (AMG, "amg"), (FSAI, "fsai"), (BlockJacobi, "bjacobi")):
        if isinstance(precond, cls):
            return prefix
    return None


class _SolverBase(_Handle):
    KIND = None       # _lib.SOLVER_*
    _trace = None

    def __init__(self, A, size, *create_args):
        self.size = int(size)
        self._create(A, self.size, *create_args)

    @classmethod
    def new(cls, A, size):
        return cls(A, size)

    # ---- options (no reference analogue; instrumentation of this backend)
    def set_mode(self, mode):
        """'fused' (default) or 'literal' (one kernel per reference op, host-consumed scalars)."""
        m = {"fused": 0, "literal": 1}[mode] if isinstance(mode, str) else int(mode)
        check(_lib.lib().sprs_solver_set_mode(self.h, self.KIND, m), self.A.ctx.h)

    def set_trace(self, capacity_rows):
        if capacity_rows:
            self._trace = np.zeros((int(capacity_rows), 8))
            check(_lib.lib().sprs_solver_set_trace(self.h, self.KIND, self._trace.ctypes.data_as(C.c_void_p),
                                                   int(capacity_rows)), self.A.ctx.h)
        else:
            self._trace = None
            check(_lib.lib().sprs_solver_set_trace(self.h, self.KIND, None, 0), self.A.ctx.h)

    def trace(self):
        rows = C.c_size_t()
        check(_lib.lib().sprs_solver_trace_rows(self.h, self.KIND, C.byref(rows)), self.A.ctx.h)
        return self._trace[: rows.value].copy() if self._trace is not None else np.zeros((0, 8))

    def set_profile(self, enable=True):
        """False / 0: off; True / 1: HIP events around every SpMV launch; k >= 2: around one pair of consecutive launches in k."""
        check(_lib.lib().sprs_solver_set_profile(self.h, self.KIND, int(enable)), self.A.ctx.h)

    def profile(self):
        ms = C.c_double(); n = C.c_int64(); tot = C.c_double()
        check(_lib.lib().sprs_solver_get_profile(self.h, self.KIND, C.byref(ms), C.byref(n), C.byref(tot)), self.A.ctx.h)
        k2 = C.c_int64(); k4 = C.c_int64()
        check(_lib.lib().sprs_solver_get_fused_launches(self.h, self.KIND, C.byref(k2), C.byref(k4)), self.A.ctx.h)
        st = C.c_int64(); do = C.c_int64(); t2 = C.c_int64(); t4 = C.c_int64()
        check(_lib.lib().sprs_solver_get_profile_counts(self.h, self.KIND, C.byref(st), C.byref(do), C.byref(t2), C.byref(t4)), self.A.ctx.h)
        k5 = C.c_int64()
        check(_lib.lib().sprs_solver_get_chain_k5_launches(self.h, self.KIND, C.byref(k5)), self.A.ctx.h)
        return dict(spmv_ms_total=ms.value, spmv_launches=n.value, solve_ms=tot.value, fused_k2=k2.value, fused_k4=k4.value, chain_k5=k5.value,
                    steps=st.value, timed_dot_other=do.value, timed_fused_k2=t2.value, timed_fused_k4=t4.value)

    # ---- the call itself
    def _solve(self, precond, rhs, x, max_iter, tol, want_precond, prefix=None):
        """prefix: None for a `DiagPrecond` (or no preconditioner); "ilu0" / "amg" / "fsai" / "bjacobi" for BiCGStab / MINRES / CG / GMRES with such a handle for the
        preconditioner: the same call under the name sprs_<prefix>_<solver>_solve[_dev]_*."""
        L = _lib.lib()
        its = C.c_size_t(0); res = _lib.REAL[self.s](0.0)
        name = self.NAME if prefix is None else "%s_%s" % (prefix, self.NAME)
        dev = is_device_array(rhs)
        if dev != is_device_array(x):
            raise TypeError("rhs and x must both be host arrays or both be device vectors")
        if dev:
            pre_sync(rhs, x)
            rp, rl, xp, xl = dev_ptr(rhs), dev_len(rhs), dev_ptr(x), dev_len(x)
            if self.NAME == "csminres":
                st = getattr(L, "sprs_csminres_solve_dev_" + self.s)(self.h, rp, rl, xp, xl, int(max_iter), float(tol),
                                                                  C.byref(its), C.byref(res))
            else:
                st = getattr(L, "sprs_%s_solve_dev_%s" % (name, self.s))(
                    self.h, precond.h if precond is not None else None, rp, rl, xp, xl, int(max_iter), float(tol),
                    C.byref(its), C.byref(res))
        else:
            rhs_a = np.ascontiguousarray(rhs, dtype=self.dtype)
            if not (isinstance(x, np.ndarray) and x.dtype == self.dtype and x.flags.c_contiguous):
                raise TypeError("x must be a contiguous %s ndarray (it is updated in place)" % self.dtype)
            rp, xp = rhs_a.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p)
            if want_precond:
                st = getattr(L, "sprs_%s_%s_%s" % (name, "precond_solve" if prefix is None else "solve", self.s))(
                    self.h, precond.h, rp, rhs_a.size, xp, x.size, int(max_iter), float(tol), C.byref(its), C.byref(res))
            else:
                st = getattr(L, "sprs_%s_solve_%s" % (self.NAME, self.s))(
                    self.h, rp, rhs_a.size, xp, x.size, int(max_iter), float(tol), C.byref(its), C.byref(res))
        return solve_result(st, its.value, res.value, self.A.ctx.h)


# ---- Eigsh, Svds, Lobpcg
def stream_vector(n, dtype, stream):
    """gen.uniform's stream `stream` (the imaginary parts: stream + 1), rounded to dtype: the default start vectors."""
    v = gen.uniform(gen.SEED, n, stream=stream)
    if np.dtype(dtype).kind == "c":
        v = v + 1j * gen.uniform(gen.SEED, n, stream=stream + 1)
    return v.astype(dtype)


def in_vec(v, dtype):
    """-> (pointer, length, is it a device vector, what keeps the pointer alive) of an input vector: a device vector, synchronised,
    or a host array made contiguous in dtype.  None: a null pointer for the host entry point."""
    if v is None:
        return None, 0, False, None
    if is_device_array(v):
        pre_sync(v)
        return dev_ptr(v), dev_len(v), True, v
    a = np.ascontiguousarray(v, dtype=dtype)
    return a.ctypes.data_as(C.c_void_p), a.size, False, a


def which_and_tol(which, tol, s, table):
    """`which` as the library's code (a name of `table`, or the code itself); tol = 0.0 as the default of the scalar type."""
    if isinstance(which, str):
        if which not in table:
            raise ValueError("which must be 'largest' or 'smallest'")
        which = table[which]
    if tol == 0.0:
        tol = 1e-4 if s in "sc" else 1e-10
    return int(which), float(tol)


def eig_call(solver, base, dev, head, k, lens, want, ncount):
    """sprs_<base>_solve[_dev]_<s>(h, *head, vals, [vectors, k * len for len in lens], res, ncount counters)
    -> (status, vals, [a (k, len) array or None for len in lens], res, [counters]).  dev: the device entry point, whose vectors
    are `DevVec`s copied back and freed here; else numpy arrays.  The vectors are None unless `want`, and after a status that
    leaves none (anything but Ok and InsufficientIterNum)."""
    rdt = np.float32 if solver.s in "sc" else np.float64
    pr = C.POINTER(_lib.REAL[solver.s])
    vals = np.zeros(max(k, 1), rdt); res = np.zeros(max(k, 1), rdt)
    cnt = [C.c_size_t(0) for _ in range(ncount)]
    if not want:
        bufs = [None] * len(lens)
    elif dev:
        bufs = [DevVec(k * n, solver.dtype, solver.A.ctx) for n in lens]
    else:
        bufs = [np.zeros((k, n), solver.dtype) for n in lens]
    vec_args = []
    for b, n in zip(bufs, lens):
        vec_args += [None if b is None else (b.ptr if dev else b.ctypes.data_as(C.c_void_p)), k * n]
    st = getattr(_lib.lib(), "sprs_%s_solve%s_%s" % (base, "_dev" if dev else "", solver.s))(
        solver.h, *head, vals.ctypes.data_as(pr), *vec_args, res.ctypes.data_as(pr), *[C.byref(c) for c in cnt])
    keep = st in (_lib.OK, _lib.INSUFFICIENT_ITER)
    vecs = []
    for b, n in zip(bufs, lens):
        if b is not None and dev:
            vecs.append(b.to_numpy().reshape(k, n) if keep else None)
            b.free()
        else:
            vecs.append(b if keep else None)
    return st, vals[:k], vecs, res[:k], [c.value for c in cnt]


def eig_result(st, out, names, iters, ctx_h, rhs_msg="Input vec dimension doesn't match the matrix size"):
    """`out` after Ok; InsufficientIterNum / BreakDown (at `iters`) carry what was computed: out's entries as attributes `names`."""
    if st == _lib.OK:
        return out
    if st == _lib.INCOMPATIBLE_RHS_SIZE:
        raise IncompatibleMatrixFormat(rhs_msg)
    if st == _lib.INCOMPATIBLE_X_SIZE:
        raise IncompatibleMatrixFormat("Input and output vec dimension do not match")
    if st in (_lib.INSUFFICIENT_ITER, _lib.BREAKDOWN):
        e = InsufficientIterNum(iters) if st == _lib.INSUFFICIENT_ITER else BreakDown(iters)
        for name, v in zip(names, out):
            setattr(e, name, v)
        raise e
    check(st, ctx_h)


# ---- CGMany, CGShift: one status per column
def column_call(solver, ncol, call):
    """call(its, res, status) -> the library's status, on arrays of ncol entries -> (its, res, status) as numpy arrays.  Solver
    events are reported there, never raised; solver.last_status is what the call returned; argument errors raise."""
    R = _lib.REAL[solver.s]
    n_out = max(int(ncol), 1)
    its = (C.c_size_t * n_out)(); res = (R * n_out)(); status = (C.c_int * n_out)()
    st = call(its, res, status)
    solver.last_status = int(st)
    if st == _lib.INVALID_ARGUMENT and solver.SAYS_WHY:
        raise _invalid_argument(solver.A.ctx.h)
    if st >= _lib.ERR_HIP or (st in _ARG_ERRORS):
        solve_result(st, 0, 0.0, solver.A.ctx.h)
    return (np.array(its[:ncol], dtype=np.int64), np.array(res[:ncol], dtype=np.dtype(R)), np.array(status[:ncol], dtype=np.int32))
