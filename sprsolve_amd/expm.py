"""w = exp(tA) v: the Krylov matrix-exponential propagator with Expokit's step control (no reference analogue)."""
import ctypes as C

import numpy as np

from . import _lib
from ._solver import _Handle, eig_result
from .device import DevVec, dev_len, dev_ptr, is_device_array, pre_sync


class Expm(_Handle):
    """`Expm.new(A, size, ncv=0)`: the action of exp(tA) on a vector for a square A of any kind, by Arnoldi projection on ncv
    vectors with error-controlled sub-stepping; 3 <= ncv <= min(48, n), 0 means min(30, n).  The recurrence is stated in
    include/sprsolve_hip.h (sprs_expm_*) and runs in C++ on device-resident vectors and scalars (sprsolve_amd/csrc/expm.hip,
    expm_fuse.hpp); the handle holds ncv + 3 work vectors.  Single GPU."""
    NAME = "expm"
    SAYS_WHY = True     # a distributed A, ncv out of range

    def __init__(self, A, size, ncv=0):
        ncv = int(ncv)
        if ncv < 0:
            raise ValueError("ncv must be >= 0")
        self.size = int(size)
        self._create(A, self.size, ncv)
        self.ncv = ncv or min(30, self.size)

    @classmethod
    def new(cls, A, size, ncv=0):
        return cls(A, size, ncv)

    def apply(self, t, v, tol=0.0, max_steps=100000, tau0=0.0, out=None):
        """-> (w, info): w = exp(tA) v and info = dict(err, hump, t_done, steps, rejects, matvecs): the sum of the accepted error
        estimates (absolute; at most 1.2 |t| tol), the largest norm of the state met on the way, the time reached, the sub-steps,
        the rejected step sizes and the products A v.  t: any finite real.  tol = 0.0 selects sqrt(eps) of the real type; tau0: the
        first step size (0.0: chosen from the first projected matrix).  v: a host array or a device vector of n entries; w is of
        the same kind (`out`, which may be v itself, or a new one).  Raises SolverError: InsufficientIterNum after max_steps
        sub-steps carries the state reached as .w (at .info["t_done"]), BreakDown (a NaN, ten rejections in one sub-step) carries
        .w = None; both carry .info."""
        L = _lib.lib()
        R = _lib.REAL[self.s]
        err = R(0); hump = R(0); t_done = R(0)
        steps = C.c_size_t(0); rejects = C.c_size_t(0); matvecs = C.c_size_t(0)
        tail = (C.byref(err), C.byref(hump), C.byref(t_done), C.byref(steps), C.byref(rejects), C.byref(matvecs))
        n = self.size
        if is_device_array(v):
            pre_sync(v, out)
            w = out if out is not None else DevVec(n, self.dtype, self.A.ctx)
            st = getattr(L, "sprs_expm_apply_dev_" + self.s)(self.h, float(t), dev_ptr(v), dev_len(v), float(tol), int(max_steps), float(tau0),
                                                            dev_ptr(w), dev_len(w), *tail)
        else:
            va = np.ascontiguousarray(v, dtype=self.dtype)
            if out is None:
                w = np.zeros(va.size, self.dtype)
            else:
                w = out
                if not (isinstance(w, np.ndarray) and w.dtype == np.dtype(self.dtype) and w.flags.c_contiguous):
                    raise TypeError("out must be a contiguous array of the operator's dtype")
            st = getattr(L, "sprs_expm_apply_" + self.s)(self.h, float(t), va.ctypes.data_as(C.c_void_p), va.size, float(tol), int(max_steps),
                                                        float(tau0), w.ctypes.data_as(C.c_void_p), w.size, *tail)
        info = dict(err=float(err.value), hump=float(hump.value), t_done=float(t_done.value), steps=steps.value, rejects=rejects.value,
                    matvecs=matvecs.value)
        return eig_result(st, (None if st == _lib.BREAKDOWN else w, info), ("w", "info"), steps.value, self.A.ctx.h)


def expm_multiply(A, v, t=1.0, ncv=0, **kw):
    """exp(tA) v in one call (scipy.sparse.linalg.expm_multiply's order of arguments): -> (w, info) of Expm.apply."""
    E = Expm.new(A, A.shape[0], ncv)
    try:
        return E.apply(t, v, **kw)
    finally:
        E.close()
