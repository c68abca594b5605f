"""sprsolve_amd — MI355X-native (gfx950, HIP) backend for sprsolve's Krylov hot path.

Public surface mirrors the reference crate's (src/lib.rs:15-19): `BiCGStab`, `MinRes`,
`CSMinRes`, `GaussSeidel`, `MatVecMul`, `precond`, `vecalg`, `error`.  All compute runs in
libsprsolve_hip.so (hand-written HIP, C ABI in include/sprsolve_hip.h); importing the
package does not load it, using it does, and there is no CPU fallback.
"""
from . import error, precond, vecalg  # noqa: F401
from .amg import AMG  # noqa: F401
from .batch import BatchCsr  # noqa: F401
from .bicg_stab import BiCGStab  # noqa: F401
from .cg import CG  # noqa: F401
from .cg_many import CGMany  # noqa: F401
from .cg_shift import CGShift  # noqa: F401
from .cs_minres import CSMinRes  # noqa: F401
from .eigsh import Eigsh  # noqa: F401
from .expm import Expm, expm_multiply  # noqa: F401
from .gauss_seidel import GaussSeidel  # noqa: F401
from .gmres import GMRES  # noqa: F401
from .fsai import FSAI  # noqa: F401
from .bjacobi import BlockJacobi  # noqa: F401
from .idrs import IDRS  # noqa: F401
from .ilu import ILU0  # noqa: F401
from .lobpcg import Lobpcg  # noqa: F401
from .lsmr import LSMR  # noqa: F401
from .device import Context, DevVec, default_ctx  # noqa: F401
from .mat import HipCsr, MatVecMul  # noqa: F401
from .minres import MinRes  # noqa: F401
from .order import color_order, inverse_permutation  # noqa: F401
from .precond import DiagPrecond  # noqa: F401
from .refine import Refine  # noqa: F401
from .svds import Svds  # noqa: F401

__version__ = "0.1.0"
