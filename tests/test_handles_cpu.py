"""CPU-only checks of the solver handles' C ABI: what every kind's create and destroy, and the context's knob entry points,
answer to null pointers.  All of it returns before any HIP call, so no GPU is needed."""
import ctypes as C
import os

import pytest

INVALID_ARGUMENT = 7

# kind -> the arguments of sprs_<kind>_create_<s> between the operator and the out-pointer
KINDS = {
    "bicgstab": (4,), "minres": (4,), "csminres": (4,), "cg": (4,), "gmres": (4, 3), "idrs": (4, 2), "cgmany": (4, 2),
    "cgshift": (4, 2), "lsmr": (None,), "eigsh": (4, 3), "lobpcg": (12, 2), "svds": (None, 3), "expm": (4, 3),
}


@pytest.fixture(scope="module")
def L():
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("s", "dzsc")
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_null_operator_and_null_handle(L, kind, s):
    create = getattr(L, "sprs_%s_create_%s" % (kind, s))
    out = C.c_void_p()
    assert create(None, *KINDS[kind], C.byref(out)) == INVALID_ARGUMENT
    assert not out.value
    assert create(None, *KINDS[kind], None) == INVALID_ARGUMENT
    assert getattr(L, "sprs_%s_destroy" % kind)(None) == 0


def test_ctx_knobs_refuse_null(L):
    ctx = C.create_string_buffer(8)                 # any non-null pointer: a null key is refused before the context is read
    assert L.sprs_ctx_set(None, b"grid", 8) == INVALID_ARGUMENT
    assert L.sprs_ctx_set(ctx, None, 8) == INVALID_ARGUMENT
    assert L.sprs_ctx_set(None, None, 8) == INVALID_ARGUMENT
    assert L.sprs_ctx_get(None, b"grid") == -1
    assert L.sprs_ctx_get(ctx, None) == -1
    assert L.sprs_ctx_get(None, None) == -1
