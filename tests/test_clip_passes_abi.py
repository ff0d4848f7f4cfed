"""CPU tier of the pass counter of a batch context: the entry points that tell which way a batch went, and hand out any clip's
lists, are declared, exported and bound; the ABI version stays 4 (the feature is detected by the symbol); a null argument is refused
with a message; the Python layer has ``Context.last_clip_passes`` and ``last_sim_indices(..., clip=)``."""
import ctypes as C
import inspect

from repet import _native
from test_abi import declared_functions

NEW = ["repet_ctx_last_clip_passes", "repet_ctx_last_sim_indices_clip"]


def test_new_names_are_declared_exported_and_bound():
    lib = _native.lib()
    declared = declared_functions()
    for name in NEW:
        assert name in declared, f"{name} is not declared in repet_hip.h"
        assert name in _native.EXPORTED_SYMBOLS and name in _native._SIGNATURES
        assert getattr(lib, name).argtypes == _native._SIGNATURES[name][1]
        assert getattr(lib, name).restype is C.c_int
    P = C.c_void_p
    assert _native._SIGNATURES[NEW[0]][1] == [P, C.POINTER(C.c_int32)]
    # the clip in front of the arguments of repet_ctx_last_sim_indices: nothing else differs
    assert _native._SIGNATURES[NEW[1]][1] == [P, C.c_int32] + _native._SIGNATURES["repet_ctx_last_sim_indices"][1][1:]
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4                      # additions: the version stays


def test_null_arguments_are_refused_with_a_message():
    lib = _native.lib()
    v = C.c_int32(7)
    buf = (C.c_int32 * 4)()
    assert lib.repet_ctx_last_clip_passes(None, C.byref(v)) == _native.ERR_BAD_ARG and lib.repet_last_error()
    assert lib.repet_ctx_last_sim_indices_clip(None, 0, buf, buf, 1, 1) == _native.ERR_BAD_ARG and lib.repet_last_error()
    assert v.value == 7


def test_python_surface():
    assert isinstance(inspect.getattr_static(_native.Context, "last_clip_passes"), property)
    p = inspect.signature(_native.Context.last_sim_indices).parameters
    assert list(p) == ["self", "n_rows", "number", "clip"] and p["clip"].default == 0
