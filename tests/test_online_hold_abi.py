"""CPU tier of held slots (``hold`` / ``resume`` of single slots of ``repet.online_streams``): the three entry points are
declared, exported, bound with their argument types and listed, the ABI version stays 4, each refuses a null handle with a
message and leaves its output alone, and the Python surface is there."""
import ctypes as C
import inspect

import repet
from repet import _native
from test_abi import declared_functions

NEW = ["repet_online_hold_streams", "repet_online_resume_streams", "repet_online_stream_held"]


def test_new_names_are_declared_exported_and_bound():
    lib = _native.lib()
    declared = declared_functions()
    for name in NEW:
        assert name in declared, f"{name} is not declared in repet_hip.h"
        assert name in _native.EXPORTED_SYMBOLS and name in _native._SIGNATURES
        assert getattr(lib, name).restype == _native._SIGNATURES[name][0] == C.c_int
        assert getattr(lib, name).argtypes == _native._SIGNATURES[name][1]
    assert _native._SIGNATURES["repet_online_hold_streams"][1] == _native._SIGNATURES["repet_online_restart_streams"][1]
    assert _native._SIGNATURES["repet_online_resume_streams"][1] == _native._SIGNATURES["repet_online_restart_streams"][1]
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4


def test_null_handles_are_refused_with_a_message():
    lib = _native.lib()
    slots = (C.c_int32 * 2)(0, 1)
    held = C.c_int32(7)
    for call in (lambda: lib.repet_online_hold_streams(None, slots, 2),
                 lambda: lib.repet_online_hold_streams(None, None, 0),
                 lambda: lib.repet_online_resume_streams(None, slots, 2),
                 lambda: lib.repet_online_resume_streams(None, None, 0),
                 lambda: lib.repet_online_stream_held(None, 0, C.byref(held))):
        assert call() == _native.ERR_BAD_ARG
        assert lib.repet_last_error()
    assert held.value == 7


def test_python_surface():
    cls = _native.OnlineStreams
    assert list(inspect.signature(cls.hold).parameters) == ["self", "slots"]
    assert list(inspect.signature(cls.resume).parameters) == ["self", "slots"]
    assert list(inspect.signature(cls.held).parameters) == ["self", "slot"]
    for name in ("hold", "resume", "held"):
        assert getattr(cls, name).__doc__
        assert not hasattr(_native.OnlineSeparator, name)          # one stream: not pushing is its hold
    doc = repet.online_streams.__doc__
    for word in ("``hold(slots)``", "``resume(slots)``", "``held(slot)``"):
        assert word in doc
