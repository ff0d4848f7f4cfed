"""CPU tier of the per-slot inboxes of ``repet.online_streams`` (``enable_feed`` / ``feed`` / ``tick``): the eight entry points are
declared, exported, bound with their argument types and listed, the ABI version stays 4, each refuses a null handle with a
message and leaves its outputs alone, and the Python surface and the docstring's words are there."""
import ctypes as C
import inspect

import numpy as np

import repet
from repet import _native
from test_abi import declared_functions

NEW = ["repet_online_enable_feed", "repet_online_feed", "repet_online_feed_device", "repet_online_queued", "repet_online_pad_feed",
       "repet_online_clear_feed", "repet_online_tick", "repet_online_tick_device"]


def test_new_names_are_declared_exported_and_bound():
    lib = _native.lib()
    declared = declared_functions()
    for name in NEW:
        assert name in declared, f"{name} is not declared in repet_hip.h"
        assert name in _native.EXPORTED_SYMBOLS and name in _native._SIGNATURES
        assert getattr(lib, name).restype == _native._SIGNATURES[name][0] == C.c_int
        assert getattr(lib, name).argtypes == _native._SIGNATURES[name][1]
    sig = _native._SIGNATURES
    # a tick is a push without a source, plus the consumed flags
    push, tick = sig["repet_online_push_streams"][1], sig["repet_online_tick"][1]
    assert tick == [push[0], C.c_int64] + push[4:6] + [C.c_void_p] + push[6:]
    push, tick = sig["repet_online_push_device"][1], sig["repet_online_tick_device"][1]
    assert tick == [push[0], C.c_int64] + push[6:10] + [C.c_void_p] + push[10:]
    # the device feed is the host feed plus strides, a wait stream and a signal stream
    assert sig["repet_online_feed_device"][1] == sig["repet_online_feed"][1] + [C.c_void_p] * 3
    assert sig["repet_online_clear_feed"][1] == sig["repet_online_hold_streams"][1]
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4


def test_null_handles_are_refused_with_a_message():
    lib = _native.lib()
    slots = (C.c_int32 * 2)(0, 1)
    counts = (C.c_int64 * 2)(4, 4)
    audio = np.zeros((2, 4, 1))
    out = np.full((2, 256, 1), 7.0)
    strides = (C.c_int64 * 3)(4, 1, 1)
    queued = (C.c_int64 * 2)(7, 7)
    pads = (C.c_int64 * 2)(7, 7)
    consumed = (C.c_uint8 * 2)(7, 7)
    written = C.c_int64(7)
    ptr = _native.ptr
    for call in (lambda: lib.repet_online_enable_feed(None, 1024),
                 lambda: lib.repet_online_feed(None, slots, counts, 2, ptr(audio), _native.F64, 4),
                 lambda: lib.repet_online_feed(None, slots, None, 2, ptr(audio), _native.F64, 4),
                 lambda: lib.repet_online_feed_device(None, slots, counts, 2, ptr(audio), _native.F64, 4, strides, None, None),
                 lambda: lib.repet_online_queued(None, 0, queued),
                 lambda: lib.repet_online_queued(None, -1, queued),
                 lambda: lib.repet_online_pad_feed(None, slots, 2, pads),
                 lambda: lib.repet_online_pad_feed(None, None, 0, pads),
                 lambda: lib.repet_online_clear_feed(None, slots, 2),
                 lambda: lib.repet_online_clear_feed(None, None, 0),
                 lambda: lib.repet_online_tick(None, 1, ptr(out), 256, consumed, C.byref(written)),
                 lambda: lib.repet_online_tick_device(None, 1, ptr(out), _native.F64, strides, None, consumed, C.byref(written))):
        assert call() == _native.ERR_BAD_ARG
        assert lib.repet_last_error()
    assert list(queued) == [7, 7] and list(pads) == [7, 7] and list(consumed) == [7, 7] and written.value == 7
    assert (out == 7.0).all()


def test_python_surface():
    cls = _native.OnlineStreams
    assert list(inspect.signature(cls.enable_feed).parameters) == ["self", "capacity_samples"]
    assert list(inspect.signature(cls.feed).parameters) == ["self", "slots", "chunk", "counts"]
    assert inspect.signature(cls.feed).parameters["counts"].default is None
    assert list(inspect.signature(cls.queued).parameters) == ["self", "slot"]
    assert list(inspect.signature(cls.pad_feed).parameters) == ["self", "slots"]
    assert list(inspect.signature(cls.clear_feed).parameters) == ["self", "slots"]
    assert list(inspect.signature(cls.tick).parameters) == ["self", "hops", "out", "which", "dtype"]
    assert inspect.signature(cls.tick).parameters["hops"].default == 1
    assert list(inspect.signature(cls.tick).parameters)[2:] == list(inspect.signature(cls.push).parameters)[2:]
    assert isinstance(cls.feed_capacity, property) and isinstance(cls.last_consumed, property)
    for name in ("enable_feed", "feed_capacity", "feed", "queued", "pad_feed", "clear_feed", "tick", "last_consumed"):
        assert getattr(cls, name).__doc__
        assert not hasattr(_native.OnlineSeparator, name)          # one stream: its push takes any n
    doc = repet.online_streams.__doc__
    for word in ("``enable_feed(capacity_samples)``", "``feed(slots, chunk, counts=None)``", "``tick(hops=1)``",
                 "``queued(slot=None)``", "``pad_feed(slots=None)``", "``clear_feed(slots=None)``", "``last_consumed``",
                 "``feed_capacity``", "starved", "bit for bit"):
        assert word in doc
    for word in ("``enable_feed(capacity_samples)``", "``tick(hops=1)``"):
        assert word in cls.__doc__
