"""CPU tier of moving a live stream between streaming handles (export_stream / import_stream): the five names are exported by
the built library, bound with argument types and listed, each refuses null arguments before any device is touched, and the
host-side header of a ``StreamState`` packs, unpacks and refuses in pure Python. What the calls compute needs a handle, hence a
device: tests/test_gpu_online_migrate.py."""
import ctypes
import struct

import numpy as np
import pytest

import repet
from repet import _native

NEW_NAMES = ["repet_online_stream_state_size", "repet_online_export_stream", "repet_online_export_stream_device",
             "repet_online_import_stream", "repet_online_import_stream_device"]


def test_new_names_are_exported_bound_and_listed():
    lib = _native.lib()
    for name in NEW_NAMES:
        assert hasattr(lib, name), name
        assert name in _native.EXPORTED_SYMBOLS and name in _native._SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _native._SIGNATURES[name][1], name
    # additive: the version the existing callers check has not moved
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4


def test_each_refuses_null_arguments():
    lib = _native.lib()
    a, b = ctypes.c_int64(7), ctypes.c_int64(7)
    header = ctypes.create_string_buffer(repet.StreamState.HEADER_BYTES)
    payload = ctypes.create_string_buffer(64)
    assert lib.repet_online_stream_state_size(None, ctypes.byref(a), ctypes.byref(b)) == _native.ERR_BAD_ARG
    assert lib.repet_online_export_stream(None, 0, header, payload) == _native.ERR_BAD_ARG
    assert lib.repet_online_export_stream_device(None, 0, header, payload, None) == _native.ERR_BAD_ARG
    assert lib.repet_online_import_stream(None, 0, header, payload) == _native.ERR_BAD_ARG
    assert lib.repet_online_import_stream_device(None, 0, header, payload, None) == _native.ERR_BAD_ARG
    assert lib.repet_online_import_stream(None, -1, None, None) == _native.ERR_BAD_ARG
    assert lib.repet_last_error()
    assert (a.value, b.value) == (7, 7)


def example_fields():
    return dict(magic=repet.StreamState.MAGIC, version=repet.StreamState.VERSION, window_length=512, step_length=256,
                buffer_frames=312, number_channels=2, number_bins=257, cutoff_bins=6, similarity_distance_frames=31,
                similarity_number=100, params_buffer_frames=312, flags=0, similarity_threshold=0.25, age_frames=-1,
                length_samples=0, history_rows=0, pending_samples=0, payload_bytes=24)


def test_header_round_trips():
    S = repet.StreamState
    fields = example_fields()
    header = S.pack_header(fields)
    assert isinstance(header, bytes) and len(header) == S.HEADER_BYTES == 96
    assert header[:4] == b"REPS" and struct.unpack_from("<I", header, 4) == (1,)
    assert S.unpack_header(header) == fields
    state = S(header, np.arange(24, dtype=np.uint8))
    assert state.fields == fields and state.age_frames == -1 and state.similarity_threshold == 0.25
    with pytest.raises(AttributeError):
        state.no_such_field
    blob = state.to_bytes()
    assert len(blob) == 96 + 24
    back = S.from_bytes(blob)
    assert back.header == header and back.payload.dtype == np.uint8 and np.array_equal(back.payload, state.payload)
    assert back.payload.flags.writeable                     # its own copy, not a view of the bytes


def test_header_refusals():
    S = repet.StreamState
    header = S.pack_header(example_fields())
    magic = bytearray(header)
    magic[2] ^= 0x40
    with pytest.raises(ValueError, match="magic"):
        S.unpack_header(bytes(magic))
    with pytest.raises(ValueError, match="version"):
        S.unpack_header(S.pack_header(dict(example_fields(), version=2)))
    for size in (0, 95, 97):
        with pytest.raises(ValueError, match="96 bytes"):
            S.unpack_header((header + b"\0")[:size])
    with pytest.raises(ValueError):
        S.unpack_header(S.pack_header(dict(example_fields(), payload_bytes=-8)))
    blob = S(header, np.zeros(24, dtype=np.uint8)).to_bytes()
    for wrong in (blob[:-1], blob + b"\0", blob[:50]):
        with pytest.raises(ValueError):
            S.from_bytes(wrong)
    with pytest.raises(ValueError):
        S(header, np.zeros(23, dtype=np.uint8)).to_bytes()   # a payload that is not what the header describes
    with pytest.raises(ValueError):
        S(header, np.zeros(6, dtype=np.float32)).to_bytes()


def test_python_surface():
    for name in ("export_stream", "import_stream", "stream_state_nbytes"):
        assert hasattr(_native.OnlineStreams, name), name
    for name in ("export_stream", "import_stream"):
        assert hasattr(_native.OnlineSeparator, name), name
    assert repet.StreamState is _native.StreamState
    assert "export_stream" in repet.online_streams.__doc__ and "import_stream" in repet.online_streams.__doc__
    assert "export_stream" in repet.online.__doc__
