"""CPU tier of the ragged batch (``repet.separate(..., lengths=...)``: clips of unequal lengths in one padded tensor): the new
entry points are declared, exported and bound, the ABI version stays 4, a null context is refused with a message, the too-short
check that needs no device says what the one-clip call says, and the Python layer rejects bad ``lengths`` before it touches the
library and routes lengths that all equal ``N`` to the unchanged path."""
import ctypes as C
import inspect

import numpy as np
import pytest

import repet
from repet import _native
from test_abi import declared_functions
from test_online_foreground_abi import bare

torch = pytest.importorskip("torch")

NEW = ["repet_ctx_upload_device_ragged", "repet_ctx_clip_lengths", "repet_check_clip_lengths"]
FS = 8000                                                                          # W = 512, H = 256, a buffer of 312 frames


class FakeTensor:
    """Enough of a tensor for the checks that come before the library: a shape."""
    def __init__(self, *shape):
        self.shape = shape


def no_library(monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    monkeypatch.setattr(_native, "is_device_tensor", lambda x: (_ for _ in ()).throw(AssertionError("the tensor was looked at")))


def test_new_names_are_declared_exported_and_bound():
    lib = _native.lib()
    declared = declared_functions()
    for name in NEW:
        assert name in declared, f"{name} is not declared in repet_hip.h"
        assert name in _native.EXPORTED_SYMBOLS and name in _native._SIGNATURES
        assert getattr(lib, name).argtypes == _native._SIGNATURES[name][1]
        assert getattr(lib, name).restype is C.c_int
    P, I64P = C.c_void_p, C.POINTER(C.c_int64)
    assert _native._SIGNATURES[NEW[0]][1] == [P, P, C.c_int, C.c_int32, C.c_int64, C.c_int32, I64P, I64P, P]
    # the strided ingest with the host array of lengths in front of the stream: nothing else differs
    assert _native._SIGNATURES[NEW[0]][1][:7] + [P] == _native._SIGNATURES["repet_ctx_upload_device_strided"][1]
    assert _native._SIGNATURES[NEW[1]][1] == [P, I64P, C.c_int32, C.POINTER(C.c_int32)]
    assert _native._SIGNATURES[NEW[2]][1] == [C.c_int, C.POINTER(_native.Params), C.c_int32, I64P, C.c_int32]
    assert lib.repet_abi_version() == _native.ABI_VERSION == 4                      # additions: the version stays


def test_a_null_context_or_table_is_refused_with_a_message():
    lib = _native.lib()
    strides = (C.c_int64 * 3)(2000, 2, 1)
    lengths = (C.c_int64 * 2)(1000, 900)
    n = C.c_int32(7)
    for call in (lambda: lib.repet_ctx_upload_device_ragged(None, None, _native.F32, 2, 1000, 2, strides, lengths, None),
                 lambda: lib.repet_ctx_clip_lengths(None, lengths, 2, C.byref(n)),
                 lambda: lib.repet_check_clip_lengths(_native.ALGO_IDS["sim"], None, 0, lengths, 2),
                 lambda: lib.repet_check_clip_lengths(_native.ALGO_IDS["sim"], repet.derive_params(FS), 0, None, 2)):
        assert call() == _native.ERR_BAD_ARG
        assert lib.repet_last_error()
    assert n.value == 7 and list(lengths) == [1000, 900]


def one_clip_limit():
    p = repet.derive_params(FS)
    return p, (p.buffer_frames - 2) * p.step_length + p.window_length               # the shortest clip simonline takes


def test_the_too_short_check_needs_no_device_and_names_the_clip():
    p, least = one_clip_limit()
    assert (p.window_length, p.step_length, p.buffer_frames) == (512, 256, 312)
    _native.check_clip_lengths("simonline", p, (least, least + 1, 98304))
    with pytest.raises(ValueError, match=r"clip 1 of the batch \(%d samples\): operands could not be broadcast together" % (least - 1)):
        _native.check_clip_lengths("simonline", p, (98304, least - 1, least))
    # start_frames: a shorter warm-up takes shorter clips, as the one-clip context does
    _native.check_clip_lengths("simonline", p, (4 * 256 + 512,), start_frames=6)
    with pytest.raises(ValueError, match="clip 0"):
        _native.check_clip_lengths("simonline", p, (4 * 256 + 511,), start_frames=6)
    # the period family: fewer frames than three periods of the shortest period
    short = 3 * p.period_lo * p.step_length - p.window_length
    for algo in ("original", "extended"):
        _native.check_clip_lengths(algo, p, (98304, 88001))
        with pytest.raises(ValueError, match=r"clip 1 .*attempt to get argmax of an empty sequence"):
            _native.check_clip_lengths(algo, p, (98304, short))
    # a clip of no samples is too short for every variant
    for algo in _native.ALGO_IDS:
        with pytest.raises(ValueError, match="clip 2 of the batch"):
            _native.check_clip_lengths(algo, p, (98304, 98304, 0))
    for algo in ("sim", "adaptive"):
        _native.check_clip_lengths(algo, p, (98304, 1))


@pytest.mark.parametrize("bad, error", [
    ([98304, 97280, 91137], ValueError),                         # three lengths, four clips
    ([98304, 97280, 91137, 88001, 5], ValueError),
    ([98304, -1, 91137, 88001], ValueError),
    ([98304, 98305, 91137, 88001], ValueError),                  # above N
    ([98304, 97280.0, 91137, 88001], TypeError),                 # not integers
    ([98304, "97280", 91137, 88001], TypeError),
    ([98304, True, 91137, 88001], TypeError),
    (np.array([98304.0, 97280, 91137, 88001]), TypeError),
    (np.array([[98304, 97280, 91137, 88001]]), (TypeError, ValueError)),
    (torch.tensor([98304.0, 97280, 91137, 88001]), TypeError),
    (97280, TypeError),
    ("1234", TypeError),
])
def test_python_rejects_bad_lengths_before_the_library_is_touched(bad, error, monkeypatch):
    no_library(monkeypatch)
    batch = FakeTensor(4, 98304, 2)
    for algo in _native.ALGO_IDS:
        with pytest.raises(error):
            repet.separate(algo, batch, FS, which="both", lengths=bad)
    with pytest.raises(error):
        _native.clip_lengths(bad, batch.shape)


def test_lengths_go_with_a_batch_only(monkeypatch):
    no_library(monkeypatch)
    with pytest.raises(ValueError, match="batch"):
        repet.separate("sim", FakeTensor(98304, 2), FS, lengths=[98304])
    with pytest.raises(ValueError, match="batch"):
        repet.separate("sim", FakeTensor(98304, 2), FS, lengths=[98304, 98304])


def test_lengths_on_a_device_are_a_type_error(monkeypatch):
    """The call must not wait for the device: a tensor anywhere but on the host is refused by its device type alone."""
    no_library(monkeypatch)
    meta = torch.empty(4, dtype=torch.int64, device="meta")
    with pytest.raises(TypeError, match="host"):
        repet.separate("simonline", FakeTensor(4, 98304, 2), FS, lengths=meta)


def test_host_forms_are_taken_alike():
    want = (98304, 97280, 91137, 88001)
    shape = (4, 98304, 2)
    for form in (list(want), want, np.array(want), np.array(want, dtype=np.int32), np.array(want, dtype=np.uint64),
                 torch.tensor(want), torch.tensor(want, dtype=torch.int32), [np.int64(v) for v in want]):
        got = _native.clip_lengths(form, shape)
        assert got == want and all(type(v) is int for v in got)
    assert _native.clip_lengths([0, 0, 0, 5], shape) == (0, 0, 0, 5)


def test_lengths_that_all_equal_n_take_the_unchanged_path(monkeypatch):
    assert _native.clip_lengths([98304] * 4, (4, 98304, 2)) is None
    assert _native.clip_lengths(torch.full((4,), 98304), (4, 98304, 2)) is None
    seen = {}
    monkeypatch.setattr(_native, "is_device_tensor", lambda x: True)
    monkeypatch.setattr(repet, "_separate_tensor", lambda *a, **kw: seen.update(kw) or "ran")
    assert repet.separate("simonline", FakeTensor(4, 98304, 2), FS, lengths=[98304] * 4) == "ran"
    assert seen["lengths"] is None                              # what a call without lengths hands over
    assert repet.separate("simonline", FakeTensor(4, 98304, 2), FS, lengths=[98304, 98304, 98304, 98303]) == "ran"
    assert seen["lengths"] == (98304, 98304, 98304, 98303)
    # and the layer below sends lengths=None to the strided ingest, anything else to the ragged one
    calls = []

    class Lib:
        def repet_ctx_upload_device_strided(self, *a):
            calls.append(("strided", len(a)))
            return 0

        def repet_ctx_upload_device_ragged(self, *a):
            calls.append(("ragged", list(a[7])))
            return 0

    class X:
        class device:
            index = 0

        def data_ptr(self):
            return 256

        def dim(self):
            return 3

        def record_stream(self, s):
            pass

    class Stream:
        cuda_stream = 0

        def wait_event(self, e):
            pass

    class Event:
        def record(self, s):
            pass

    monkeypatch.setattr(_native, "lib", lambda: Lib())
    ctx = bare(_native.Context)
    try:
        ctx._device, ctx._ingested, ctx._torch_stream = 0, Event(), Stream()
        monkeypatch.setattr(_native.Context, "torch_stream", lambda self: self._torch_stream)
        ctx.upload_layout(X(), _native.F32, (4, 98304, 2), (196608, 2, 1), stream=Stream(), lengths=None)
        ctx.upload_layout(X(), _native.F32, (4, 98304, 2), (196608, 2, 1), stream=Stream(), lengths=(98304, 97280, 91137, 88001))
    finally:
        ctx._h = None                          # (its __del__ must find nothing to close)
    assert calls == [("strided", 8), ("ragged", [98304, 97280, 91137, 88001])]
    assert ctx.shape == (4, 98304, 2)                           # the padded shape


def test_signatures():
    assert "lengths" in repet.separate.__doc__
    with pytest.raises(TypeError):                              # keyword only: twelve positional arguments are one too many
        repet.separate("sim", FakeTensor(2, 98304, 2), FS, None, "background", None, False, None, "reference", None, None, [98304, 1])
    p = inspect.signature(_native.Context.upload_tensor).parameters
    assert list(p) == ["self", "x", "stream", "lengths"] and p["lengths"].default is None
    assert list(inspect.signature(_native.Context.clip_lengths).parameters) == ["self"]
