"""The ABI and binding side of the 16-bit destination dtypes, without a GPU: the detection symbol, the tensor dtype mapping and the
header as a C compiler reads it."""
import ctypes as C
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")

from repet import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "repet_hip.h")


def test_detection_symbol_is_exported_bound_and_declared():
    assert "repet_emit_dtype_supported" in _native.EXPORTED_SYMBOLS
    assert hasattr(_native.lib(), "repet_emit_dtype_supported")
    with open(HEADER) as f:
        assert re.search(r"^int repet_emit_dtype_supported\(int dtype\);", f.read(), re.M)
    assert _native.lib().repet_abi_version() == 4 == _native.ABI_VERSION           # an addition: the version stays


def test_detection_symbol_answers_for_the_five_codes_only():
    fn = _native.lib().repet_emit_dtype_supported
    assert (_native.F32, _native.F64, _native.I16, _native.F16, _native.BF16) == (0, 1, 2, 3, 4)
    for code in range(5):
        assert fn(code) == 1, code
    for code in (-1, 5, 6, 1 << 20, -(1 << 31)):
        assert fn(code) == 0, code


def test_emit_tensor_code_maps_the_five_dtypes():
    want = {torch.float64: _native.F64, torch.float32: _native.F32, torch.int16: _native.I16, torch.float16: _native.F16,
            torch.bfloat16: _native.BF16}
    for dtype, code in want.items():
        assert _native.emit_tensor_code(torch.zeros(1, dtype=dtype)) == code
    for dtype in (torch.int32, torch.int8, torch.uint8, torch.int64, torch.complex64, torch.bool):
        with pytest.raises(ValueError):
            _native.emit_tensor_code(torch.zeros(1, dtype=dtype))


def test_result_tensor_code_is_what_it_was():
    """The older function keeps its two dtypes: the new ones go through emit_tensor_code."""
    assert _native.result_tensor_code(torch.zeros(1, dtype=torch.float32)) == _native.F32
    for dtype in (torch.int16, torch.float16, torch.bfloat16):
        with pytest.raises(ValueError):
            _native.result_tensor_code(torch.zeros(1, dtype=dtype))


def test_dtype_keyword_is_checked_before_anything_runs():
    assert _native.emit_dtype(None) is torch.float64
    for dtype in (torch.float64, torch.float32, torch.int16, torch.float16, torch.bfloat16):
        assert _native.emit_dtype(dtype, (None, torch.zeros(1, dtype=dtype))) is dtype
    for bad in (torch.int32, "int16", 2):
        with pytest.raises(ValueError):
            _native.emit_dtype(bad)
    with pytest.raises(ValueError):
        _native.emit_dtype(torch.int16, (torch.zeros(1, dtype=torch.float16),))


def test_c_snippet_with_a_16_bit_destination_compiles(tmp_path):
    src = tmp_path / "emit.c"
    src.write_text('#include "repet_hip.h"\n'
                   'int go(repet_online* h, const int16_t* x, int16_t* y, int16_t* z, void* stream) {\n'
                   '    const int64_t in_strides[3] = {2000, 2, 1};\n'
                   '    const int64_t out_strides[3] = {2000, 2, 1};\n'
                   '    int64_t n = 0;\n'
                   '    repet_params p;\n'
                   '    int rc = repet_derive_params(0, 8000.0, &p);\n'
                   '    if (!repet_emit_dtype_supported(REPET_I16) || !repet_emit_dtype_supported(REPET_BF16)) return REPET_ERR_BAD_ARG;\n'
                   '    if (rc == REPET_OK) rc = repet_run_device(REPET_SIM, x, REPET_I16, 1, 1000, 2, in_strides,\n'
                   '                                              y, REPET_I16, out_strides, &p, 0, stream);\n'
                   '    if (rc == REPET_OK) rc = repet_online_also_emit(h, REPET_OUT_FOREGROUND, z, REPET_I16, out_strides);\n'
                   '    if (rc == REPET_OK) rc = repet_online_push_device(h, x, REPET_I16, 1000, in_strides, stream, y, REPET_I16, out_strides,\n'
                   '                                                      stream, &n);\n'
                   '    if (rc == REPET_OK) rc = repet_online_last_emission_device(h, REPET_OUT_MIXTURE, y, REPET_F16, out_strides, stream, &n);\n'
                   '    return rc;\n'
                   '}\n')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(tmp_path / "emit.o")])


def test_device_entries_still_refuse_null_handles():
    """Without a device only the null checks in front of the dtype check are reached: they stay refusals for every code. (The
    dtype check itself runs where a device exists: tests/test_gpu_emit_dtypes.py.)"""
    lib = _native.lib()
    strides = (C.c_int64 * 3)(2, 1, 1)
    for code in (_native.I16, _native.F16, _native.BF16, 7):
        assert lib.repet_online_also_emit(None, _native.OUT_FOREGROUND, None, code, strides) == _native.ERR_BAD_ARG
        assert lib.repet_ctx_download_device_strided(None, None, code, strides, None) == _native.ERR_BAD_ARG
