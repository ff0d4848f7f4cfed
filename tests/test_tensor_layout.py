"""CPU checks of the tensor path: how a torch tensor's layout and dtype are resolved for the strided ingest (element strides
of .T and step views, the float64 fallback, the refusals), the C declarations of the device-side entries, and that torch is
not needed to import repet."""
import os
import subprocess
import sys

import numpy as np
import pytest

from repet import _native
import repet

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_contiguous_2d():
    x = torch.zeros(1000, 2, dtype=torch.float64)
    t, code, shape, strides = _native.tensor_layout(x)
    assert t is x and code == _native.F64 and shape == (1, 1000, 2) and strides == (2000, 2, 1)


def test_channels_first_view_and_step_slice_keep_their_strides():
    cf = torch.zeros(2, 1000, dtype=torch.float32)
    t, code, shape, strides = _native.tensor_layout(cf.T)
    assert code == _native.F32 and shape == (1, 1000, 2) and strides[1:] == (1, 1000)
    assert t.data_ptr() == cf.data_ptr()                      # no copy
    x = torch.zeros(2000, 2, dtype=torch.int16)
    t, code, shape, strides = _native.tensor_layout(x[::2])
    assert code == _native.I16 and shape == (1, 1000, 2) and strides[1:] == (4, 1)


def test_batch_and_batch_slice():
    xb = torch.zeros(3, 1000, 2, dtype=torch.bfloat16)
    t, code, shape, strides = _native.tensor_layout(xb, batched=True)
    assert code == _native.BF16 and shape == (3, 1000, 2) and strides == (2000, 2, 1)
    t, code, shape, strides = _native.tensor_layout(xb[1])
    assert shape == (1, 1000, 2) and strides[1:] == (2, 1) and t.data_ptr() == xb[1].data_ptr()
    t, code, shape, strides = _native.tensor_layout(torch.zeros(3, 1000, 2, dtype=torch.float16).transpose(1, 2).transpose(1, 2), batched=True)
    assert code == _native.F16


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.uint8, torch.bool])
def test_other_real_dtypes_become_float64(dtype):
    x = torch.ones(100, 2, dtype=dtype)
    t, code, shape, strides = _native.tensor_layout(x)
    assert code == _native.F64 and t.dtype == torch.float64 and strides == (200, 2, 1)
    assert torch.equal(t, x.to(torch.float64))


@pytest.mark.parametrize("shape", [(100,), (2, 100, 2), (1, 2, 3, 4)])
def test_shapes_the_numpy_path_refuses_are_refused(shape):
    with pytest.raises(ValueError):
        _native.tensor_layout(torch.zeros(shape))
    with pytest.raises(ValueError):                          # what the NumPy path's unpacking raises (repet._separate)
        number_samples, number_channels = np.shape(np.zeros(shape))


def test_batched_layout_refuses_other_ranks():
    with pytest.raises(ValueError):
        _native.tensor_layout(torch.zeros(100), batched=True)
    with pytest.raises(ValueError):
        _native.tensor_layout(torch.zeros(1, 2, 3, 4), batched=True)


def test_result_dtypes():
    assert _native.result_tensor_code(torch.zeros(1, dtype=torch.float32)) == _native.F32
    assert _native.result_tensor_code(torch.zeros(1, dtype=torch.float64)) == _native.F64
    with pytest.raises(ValueError):
        _native.result_tensor_code(torch.zeros(1, dtype=torch.float16))


def test_cpu_tensors_are_not_device_tensors():
    x = torch.zeros(10, 2)
    assert _native.is_tensor(x) and not _native.is_device_tensor(x)
    assert not _native.is_tensor(np.zeros((10, 2)))


def test_separate_refuses_host_input_and_unknown_algorithms():
    with pytest.raises(TypeError):
        repet.separate("sim", np.zeros((100, 2)), 8000)
    with pytest.raises(ValueError):
        repet.separate("nope", torch.zeros(100, 2), 8000)


def test_repet_imports_without_torch():
    code = ("import sys; sys.modules['torch'] = None; import repet; from repet import _native; "
            "assert not _native.is_tensor([1.0]); print('ok')")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "repet-python_amd"), ROOT]))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def test_c_snippet_with_the_device_entries_compiles(tmp_path):
    src = tmp_path / "dev.c"
    src.write_text('#include "repet_hip.h"\n'
                   'int go(repet_ctx* ctx, const double* x, float* y, void* stream) {\n'
                   '    const int64_t in_strides[3] = {2000, 1, 1000};\n'
                   '    const int64_t out_strides[3] = {2000, 2, 1};\n'
                   '    repet_params p;\n'
                   '    int rc = repet_derive_params(0, 44100.0, &p);\n'
                   '    if (rc == REPET_OK) rc = repet_ctx_upload_device_strided(ctx, x, REPET_F64, 1, 1000, 2, in_strides, stream);\n'
                   '    if (rc == REPET_OK) rc = repet_ctx_execute_async(ctx, REPET_SIM, &p);\n'
                   '    if (rc == REPET_OK) rc = repet_ctx_download_device_strided(ctx, y, REPET_F32, out_strides, stream);\n'
                   '    if (rc == REPET_OK) rc = repet_run_device(REPET_SIM, x, REPET_BF16 - REPET_BF16 + REPET_F64, 1, 1000, 2, in_strides,\n'
                   '                                              y, REPET_F32, out_strides, &p, 0, stream);\n'
                   '    return rc + REPET_F16;\n'
                   '}\n')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-std=c11", "-c", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(tmp_path / "dev.o")])


def test_device_entries_are_bound():
    lib = _native.lib()
    for name in ("repet_ctx_upload_device_strided", "repet_ctx_download_device_strided", "repet_run_device"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_device_entries_check_their_arguments():
    """The entries return an error for a null context or null parameters. (Without a HIP device every call fails anyway: the
    argument checks themselves are exercised where a device exists.)"""
    lib = _native.lib()
    import ctypes as C
    strides = (C.c_int64 * 3)(2, 1, 1)
    assert lib.repet_ctx_upload_device_strided(None, None, _native.F64, 1, 10, 2, strides, None) == _native.ERR_BAD_ARG
    assert lib.repet_ctx_download_device_strided(None, None, _native.F64, strides, None) == _native.ERR_BAD_ARG
    assert lib.repet_run_device(0, None, _native.F64, 1, 10, 2, strides, None, _native.F64, strides, None, 0, None) != 0


def test_host_entries_refuse_half_codes():
    """The host entries do not take REPET_F16 / REPET_BF16. Without a HIP device these calls fail whatever the dtype check
    does; the refusal itself is only exercised where a device exists."""
    lib = _native.lib()
    import ctypes as C
    x = np.zeros((10, 2), dtype=np.float16)
    out = np.zeros((10, 2))
    p = repet.derive_params(8000)
    assert lib.repet_run(0, _native.ptr(x), _native.F16, 10, 2, p, _native.ptr(out), 0, None) != 0
    ins = (C.c_void_p * 1)(x.ctypes.data)
    outs = (C.c_void_p * 1)(out.ctypes.data)
    assert lib.repet_run_batch(0, 1, ins, _native.BF16, (C.c_int64 * 1)(10), (C.c_int32 * 1)(2), p, outs, 1) != 0
