"""ctypes binding of librepet_hip.so (include/repet_hip.h). No CPU fallback: if the library or a GPU
is missing the calls raise, loudly."""
import collections
import ctypes as C
import os
import struct
import sys
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("REPET_HIP_LIB", os.path.join(os.path.dirname(_HERE), "lib", "librepet_hip.so"))

ABI_VERSION = 4
ORIGINAL, EXTENDED, ADAPTIVE, SIM, SIMONLINE = range(5)
ALGO_IDS = {"original": ORIGINAL, "extended": EXTENDED, "adaptive": ADAPTIVE, "sim": SIM, "simonline": SIMONLINE}
F32, F64, I16, F16, BF16 = 0, 1, 2, 3, 4      # (F16 / BF16: the device-side entries only)
MAX_STAGES = 16

ERR_BAD_ARG, ERR_TOO_SHORT, ERR_HIP, ERR_OOM, ERR_LIMIT = -1, -2, -3, -4, -5
FLAG_STRICT_REFERENCE = 1      # (ABI 3 opt-in; the default since ABI 4)
FLAG_REFUSE_NONFINITE = 2
FLAG_SILENT_FRAMES_ZERO = 4    # simonline and the live handles: frames of digital silence are separated, not answered with NaN
SILENT_FRAMES = {"reference": 0, "zero": FLAG_SILENT_FRAMES_ZERO}
# what an emitting call of a live handle, or the egress of a tensor call, delivers (REPET_OUT_* of include/repet_hip.h);
# "both" is the Python layer's pair (background, foreground) from one pass
OUT_BACKGROUND, OUT_FOREGROUND, OUT_MIXTURE = 0, 1, 2
WHICH_CODES = {"background": OUT_BACKGROUND, "foreground": OUT_FOREGROUND, "mixture": OUT_MIXTURE}


# the fields of a level record (REPET_LEVEL_* of include/repet_hip.h, in index order): per stream and channel the sums of
# squares and the largest magnitudes of the three signals of an emission, its live samples and those whose mixture is not finite
LEVELS = ("mixture_energy", "background_energy", "foreground_energy", "mixture_peak", "background_peak", "foreground_peak",
          "live_samples", "nonfinite_samples")
LEVEL_FIELDS = len(LEVELS)
LEVEL_CHUNK = 4096             # REPET_LEVEL_CHUNK: samples of one stream per workgroup of the reduction

# what last_matches of a live handle returns: per frame the length of its similar-frame list, and per entry how many of the
# stream's own frames back it lies (ascending; -1 behind the list) and its cosine similarity (0 behind the list)
Matches = collections.namedtuple("Matches", ["count", "age", "similarity"])


def device_out(out, shape, device, dtype=None, dtype_words="", dense=False, name="out", what="the result"):
    """The one check of a device ``out=`` tensor: on cuda:``device``, of ``dtype`` (None: any; ``dtype_words`` is the refusal,
    formatted with ``want`` and ``got``), of ``shape`` (``what`` has it) and dense, or else at least free of negative strides.
    ``name`` is what the messages call the tensor. ValueError otherwise, before anything runs."""
    import torch
    dev = torch.device("cuda", device)
    if not is_device_tensor(out) or out.device != dev:
        raise ValueError(f"{name} must be a tensor on {dev}")
    if dtype is not None and out.dtype != dtype:
        raise ValueError(dtype_words.format(want=dtype, got=out.dtype))
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"{name} has shape {tuple(out.shape)}, {what} {tuple(shape)}")
    if dense and not out.is_contiguous():
        raise ValueError(f"{name} must be dense (contiguous)")
    if not dense and any(st < 0 for st in out.stride()):
        raise ValueError(f"{name} has negative strides")
    return out


def levels_out(out, shape, device):
    """``out=`` of a levels call: None (a fresh float64 tensor of ``shape`` on cuda:``device``), or a dense float64 tensor of
    that shape there. ValueError otherwise, before anything runs."""
    import torch
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=torch.device("cuda", device))
    return device_out(out, shape, device, torch.float64, "levels are float64, out is {got}", dense=True, what="the levels")


def read_back(device, on_device, shapes, dtypes, host_call, device_call, outs=None):
    """A record of a live handle, one body for its host and device forms: NumPy arrays of ``shapes`` and ``dtypes`` filled by
    ``host_call(*arrays)``, or (``on_device``) tensors on cuda:``device`` filled by ``device_call(*tensors, stream handle)``
    behind the current stream with no host wait. ``outs``: the destinations, already checked (None: fresh ones). Either call
    returns the library's code. Returns the tuple of results."""
    if not on_device:
        results = outs or tuple(np.empty(shape, dtype=dtype) for shape, dtype in zip(shapes, dtypes))
        check(host_call(*results))
        return results
    import torch
    dev = torch.device("cuda", device)
    results = outs or tuple(torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
                            for shape, dtype in zip(shapes, dtypes))
    check(device_call(*results, _stream_handle(torch.cuda.current_stream(dev))))
    return results


def which_codes(which):
    """The REPET_OUT_* code(s) of ``which``: one for "background" / "foreground" / "mixture", the pair for "both".
    ValueError for anything else -- raised before any device is touched."""
    if which == "both":
        return (OUT_BACKGROUND, OUT_FOREGROUND)
    if not isinstance(which, str) or which not in WHICH_CODES:
        raise ValueError(f"which must be 'background', 'foreground', 'mixture' or 'both', not {which!r}")
    return (WHICH_CODES[which],)


def background_gains(gain, count=None):
    """``gain`` as a float32 array: a scalar (``count`` None), or one value per named slot -- a scalar is repeated ``count``
    times. ValueError, before any device is touched, for a value that is NaN, infinite or outside [0, 1] (checked on the float32
    value the library takes) or for another number of values than slots."""
    try:
        g = np.asarray(gain, dtype=np.float64).astype(np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"background_gain must be a number in [0, 1], not {gain!r}") from None
    if count is None:
        if g.ndim != 0:
            raise ValueError("background_gain is one number here")
        g = g.reshape(1)
    elif g.ndim == 0:
        g = np.full(count, g, dtype=np.float32)
    elif g.ndim != 1 or g.size != count:
        raise ValueError(f"{g.size} background gains for {count} slots")
    if not np.all((g >= 0) & (g <= 1)):
        raise ValueError(f"background_gain must lie in [0, 1] (NaN and infinities are refused), not {gain!r}")
    return np.ascontiguousarray(g)


def band_gain_rows(gains, edges, bins, count=None):
    """``gains`` / ``edges`` of ``set_background_band_gains`` as what the library takes: ``(edges, g)`` with ``edges`` None (one
    gain per bin, ``bins`` of them) or the int32 array of ``band_edge_array`` with at most ``bins`` bands, and ``g`` float32
    ``(rows, n_bands)`` with ``rows`` 1, or ``count`` where one row per named slot was given. ValueError, before any device is
    touched, for a value that is NaN, infinite or outside [0, 1] (checked on the float32 value the library takes), edges that
    are not ascending bins in [0, bins], or a wrong size."""
    if edges is not None:
        edges = band_edge_array(edges)
        if edges.size - 1 > bins or (edges < 0).any() or (edges > bins).any() or (np.diff(edges) < 0).any():
            raise ValueError(f"edges are at most {bins} bands: ascending bin edges in [0, {bins}]")
    n_bands = bins if edges is None else edges.size - 1
    try:
        g = np.asarray(gains, dtype=np.float64).astype(np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"band gains must be numbers in [0, 1], not {gains!r}") from None
    if g.ndim == 1:
        g = g.reshape(1, -1)
    if g.ndim != 2 or g.shape[1] != n_bands or (g.shape[0] != 1 and g.shape[0] != count):
        what = f"({n_bands},)" + ("" if count is None else f" or ({count}, {n_bands})")
        raise ValueError(f"band gains of shape {np.shape(gains)}: {what} is expected")
    if not np.all((g >= 0) & (g <= 1)):
        raise ValueError("band gains must lie in [0, 1] (NaN and infinities are refused)")
    return edges, np.ascontiguousarray(g)


def g_rows(gains):
    """The number of rows a two-dimensional ``gains`` has (None for anything else: ``band_gain_rows`` then expects one row)."""
    shape = np.shape(gains) if not hasattr(gains, "shape") else tuple(gains.shape)
    return int(shape[0]) if len(shape) == 2 else None


def _set_band_gains(handle_of, slots, n_slots, gains, edges, bins, count):
    """(the arguments are checked before the handle is looked at: ``handle_of`` returns it)"""
    edges, g = band_gain_rows(gains, edges, bins, count)
    check(lib().repet_online_set_background_band_gains(handle_of(), slots, n_slots, None if edges is None else ptr(edges), g.shape[1],
                                                       ptr(g), g.shape[0]))


def _get_band_gains(handle, slot, bins):
    out = np.zeros(bins, dtype=np.float32)
    check(lib().repet_online_background_band_gains(handle, slot, ptr(out), bins))
    return out


class Params(C.Structure):
    _fields_ = [("window_length", C.c_int32), ("step_length", C.c_int32), ("period_lo", C.c_int32),
                ("period_hi", C.c_int32), ("cutoff_bins", C.c_int32), ("filter_order", C.c_int32),
                ("seg_len_frames", C.c_int32), ("seg_step_frames", C.c_int32),
                ("sim_distance_frames", C.c_int32), ("sim_number", C.c_int32), ("buffer_frames", C.c_int32),
                ("flags", C.c_int32), ("seg_len_samples", C.c_int64), ("seg_step_samples", C.c_int64),
                ("sim_threshold", C.c_double)]


class Settings(C.Structure):
    """repet_settings of include/repet_hip.h: the nine module-level parameters of the reference."""
    _fields_ = [("cutoff_frequency", C.c_double), ("period_range", C.c_double * 2), ("segment_length", C.c_double),
                ("segment_step", C.c_double), ("similarity_threshold", C.c_double), ("similarity_distance", C.c_double),
                ("buffer_length", C.c_double), ("filter_order", C.c_int32), ("similarity_number", C.c_int32)]


class WavInfo(C.Structure):
    """repet_wav_info of include/repet_hip.h."""
    _fields_ = [("format", C.c_int32), ("n_channels", C.c_int32), ("sampling_frequency", C.c_int32),
                ("bits_per_sample", C.c_int32), ("bytes_per_sample", C.c_int32), ("reserved0", C.c_int32),
                ("data_offset", C.c_int64), ("n_samples", C.c_int64)]


class Timing(C.Structure):
    _fields_ = [("n_stages", C.c_int32), ("reserved0", C.c_int32), ("total_ms", C.c_float),
                ("stage_ms", C.c_float * MAX_STAGES), ("stage_name", (C.c_char * 24) * MAX_STAGES),
                ("stage_bytes", C.c_double * MAX_STAGES), ("stage_flops", C.c_double * MAX_STAGES)]

    def as_dict(self):
        stages = []
        for i in range(self.n_stages):
            stages.append({"name": self.stage_name[i].value.decode(), "ms": float(self.stage_ms[i]),
                           "bytes": float(self.stage_bytes[i]), "flops": float(self.stage_flops[i])})
        return {"total_ms": float(self.total_ms), "stages": stages}


_P = C.c_void_p
_SIGNATURES = {
    "repet_abi_version": (C.c_int, []),
    "repet_device_count": (C.c_int, []),
    "repet_device_host_cpus": (C.c_int, [C.c_int, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]),
    "repet_last_error": (C.c_char_p, []),
    "repet_default_settings": (None, [C.POINTER(Settings)]),
    "repet_derive_params": (C.c_int, [C.POINTER(Settings), C.c_double, C.POINTER(Params)]),
    "repet_ctx_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "repet_ctx_destroy": (C.c_int, [_P]),
    "repet_ctx_upload": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int32]),
    "repet_ctx_upload_batch": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int32, C.c_int32]),
    "repet_ctx_execute": (C.c_int, [_P, C.c_int, C.POINTER(Params), C.POINTER(Timing)]),
    "repet_ctx_download": (C.c_int, [_P, _P]),
    "repet_ctx_upload_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32]),
    "repet_ctx_upload_device_split": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32]),
    "repet_ctx_download_device": (C.c_int, [_P, _P]),
    "repet_ctx_upload_device_strided": (C.c_int, [_P, _P, C.c_int, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64), _P]),
    "repet_ctx_download_device_strided": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int64), _P]),
    "repet_ctx_upload_device_ragged": (C.c_int, [_P, _P, C.c_int, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    "repet_ctx_clip_lengths": (C.c_int, [_P, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int32)]),
    "repet_check_clip_lengths": (C.c_int, [C.c_int, C.POINTER(Params), C.c_int32, C.POINTER(C.c_int64), C.c_int32]),
    "repet_last_batch_info": (C.c_int, [C.POINTER(C.c_int64)]),
    "repet_ctx_download_input": (C.c_int, [_P, _P, _P, C.POINTER(C.c_int32)]),
    "repet_ctx_set_window": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "repet_ctx_set_strict_reference": (C.c_int, [_P, C.c_int]),
    "repet_ctx_stream": (C.c_int, [_P, C.POINTER(_P)]),
    "repet_ctx_result_view": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "repet_ctx_input_view": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int64)]),
    "repet_ctx_download_from": (C.c_int, [_P, _P, C.c_int64, _P]),
    "repet_ctx_execute_extended_range_async": (C.c_int, [_P, C.POINTER(Params), C.c_int64, C.c_int64]),
    "repet_wav_parse": (C.c_int, [_P, C.c_int64, C.POINTER(WavInfo)]),
    "repet_ctx_upload_wav": (C.c_int, [_P, _P, C.c_int64, C.POINTER(WavInfo)]),
    "repet_ctx_result_wav": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "repet_ctx_set_sampling_frequency": (C.c_int, [_P, C.c_int32]),
    "repet_host_alloc": (C.c_void_p, [C.c_size_t]),
    "repet_host_free": (None, [C.c_void_p]),
    "repet_ctx_execute_async": (C.c_int, [_P, C.c_int, C.POINTER(Params)]),
    "repet_ctx_synchronize": (C.c_int, [_P]),
    "repet_ctx_timing_series_begin": (C.c_int, [_P, C.c_int32]),
    "repet_ctx_timing_series_end": (C.c_int, [_P, C.POINTER(Timing), C.POINTER(C.c_int32)]),
    "repet_ctx_download_foreground": (C.c_int, [_P, _P]),
    "repet_ctx_spectrogram": (C.c_int, [_P, C.c_int, C.c_int32, _P, C.c_int64]),
    "repet_extended_segment_count": (C.c_int64, [C.c_int64, C.POINTER(Params)]),
    "repet_ctx_execute_extended_range": (C.c_int, [_P, C.POINTER(Params), C.c_int64, C.c_int64, C.POINTER(Timing)]),
    "repet_release_thread_ctx": (C.c_int, []),
    "repet_median_network_info": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "repet_run": (C.c_int, [C.c_int, _P, C.c_int, C.c_int64, C.c_int32, C.POINTER(Params), _P, C.c_int,
                            C.POINTER(Timing)]),
    "repet_run_batch": (C.c_int, [C.c_int, C.c_int32, C.POINTER(_P), C.c_int, C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int32), C.POINTER(Params), C.POINTER(_P), C.c_int32]),
    "repet_run_batch_rccl": (C.c_int, [C.c_int, C.c_int32, C.POINTER(_P), C.c_int, C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int32), C.POINTER(Params), C.POINTER(_P), C.c_int32]),
    "repet_run_stream": (C.c_int, [C.c_int, C.c_int32, C.POINTER(_P), C.c_int, C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int32), C.POINTER(Params), C.POINTER(_P), C.c_int, C.c_int32]),
    "repet_run_device": (C.c_int, [C.c_int, _P, C.c_int, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64), _P, C.c_int,
                                   C.POINTER(C.c_int64), C.POINTER(Params), C.c_int, _P]),
    "repet_host_conversion_selftest": (C.c_int64, [C.c_int64, C.c_uint32]),
    "repet_frame_count": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "repet_stft": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64]),
    "repet_istft": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32, C.c_int32, _P, C.c_int64]),
    "repet_selfsim": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P]),
    "repet_selfsim_records": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P, _P]),
    "repet_debug_gram_full_stage": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32]),
    "repet_similarity": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.c_int32, _P]),
    "repet_acorr": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P]),
    "repet_beat_spectrum": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int32]),
    "repet_beat_spectrogram": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P]),
    "repet_periods": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "repet_local_maxima": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, _P, _P]),
    "repet_mask_period": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P]),
    "repet_mask_adaptive": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, C.c_int32, _P]),
    "repet_mask_sim": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, C.c_int32, _P]),
    "repet_rank_columns": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P]),
    "repet_mask_sim_ranked": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "repet_ctx_last_periods": (C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    "repet_ctx_last_median_path": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "repet_ctx_last_median_codes": (C.c_int, [_P, _P, C.c_int64, C.c_int32]),
    "repet_ctx_last_sim_indices": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32]),
    "repet_ctx_last_sim_indices_clip": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int32, C.c_int32]),
    "repet_ctx_last_clip_passes": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "repet_ctx_last_frame_count": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "repet_ctx_last_refine_stats": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "repet_ctx_last_exact_stats": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "repet_online_open": (C.c_int, [C.c_int, C.c_int32, C.POINTER(Params), C.POINTER(_P)]),
    "repet_online_push": (C.c_int, [_P, _P, C.c_int, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "repet_online_finish": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "repet_online_close": (C.c_int, [_P]),
    "repet_online_open_streams": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.POINTER(Params), C.c_int64, C.POINTER(_P)]),
    "repet_online_emit_count": (C.c_int, [_P, C.c_int64, C.c_int, C.POINTER(C.c_int64)]),
    "repet_online_push_streams": (C.c_int, [_P, _P, C.c_int, C.c_int64, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "repet_online_push_device": (C.c_int, [_P, _P, C.c_int, C.c_int64, _P, _P, _P, C.c_int, _P, _P, C.POINTER(C.c_int64)]),
    "repet_online_finish_streams": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "repet_online_finish_device": (C.c_int, [_P, _P, C.c_int, _P, _P, C.POINTER(C.c_int64)]),
    "repet_online_restart_streams": (C.c_int, [_P, _P, C.c_int32]),
    "repet_online_release_streams": (C.c_int, [_P, _P, C.c_int32]),
    "repet_online_stream_emit_count": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int64)]),
    "repet_online_finish_stream": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "repet_online_finish_stream_device": (C.c_int, [_P, C.c_int32, _P, C.c_int, _P, _P, C.POINTER(C.c_int64)]),
    "repet_online_stream_state_size": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "repet_online_export_stream": (C.c_int, [_P, C.c_int32, _P, _P]),
    "repet_online_export_stream_device": (C.c_int, [_P, C.c_int32, _P, _P, _P]),
    "repet_online_import_stream": (C.c_int, [_P, C.c_int32, _P, _P]),
    "repet_online_import_stream_device": (C.c_int, [_P, C.c_int32, _P, _P, _P]),
    "repet_online_set_output": (C.c_int, [_P, C.c_int]),
    "repet_online_also_emit": (C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    "repet_online_last_emission": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "repet_online_last_emission_device": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P, C.POINTER(C.c_int64)]),
    "repet_ctx_select_result": (C.c_int, [_P, C.c_int]),
    "repet_online_set_start_frames": (C.c_int, [_P, C.c_int32]),
    "repet_online_start_frames": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "repet_ctx_set_online_start": (C.c_int, [_P, C.c_int32]),
    "repet_select_run_result": (C.c_int, [C.c_int, C.c_int]),
    "repet_online_set_background_gain": (C.c_int, [_P, _P, C.c_int32, _P]),
    "repet_online_background_gain": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_float)]),
    "repet_online_set_background_band_gains": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32]),
    "repet_online_background_band_gains": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "repet_ctx_set_background_gain": (C.c_int, [_P, C.c_float]),
    "repet_set_run_background_gain": (C.c_int, [C.c_int, C.c_float]),
    "repet_ctx_set_background_band_gains": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, C.c_int32]),
    "repet_ctx_background_band_gains": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "repet_set_run_background_band_gains": (C.c_int, [C.c_int, C.c_int32, _P, C.c_int32, _P, C.c_int32]),
    "repet_online_last_levels": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "repet_online_last_levels_device": (C.c_int, [_P, _P, _P]),
    "repet_ctx_result_levels_device": (C.c_int, [_P, _P, _P]),
    "repet_emit_dtype_supported": (C.c_int, [C.c_int]),
    "repet_silent_frames_supported": (C.c_int, []),
    "repet_online_hold_streams": (C.c_int, [_P, _P, C.c_int32]),
    "repet_online_resume_streams": (C.c_int, [_P, _P, C.c_int32]),
    "repet_online_stream_held": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int32)]),
    "repet_online_last_frame_range": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "repet_online_last_frames": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "repet_online_last_frames_device": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "repet_online_last_band_energies": (C.c_int, [_P, C.c_int, _P, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "repet_online_last_band_energies_device": (C.c_int, [_P, C.c_int, _P, C.c_int32, _P, _P]),
    "repet_online_match_capacity": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "repet_online_last_matches": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "repet_online_last_matches_device": (C.c_int, [_P, _P, _P, _P, _P]),
    "repet_online_enable_feed": (C.c_int, [_P, C.c_int64]),
    "repet_online_feed": (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int, C.c_int64]),
    "repet_online_feed_device": (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_int, C.c_int64, _P, _P, _P]),
    "repet_online_queued": (C.c_int, [_P, C.c_int32, _P]),
    "repet_online_pad_feed": (C.c_int, [_P, _P, C.c_int32, _P]),
    "repet_online_clear_feed": (C.c_int, [_P, _P, C.c_int32]),
    "repet_online_tick": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _P, C.POINTER(C.c_int64)]),
    "repet_online_tick_device": (C.c_int, [_P, C.c_int64, _P, C.c_int, _P, _P, _P, C.POINTER(C.c_int64)]),
    "repet_ctx_request_frames": (C.c_int, [_P, C.c_int, _P, C.c_int32, _P, _P, _P]),
    "repet_ctx_clear_requests": (C.c_int, [_P]),
    "repet_result_frame_count": (C.c_int64, [C.c_int, C.POINTER(Params), C.c_int64]),
    "repet_ctx_last_spectrum_form": (C.c_int, [_P, C.POINTER(C.c_int32)]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def _preload_hip_runtime():
    """One HIP runtime per process. PyTorch-ROCm wheels bundle their own libamdhip64 with the system library's soname, so
    whichever is loaded first serves both; with the system one first, a later ``import torch`` finds no GPU (its other
    bundled libraries do not match). When a PyTorch-ROCm is installed its runtime is therefore loaded first -- found on
    disk, not imported. REPET_HIP_RUNTIME=system skips this."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("REPET_HIP_RUNTIME") == "system":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    bundled = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(bundled):
        try:
            C.CDLL(bundled, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load librepet_hip.so once. Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"librepet_hip.so not found at {LIB_PATH}: build it with `make -C repet-python_amd/csrc` "
                "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
        _preload_hip_runtime()
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        if handle.repet_abi_version() != ABI_VERSION:
            raise RuntimeError("librepet_hip.so ABI version mismatch")
        _lib = handle
    return _lib


def check(rc):
    if rc == 0:
        return
    msg = lib().repet_last_error().decode(errors="replace")
    if rc in (ERR_BAD_ARG, ERR_TOO_SHORT):
        raise ValueError(msg)
    if rc == ERR_OOM:
        raise MemoryError(msg)
    raise RuntimeError(f"librepet_hip error {rc}: {msg}")


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def as_input(audio_signal):
    """(array, dtype code) in a layout/dtype the ABI takes without a host-side conversion pass."""
    a = np.asarray(audio_signal)
    if a.dtype == np.float64:
        code = F64
    elif a.dtype == np.float32:
        code = F32
    elif a.dtype == np.int16:
        code = I16
    else:
        a = a.astype(np.float64)
        code = F64
    return np.ascontiguousarray(a), code


# ---- torch tensors on a ROCm device (devio.hip) ----------------------------------------------------------------------
# torch is never imported here: a tensor is recognised by its type once the caller has imported torch, so a host without
# torch still imports repet.
_TENSOR_CODES = {"torch.float64": F64, "torch.float32": F32, "torch.int16": I16, "torch.float16": F16, "torch.bfloat16": BF16}


def is_tensor(x):
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(x, torch.Tensor)


def is_device_tensor(x):
    """A torch tensor in GPU memory (ROCm devices are torch's "cuda" devices); CPU tensors take the NumPy path."""
    return is_tensor(x) and x.device.type == "cuda"


def tensor_layout(x, batched=False):
    """(tensor, dtype code, (n_clips, n_samples, n_channels), element strides) of a tensor as the strided ingest reads it.
    ``batched``: ``(N, C)`` or ``(B, N, C)``; otherwise ``(N, C)`` only (ValueError like the NumPy path's ``np.shape``
    unpacking). Real dtypes the ingest does not take are converted with ``x.to(torch.float64)`` (what ``as_input``'s
    ``astype(float64)`` does); negative strides fall back to a contiguous copy."""
    import torch
    if x.dim() != 2 and not (batched and x.dim() == 3):
        raise ValueError("audio_signal must be (number_samples, number_channels)" +
                         (" or (number_clips, number_samples, number_channels)" if batched else ""))
    code = _TENSOR_CODES.get(str(x.dtype))
    if code is None:
        x = x.to(torch.float64)
        code = F64
    if any(st < 0 for st in x.stride()):
        x = x.contiguous()
    shape = tuple(int(d) for d in x.shape)
    strides = tuple(int(st) for st in x.stride())
    if x.dim() == 2:
        shape = (1,) + shape
        strides = (shape[1] * shape[2],) + strides
    return x, code, shape, strides


def clip_lengths(lengths, shape):
    """``lengths=`` of a ragged batch against the shape of its padded tensor, before the library is touched: a sequence of ``B``
    integers on the HOST (a list or tuple, a NumPy integer array, a CPU tensor of an integer dtype), each in ``[0, N]``. Returns a
    tuple of ints -- or None where every clip is ``N`` long, which is the equal-length call. TypeError for a tensor on a device
    (frame counts and the too-short checks are host decisions: the call must not wait for the device) and for values that are not
    integers; ValueError for a tensor that is not ``(B, N, C)``, a wrong count or a value outside ``[0, N]``."""
    import numbers
    if is_tensor(lengths):
        if lengths.device.type != "cpu":
            raise TypeError("lengths must be on the host (a list, a NumPy array or a CPU tensor), not on a device")
        if lengths.is_floating_point() or lengths.is_complex() or str(lengths.dtype) == "torch.bool":
            raise TypeError("lengths must be integers")
        lengths = lengths.tolist()
    elif isinstance(lengths, np.ndarray):
        if lengths.dtype.kind not in "iu":
            raise TypeError("lengths must be integers")
        lengths = lengths.tolist()
    if isinstance(lengths, (str, bytes)) or not hasattr(lengths, "__len__") or not hasattr(lengths, "__iter__"):
        raise TypeError("lengths must be a sequence of integers, one per clip")
    values = list(lengths)
    for v in values:
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise TypeError("lengths must be integers")
    shape = tuple(shape)
    if len(shape) != 3:
        raise ValueError("lengths go with a batch (number_clips, number_samples, number_channels) only")
    if len(values) != int(shape[0]):
        raise ValueError(f"lengths has {len(values)} entries, the batch {int(shape[0])} clips")
    n = int(shape[1])
    for b, v in enumerate(values):
        if v < 0 or v > n:
            raise ValueError(f"lengths[{b}] = {int(v)} lies outside [0, {n}]")
    values = tuple(int(v) for v in values)
    return None if all(v == n for v in values) else values


def check_clip_lengths(algo, params, lengths, start_frames=0):
    """The refusal a ragged batch's execute would make of a clip too short for ``algo``, made before anything is uploaded or
    enqueued: ValueError with the one-clip call's text and the clip named in front."""
    arr = (C.c_int64 * len(lengths))(*lengths)
    check(lib().repet_check_clip_lengths(ALGO_IDS[algo], params, int(start_frames), arr, len(lengths)))


def result_tensor_code(out):
    code = {"torch.float64": F64, "torch.float32": F32}.get(str(out.dtype))
    if code is None:
        raise ValueError("out must be a float32 or float64 tensor")
    return code


def emit_tensor_code(out):
    """The dtype code of a destination tensor of the device-side egress (a live handle's ``out=``, ``download_tensor``,
    ``repet.separate``): float64, float32, int16, float16 or bfloat16 -- each the inverse of the same source dtype, a cast of
    the float64 value the engine holds and never a rescale. ValueError for anything else."""
    code = _TENSOR_CODES.get(str(out.dtype))
    if code is None:
        raise ValueError("out must be a float64, float32, int16, float16 or bfloat16 tensor")
    return code


def emit_dtype(dtype, outs=()):
    """``dtype=`` of a device-path call: the torch dtype of a fresh result -- ``dtype``, or float64 for None. ValueError, before
    anything runs, for a dtype the egress does not write and for an ``out`` tensor (None entries skipped) of another dtype."""
    import torch
    if dtype is None:
        return torch.float64
    if not isinstance(dtype, torch.dtype) or str(dtype) not in _TENSOR_CODES:
        raise ValueError(f"dtype must be torch.float64, float32, int16, float16 or bfloat16, not {dtype!r}")
    for o in outs:
        if o is not None and is_tensor(o) and o.dtype != dtype:
            raise ValueError(f"dtype is {dtype}, out is {o.dtype}")
    return dtype


def _strides(strides):
    return (C.c_int64 * 3)(*strides)


def out_pair(out):
    """``out=`` of a ``which="both"`` call: None, or a pair of tensors (background, foreground) that share no memory."""
    if out is None:
        return None, None
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise ValueError('which="both" takes out=(background, foreground), a pair of tensors')
    a, b = out
    if is_tensor(a) and is_tensor(b) and a.dtype != b.dtype:
        raise ValueError("the two tensors of out have one dtype")
    if is_device_tensor(a) and is_device_tensor(b) and a.numel() and b.numel():
        span = lambda t: (t.data_ptr(), t.data_ptr() + (sum(st * (d - 1) for st, d in zip(t.stride(), t.shape)) + 1) * t.element_size())
        (a0, a1), (b0, b1) = span(a), span(b)
        if a0 < b1 and b0 < a1:
            raise ValueError("the two tensors of out overlap (their address ranges must not intersect)")
    return a, b


def _stream_handle(stream):
    return C.c_void_p(int(stream.cuda_stream) or None)


_tensor_ctx = threading.local()


def tensor_context(device):
    """This thread's context for tensors on ``device`` (one per thread and device, like repet_run's)."""
    ctxs = getattr(_tensor_ctx, "by_device", None)
    if ctxs is None:
        ctxs = _tensor_ctx.by_device = {}
    ctx = ctxs.get(device)
    if ctx is None:
        ctx = ctxs[device] = Context(device)
    return ctx


def release_tensor_contexts():
    for ctx in getattr(_tensor_ctx, "by_device", {}).values():
        ctx.close()
    _tensor_ctx.by_device = {}


def result_array(shape):
    """A fresh C-contiguous float64 array for a result, backed by a pinned host buffer of the library's recycling pool
    (repet_host_alloc): when the caller drops the array its buffer goes back to the pool, so the next result lands in
    memory that is already faulted in and pinned -- a fresh np.empty of a 3-minute clip takes 31 000 page faults on
    first touch. Falls back to np.empty when the pool declines (REPET_PINNED_RESULTS=0, or too much outstanding)."""
    count = 1
    for d in shape:
        count *= int(d)
    if count == 0 or os.environ.get("REPET_PINNED_RESULTS") == "0":
        return np.empty(shape, dtype=np.float64)
    address = lib().repet_host_alloc(count * 8)
    if not address:
        return np.empty(shape, dtype=np.float64)
    buffer = (C.c_double * count).from_address(address)
    weakref.finalize(buffer, lib().repet_host_free, address)      # the array (and every view of it) keeps `buffer` alive
    return np.frombuffer(buffer, dtype=np.float64, count=count).reshape(shape)


class Context:
    """One device context: upload a clip once, execute variants on the resident copy, download."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        if lib().repet_device_count() < 1:
            raise RuntimeError("no HIP device visible: the REPET engine has no CPU fallback")
        check(lib().repet_ctx_create(int(device), C.byref(self._h)))
        self._device = int(device)
        self._torch_stream = None
        self._ingested = None
        self.shape = None

    def close(self):
        if self._h:
            lib().repet_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    @property
    def handle(self):
        return self._h

    def upload(self, audio_signal):
        n, c = np.shape(audio_signal)
        a, code = as_input(audio_signal)
        check(lib().repet_ctx_upload(self._h, ptr(a), code, n, c))
        self.shape = (n, c)

    def upload_batch(self, audio_signals):
        """Equal-shape clips ``(number_clips, number_samples, number_channels)`` (or a list of such clips) made
        resident together; ``download`` then returns the same shape. ``simonline`` runs every stage once over
        all of them."""
        clips = np.stack([np.asarray(a) for a in audio_signals]) if not isinstance(audio_signals, np.ndarray) else audio_signals
        if clips.ndim != 3:
            raise ValueError("audio_signals must be (number_clips, number_samples, number_channels)")
        b, n, c = clips.shape
        a, code = as_input(clips.reshape(b * n, c))
        check(lib().repet_ctx_upload_batch(self._h, ptr(a), code, n, c, b))
        self.shape = (b, n, c)

    def upload_device(self, data_ptr, number_samples, number_channels, number_clips=1, remainder_ptr=None):
        """fp32 interleaved samples already in device memory (e.g. ``tensor.data_ptr()`` of what an RCCL recv filled;
        its producer must have finished: synchronise that stream first). No host bounce. ``remainder_ptr``: the fp32
        remainders of a float64 waveform (``x - float64(float32(x))``) in the same layout -- with them the float64 decisions
        of the peak picking see what a single-GPU call on the float64 array sees."""
        check(lib().repet_ctx_upload_device_split(self._h, C.c_void_p(int(data_ptr)), C.c_void_p(int(remainder_ptr)) if remainder_ptr else None,
                                                  int(number_samples), int(number_channels), int(number_clips)))
        self.shape = (number_samples, number_channels) if number_clips == 1 else (number_clips, number_samples, number_channels)

    def upload_tensor(self, x, stream=None, lengths=None):
        """A ``(N, C)`` or ``(B, N, C)`` torch tensor on this context's device (float64 / float32 / int16 / float16 / bfloat16,
        any non-negative strides; other real dtypes are converted to float64) becomes the resident clip(s), narrowed on the
        device. ``lengths`` (a host sequence of ``B`` integers in ``[0, N]``, with a ``(B, N, C)`` tensor): a RAGGED batch --
        clip ``b`` is ``x[b, :lengths[b]]``, the samples behind it are never read, and ``execute``, ``download_tensor`` and
        ``result_levels`` follow the lengths (see ``repet.separate``); ``shape`` stays the padded shape. Ordered behind ``stream`` (default: the tensor device's current stream) by an event, and ``stream`` behind
        the ingest: no host wait, except in the refusal mode (``set_strict_reference(False)``), which reads back whether a
        sample was not finite."""
        if not is_device_tensor(x):
            raise TypeError("upload_tensor takes a torch tensor on a ROCm device")
        if lengths is not None:
            lengths = clip_lengths(lengths, x.shape)
        return self.upload_layout(*tensor_layout(x, batched=True), stream=stream, lengths=lengths)

    def clip_lengths(self):
        """The lengths of the resident batch's clips, a tuple of ints: what a ragged ``upload_tensor`` was given, the common
        length of an equal batch otherwise. ``shape`` stays the padded shape."""
        n = C.c_int32()
        check(lib().repet_ctx_clip_lengths(self._h, None, 0, C.byref(n)))
        out = (C.c_int64 * max(n.value, 1))()
        check(lib().repet_ctx_clip_lengths(self._h, out, n.value, C.byref(n)))
        return tuple(int(v) for v in out[:n.value])

    def upload_layout(self, x, code, shape, strides, stream=None, lengths=None):
        """``upload_tensor`` of a tensor whose layout ``tensor_layout`` has already resolved. ``lengths``: None, or what
        ``clip_lengths`` returned for a ragged batch."""
        import torch
        if x.device.index != self._device:
            raise ValueError(f"tensor is on {x.device}, the context on device {self._device}")
        if stream is None:
            stream = torch.cuda.current_stream(x.device)
        if lengths is None:
            check(lib().repet_ctx_upload_device_strided(self._h, C.c_void_p(x.data_ptr() or None), code, shape[0], shape[1], shape[2],
                                                        _strides(strides), _stream_handle(stream)))
        else:
            check(lib().repet_ctx_upload_device_ragged(self._h, C.c_void_p(x.data_ptr() or None), code, shape[0], shape[1], shape[2],
                                                       _strides(strides), (C.c_int64 * len(lengths))(*lengths), _stream_handle(stream)))
        # The tensor's memory must not be reused under the ingest. `stream` waits for the ingest (an event on the engine's
        # stream) and the tensor is recorded on `stream`: the caching allocator then hands the block out again only behind
        # it. (Recording it on the engine's stream itself would leave torch holding that stream's handle for as long as the
        # block lives -- past release_workspaces(), which destroys the stream.) One event, re-recorded: a wait already
        # enqueued keeps the point it was given.
        if self._ingested is None:
            self._ingested = torch.cuda.Event()
        self._ingested.record(self.torch_stream())
        stream.wait_event(self._ingested)
        x.record_stream(stream)
        self.shape = shape[1:] if x.dim() == 2 else shape
        return x

    def download_tensor(self, out=None, stream=None, which="background", dtype=None):
        """The result of the last run into ``out`` (a float64, float32, int16, float16 or bfloat16 tensor of the resident
        shape, any non-negative strides whose elements do not overlap) or a fresh tensor of ``dtype`` (None: float64), written
        on the engine's stream behind what ``stream`` (default: the current stream of this context's device) has enqueued so
        far; ``stream`` then waits for it. No host wait. ``which``: "background", "foreground" (resident input - background,
        from the samples and, after a float64 upload, their remainders) or "mixture". A 16-bit destination takes the float64
        value rounded once, to nearest, ties to even -- a cast, never a rescale (int16 saturates, NaN is 0); ``dtype`` beside an
        ``out`` of another dtype is a ValueError."""
        import torch
        codes = which_codes(which)
        if len(codes) != 1:
            raise ValueError("download_tensor writes one signal (repet.separate pairs two calls for \"both\")")
        code = codes[0]
        device = torch.device("cuda", self._device)
        dtype = emit_dtype(dtype, (out,))
        if out is None:
            out = torch.empty(self.shape, dtype=dtype, device=device)
        elif not is_device_tensor(out) or out.device != device:
            raise ValueError(f"out must be a tensor on {device}")
        if tuple(out.shape) != tuple(self.shape):
            raise ValueError(f"out has shape {tuple(out.shape)}, the result {tuple(self.shape)}")
        if any(st < 0 for st in out.stride()):
            raise ValueError("out has negative strides")
        strides = tuple(int(st) for st in out.stride())
        if out.dim() == 2:
            strides = (out.shape[0] * out.shape[1],) + strides
        if stream is None:
            stream = torch.cuda.current_stream(device)
        out_code = emit_tensor_code(out)
        check(lib().repet_ctx_select_result(self._h, code))
        try:
            check(lib().repet_ctx_download_device_strided(self._h, C.c_void_p(out.data_ptr() or None), out_code,
                                                          _strides(strides), _stream_handle(stream)))
        finally:
            lib().repet_ctx_select_result(self._h, OUT_BACKGROUND)
        return out

    def result_levels(self, out=None, stream=None):
        """The levels of the resident result (``repet.LEVELS``): a float64 tensor ``(C, 8)``, or ``(B, C, 8)`` for a batch, on
        this context's device -- ``out`` (dense float64 of that shape) or a fresh one --, reduced on the engine's stream and
        ordered on ``stream`` (default: the current one) like ``download_tensor``. Every sample is live; the foreground is
        the one ``set_background_gain`` describes. No host wait."""
        import torch
        if self.shape is None:
            raise ValueError("no clip uploaded")
        shape = tuple(self.shape[:-2]) + (self.shape[-1], LEVEL_FIELDS)
        out = levels_out(out, shape, self._device)
        if stream is None:
            stream = torch.cuda.current_stream(out.device)
        check(lib().repet_ctx_result_levels_device(self._h, C.c_void_p(out.data_ptr()), _stream_handle(stream)))
        return out

    def set_background_gain(self, gain):
        """The foreground ``download_tensor`` writes from now on keeps ``gain`` (in [0, 1]) of the background:
        ``x - float32(1 - gain) * background``. 0, the default, is the plain foreground. ValueError outside [0, 1]."""
        g = background_gains(gain)
        check(lib().repet_ctx_set_background_gain(self._h, float(g[0])))

    def set_background_band_gains(self, gains, edges=None, window_length=None):
        """Keep a share of the background BAND BY BAND in the foreground of the runs enqueued from now on: ``gains`` in [0, 1],
        ``(n_bands,)`` or one row per clip of the batch that will be resident, ``(B, n_bands)``; ``edges`` the ``n_bands + 1``
        ascending bin edges in ``[0, window_length / 2 + 1]`` (``repet.band_edges`` fits) or None for one gain per bin.
        ``window_length`` is the one of the runs to come (``derive_params(fs).window_length``), at most 4096. The foreground is
        ``x - float32(1 - background_gain) * shaped``, where ``shaped`` is the variant's inverse STFT of the masked spectrum with
        bin ``k`` multiplied by ``float32(1 - g[k])``; background, mixture and everything else keep their bits. The table in
        force when ``execute`` / ``execute_async`` is enqueued shapes that run's result, whatever is set afterwards. ValueError,
        before the library is touched, for gains outside [0, 1] (NaN included), bad edges or a wrong size."""
        if window_length is None:
            raise ValueError("window_length of the runs the table is for (derive_params(fs).window_length)")
        w = int(window_length)
        if w < 64 or w > 8192 or w & (w - 1):
            raise ValueError("window_length must be a power of two in [64, 8192]")
        bins = w // 2 + 1
        edges, g = band_gain_rows(gains, edges, bins, g_rows(gains))
        check(lib().repet_ctx_set_background_band_gains(self._h, w, None if edges is None else ptr(edges), g.shape[1], ptr(g), g.shape[0]))
        self._band_bins = bins

    def background_band_gains(self, clip=0):
        """The float32 ``(F,)`` table in force for ``clip`` (a host copy); None when no table is set."""
        bins = getattr(self, "_band_bins", None)
        if bins is None:
            return None
        out = np.zeros(bins, dtype=np.float32)
        check(lib().repet_ctx_background_band_gains(self._h, int(clip), ptr(out), bins))
        return out

    def clear_background_band_gains(self):
        """No table: the runs enqueued from now on take the plain path."""
        check(lib().repet_ctx_set_background_band_gains(self._h, 0, None, 0, None, 0))
        self._band_bins = None

    def torch_stream(self):
        """The context's stream as a ``torch.cuda.ExternalStream`` (cached)."""
        if self._torch_stream is None:
            import torch
            self._torch_stream = torch.cuda.ExternalStream(self.stream(), device=torch.device("cuda", self._device))
        return self._torch_stream

    def resident_input(self):
        """(fp32 samples, fp32 remainders, has_remainders) of the resident clip as the engine holds it."""
        hi = np.empty(self.shape, dtype=np.float32)
        lo = np.empty(self.shape, dtype=np.float32)
        flag = C.c_int32(0)
        check(lib().repet_ctx_download_input(self._h, ptr(hi), ptr(lo), C.byref(flag)))
        return hi, lo, bool(flag.value)

    def download_device(self, data_ptr):
        """The result as fp32 interleaved samples into device memory of at least ``prod(self.shape)`` floats."""
        check(lib().repet_ctx_download_device(self._h, C.c_void_p(int(data_ptr))))

    def set_strict_reference(self, on=True):
        """NaN / infinite samples are let through as repet.py lets them (the default since ABI 4); ``on=False``: host uploads
        with such samples are refused (REPET_FLAG_REFUSE_NONFINITE)."""
        check(lib().repet_ctx_set_strict_reference(self._h, 1 if on else 0))

    def stream(self):
        """The context's HIP stream as an integer handle (``torch.cuda.ExternalStream(ctx.stream())`` orders torch's
        sends, receives and adds behind a run without a host wait)."""
        h = C.c_void_p()
        check(lib().repet_ctx_stream(self._h, C.byref(h)))
        return int(h.value or 0)

    def result_view(self):
        """(device pointer, number of fp32 values) of the last run's result inside the context: borrowed, valid until the
        next upload; writes to it are ordered on ``stream()``."""
        ptr_, n = C.c_void_p(), C.c_int64()
        check(lib().repet_ctx_result_view(self._h, C.byref(ptr_), C.byref(n)))
        return int(ptr_.value or 0), int(n.value)

    def input_view(self):
        """(pointer to the resident fp32 samples, pointer to their fp32 remainders or None, number of values)."""
        hi, lo, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        check(lib().repet_ctx_input_view(self._h, C.byref(hi), C.byref(lo), C.byref(n)))
        return int(hi.value or 0), (int(lo.value) if lo.value else None), int(n.value)

    def download_from(self, data_ptr, shape):
        """fp32 values in device memory (e.g. a result received from a peer) widened into a fresh float64 host array through
        the context's pinned ring."""
        out = result_array(shape)
        check(lib().repet_ctx_download_from(self._h, C.c_void_p(int(data_ptr)), int(np.prod(shape)), ptr(out)))
        return out

    def execute_extended_range_async(self, params, first, n_segments):
        check(lib().repet_ctx_execute_extended_range_async(self._h, C.byref(params), int(first), int(n_segments)))

    def set_window(self, number_samples_total, first_sample):
        """The resident samples are ``[first_sample, first_sample + N)`` of a clip of ``number_samples_total`` samples
        (for ``execute_extended_range`` on a rank that holds only its own segments' samples)."""
        check(lib().repet_ctx_set_window(self._h, int(number_samples_total), int(first_sample)))

    def upload_wav(self, audio_file):
        """A WAVE file becomes the resident clip: its raw PCM bytes cross PCIe and are decoded and normalised on the
        device exactly as ``repet.wavread`` would (repet.py:914-931). Returns the sampling frequency."""
        image = np.fromfile(audio_file, dtype=np.uint8)
        info = WavInfo()
        check(lib().repet_ctx_upload_wav(self._h, ptr(image), image.size, C.byref(info)))
        self.shape = (info.n_samples, info.n_channels)
        return info.sampling_frequency

    def write_wav(self, audio_file, which="background", dtype=np.float64, sampling_frequency=None):
        """Write the background (or ``audio - background``) of the last run as the file ``repet.wavwrite`` writes for
        an array of ``dtype`` float64 / float32 (repet.py:934-946), straight from the device result."""
        if sampling_frequency is not None:
            check(lib().repet_ctx_set_sampling_frequency(self._h, int(sampling_frequency)))
        code = {"background": 1, "foreground": 2}[which]
        item = np.dtype(dtype).itemsize
        image = np.empty(58 + int(np.prod(self.shape)) * item, dtype=np.uint8)
        written = C.c_int64()
        check(lib().repet_ctx_result_wav(self._h, code, F64 if item == 8 else F32, ptr(image), image.size, C.byref(written)))
        image[:written.value].tofile(audio_file)

    def _serves(self, algo, params):
        """An armed request was sized for one run: any other run refuses it (and drops it) before the library is called."""
        armed, self._armed = getattr(self, "_armed", None), None
        if armed is not None and armed != (ALGO_IDS[algo] if isinstance(algo, str) else algo, params.window_length,
                                           params.step_length, tuple(self.shape)):
            self.clear_requests()
            raise ValueError("the frames were requested for another algorithm, window or resident clip than this run's")

    def execute(self, algo, params, timing=False):
        self._serves(algo, params)
        t = Timing() if timing else None
        check(lib().repet_ctx_execute(self._h, ALGO_IDS[algo] if isinstance(algo, str) else algo,
                                      C.byref(params), C.byref(t) if timing else None))
        return t.as_dict() if timing else None

    def execute_async(self, algo, params):
        self._serves(algo, params)
        check(lib().repet_ctx_execute_async(self._h, ALGO_IDS[algo] if isinstance(algo, str) else algo, C.byref(params)))

    def synchronize(self):
        check(lib().repet_ctx_synchronize(self._h))

    def timing_series_begin(self, n_steps):
        """Every ``execute_async`` up to ``n_steps`` records its own per-stage events; no host wait between the runs."""
        check(lib().repet_ctx_timing_series_begin(self._h, int(n_steps)))

    def timing_series_end(self):
        """Wait for the stream; mean per-stage device times over the runs since ``timing_series_begin``."""
        t, n = Timing(), C.c_int32()
        check(lib().repet_ctx_timing_series_end(self._h, C.byref(t), C.byref(n)))
        d = t.as_dict()
        d["steps"] = int(n.value)
        return d

    def execute_extended_range(self, params, first, n_segments, timing=False):
        t = Timing() if timing else None
        check(lib().repet_ctx_execute_extended_range(self._h, C.byref(params), int(first), int(n_segments), C.byref(t) if timing else None))
        return t.as_dict() if timing else None

    def download(self):
        out = result_array(self.shape)
        check(lib().repet_ctx_download(self._h, ptr(out)))
        return out

    def foreground(self):
        """audio_signal - background_signal of the last run (float64, computed on the device)."""
        out = np.empty(self.shape, dtype=np.float64)
        check(lib().repet_ctx_download_foreground(self._h, ptr(out)))
        return out

    def spectrogram(self, which, window_length):
        """(F, T) magnitude spectrogram of the channel-mean mixture / background / foreground signal."""
        code = {"mixture": 0, "background": 1, "foreground": 2}[which] if isinstance(which, str) else int(which)
        t = lib().repet_frame_count(self.shape[0], window_length, window_length // 2, 1)
        spec = np.empty((t, window_length // 2 + 1), dtype=np.float32)
        check(lib().repet_ctx_spectrogram(self._h, code, window_length, ptr(spec), t))
        return spec.T.astype(np.float64)

    def last_periods(self, capacity):
        out = np.empty(max(capacity, 1), dtype=np.int32)
        n = C.c_int32()
        check(lib().repet_ctx_last_periods(self._h, ptr(out), capacity, C.byref(n)))
        return out[:n.value].copy()

    def last_median_path(self):
        """'f32', 'rank' or 'bits': the form of sim's median the last run took (see repet_ctx_last_median_path)."""
        v = C.c_int32()
        check(lib().repet_ctx_last_median_path(self._h, C.byref(v)))
        return ("f32", "rank", "bits")[v.value]

    def last_median_codes(self, number_bins):
        """uint32[channels][frames][number_bins] of the last `sim` run on the bit-sliced path (repet_ctx_last_median_codes)."""
        t = self.last_frame_count()
        ch = self.shape[-1]
        out = np.empty((ch, t, number_bins), dtype=np.uint32)
        check(lib().repet_ctx_last_median_codes(self._h, ptr(out), t, number_bins))
        return out

    def last_frame_count(self):
        t = C.c_int64()
        check(lib().repet_ctx_last_frame_count(self._h, C.byref(t)))
        return t.value

    def last_refine_stats(self):
        """Near-tie refinement counters of the last sim/simonline run (see repet_ctx_last_refine_stats)."""
        out = (C.c_int64 * 4)()
        check(lib().repet_ctx_last_refine_stats(self._h, out))
        return {"rows_refined": out[0], "elements_refined": out[1], "decisions_changed": out[2], "flat_rows": out[3]}

    def last_exact_stats(self):
        """Second level of the peak picking (float64 spectra; see repet_ctx_last_exact_stats)."""
        out = (C.c_int64 * 8)()
        check(lib().repet_ctx_last_exact_stats(self._h, out))
        return {"rows_exact": out[0], "elements_exact": out[1], "rows_changed": out[2], "level2_max_diff": out[3] * 1e-12,
                "unit_rows_f64": out[4], "input_has_remainders": bool(out[5]), "rows_fast_path": out[6], "rows_handed_on": out[7]}

    def set_online_start(self, start_frames):
        """``start_frames`` M of this context's ``simonline`` runs (see ``repet.online``): frames M - 1 .. buffer_frames - 2 are
        separated on the buffer as far as it has filled, and ``last_sim_indices`` then has ``T - M + 1`` rows. 0: the reference
        (buffer_frames). Checked against buffer_frames when a run executes (ValueError for a larger value)."""
        check(lib().repet_ctx_set_online_start(self._h, int(start_frames)))

    def last_sim_indices(self, n_rows, number, clip=0):
        """The index lists of the last sim / simonline run. ``clip``: of a batch whose run kept every clip's lists (simonline
        over a batch), that clip's, with ``n_rows`` the rows of one clip; ``clip=0`` also takes the rows of all clips, back to
        back. After a run that worked through the clips one after the other only ``clip=0`` is accepted, and the lists are the
        last clip's, as ever."""
        idx = np.empty((max(n_rows, 1), number), dtype=np.int32)
        cnt = np.empty(max(n_rows, 1), dtype=np.int32)
        check(lib().repet_ctx_last_sim_indices_clip(self._h, int(clip), ptr(idx), ptr(cnt), n_rows, number))
        return idx[:n_rows], cnt[:n_rows]

    @property
    def last_clip_passes(self):
        """How often the last execute enqueued its variant's pipeline: 1 for a single clip and for a batch that went through
        every stage together (``simonline``, ``original`` over equal clips), the number of clips for a variant, or a ragged
        batch, that works through the clips one after the other."""
        v = C.c_int32()
        check(lib().repet_ctx_last_clip_passes(self._h, C.byref(v)))
        return v.value

    def request_frames(self, algo, params, which, out, bands=None, stream=None):
        """Arm a request for the spectra of the NEXT ``execute`` / ``execute_async``, which must be the one of ``algo`` and
        ``params`` on the clip(s) resident now (repet_ctx_request_frames): ``which`` ("mixture", "background", "foreground") of
        every frame into ``out``, a tensor on this context's device -- float32 ``(T, C, F)`` or ``(B, T, C, F)`` with any
        non-overlapping strides, or with ``bands`` (``n_bands + 1`` bin edges) dense float64 ``(..., T, C, n_bands)`` --,
        ``T = result_frame_count(algo, params, N)``. Served behind every pass of that run on the engine's stream,
        which goes behind ``stream`` (default: the device's current one) now; ``stream`` goes behind the last launch when the
        run is enqueued. The request is dropped with that execute, also when it fails; ``clear_requests`` drops it before.
        ValueError for whatever ``repet.separate`` refuses of its ``frames`` keywords, and from a run other than the one named."""
        import torch
        if self.shape is None:
            raise ValueError("no clip uploaded")
        _, edges, _, _ = frames_request(algo if isinstance(algo, str) else {v: k for k, v in ALGO_IDS.items()}.get(algo), params, which,
                                        bands, out, self.shape, torch.device("cuda", self._device))
        if stream is None:
            stream = torch.cuda.current_stream(out.device)
        strides = tuple(int(st) for st in out.stride())
        strides = (0,) * (4 - len(strides)) + strides
        check(lib().repet_ctx_request_frames(self._h, WHICH_CODES[which], None if edges is None else ptr(edges),
                                             0 if edges is None else edges.size - 1, C.c_void_p(out.data_ptr() or None),
                                             (C.c_int64 * 4)(*strides), _stream_handle(stream)))
        self._armed = (ALGO_IDS[algo] if isinstance(algo, str) else algo, params.window_length, params.step_length, tuple(self.shape))
        return out

    def clear_requests(self):
        """Drop an armed request (host only)."""
        self._armed = None
        check(lib().repet_ctx_clear_requests(self._h))

    @property
    def last_spectrum_form(self):
        """How the last pass of the last run left its masked spectrum: 0 masked in place, 1 the spectrum and a mask plane,
        2 the spectrum, the repeating-segment model and the period (the inverse STFT forms the mask as it fetches)."""
        v = C.c_int32()
        check(lib().repet_ctx_last_spectrum_form(self._h, C.byref(v)))
        return v.value


_default_ctx = {}


def default_context(device=0):
    ctx = _default_ctx.get(device)
    if ctx is None:
        ctx = _default_ctx[device] = Context(device)
    return ctx


def silent_frames_flag(silent_frames, algo="simonline"):
    """The bit of ``Params.flags`` for ``silent_frames`` ("reference": 0, "zero": FLAG_SILENT_FRAMES_ZERO). ValueError for any
    other value, and for a rule other than the reference's with a variant other than simonline: nothing has run by then."""
    if not isinstance(silent_frames, str):
        # (in ``repet.separate`` the keyword sits in front of ``background_band_gains``: a caller who passed the band gains as
        # the ninth positional argument lands here)
        raise ValueError('silent_frames is "reference" or "zero", not a %s: pass background_band_gains and band_edges of '
                         'repet.separate by keyword (silent_frames was added in front of them)' % type(silent_frames).__name__)
    if silent_frames not in SILENT_FRAMES:
        raise ValueError(f'silent_frames is "reference" or "zero", not {silent_frames!r}')
    flag = SILENT_FRAMES[silent_frames]
    if flag and algo != "simonline":
        raise ValueError(f'silent_frames={silent_frames!r} goes with algo="simonline" and the live handles only, not {algo!r}')
    return flag


def _silent_frames_of(params):
    return "zero" if params.flags & FLAG_SILENT_FRAMES_ZERO else "reference"


def start_frames_for(params, sampling_frequency, start_length):
    """``start_length`` in seconds as frames, derived as buffer_frames is and clamped to [1, buffer_frames]; None stays None (the
    handle is then opened as it always was)."""
    if start_length is None:
        return None
    frames = int(round(start_length * sampling_frequency / params.step_length))
    return min(int(params.buffer_frames), max(1, frames))


def _set_start_frames(owner, start_frames):
    """start_frames of a handle that was just opened (None: left alone); a refusal closes the handle before it is raised."""
    if start_frames is None:
        return
    try:
        check(lib().repet_online_set_start_frames(owner._h, int(start_frames)))
    except Exception:
        owner.close()
        raise


def _start_frames(handle):
    out = C.c_int32()
    check(lib().repet_online_start_frames(handle, C.byref(out)))
    return out.value


def _select_output(handle, codes, second=None, dtype=F64, strides=None):
    """What the next emitting call of a live handle delivers: codes[0] in its own destination and, for a pair, codes[1] in
    ``second`` (a pointer) by the same launch."""
    check(lib().repet_online_set_output(handle, codes[0]))
    if len(codes) == 2:
        check(lib().repet_online_also_emit(handle, codes[1], second, dtype, strides))


class StreamState:
    """The state of one live stream as a value (``export_stream`` of a streaming handle): ``header``, a small ``bytes`` the
    host knows without touching the device, and ``payload``, a ``numpy.uint8`` array or a ``torch.uint8`` tensor on a ROCm
    device. ``import_stream`` of any handle opened with the same parameters takes it; ``to_bytes()`` / ``from_bytes(b)``
    serve persistence (they may wait for the device). The header's fields are attributes (``window_length``, ``age_frames``,
    ``length_samples``, ``payload_bytes``, ...), listed in ``StreamState.FIELDS``."""

    MAGIC = 0x53504552                 # b"REPS", little-endian
    VERSION = 1
    _FORMAT = "<II10id5q"
    HEADER_BYTES = struct.calcsize(_FORMAT)
    FIELDS = ("magic", "version", "window_length", "step_length", "buffer_frames", "number_channels", "number_bins",
              "cutoff_bins", "similarity_distance_frames", "similarity_number", "params_buffer_frames", "flags",
              "similarity_threshold", "age_frames", "length_samples", "history_rows", "pending_samples", "payload_bytes")

    def __init__(self, header, payload):
        self.header = bytes(header)
        self.fields = self.unpack_header(self.header)
        self.payload = payload

    def __getattr__(self, name):
        fields = self.__dict__.get("fields")
        if fields is not None and name in fields:
            return fields[name]
        raise AttributeError(name)

    @classmethod
    def pack_header(cls, fields):
        """The header bytes of a dict with every name of ``FIELDS``."""
        return struct.pack(cls._FORMAT, *(fields[name] for name in cls.FIELDS))

    @classmethod
    def unpack_header(cls, header):
        """The fields of a header as a dict. ValueError for a wrong size, an unknown magic word or an unknown version."""
        header = bytes(header)
        if len(header) != cls.HEADER_BYTES:
            raise ValueError(f"a stream state header is {cls.HEADER_BYTES} bytes, not {len(header)}")
        fields = dict(zip(cls.FIELDS, struct.unpack(cls._FORMAT, header)))
        if fields["magic"] != cls.MAGIC:
            raise ValueError("not a stream state (unknown magic word)")
        if fields["version"] != cls.VERSION:
            raise ValueError(f"unknown version {fields['version']} of the stream state")
        if fields["payload_bytes"] < 0:
            raise ValueError("the stream state has a negative payload size")
        return fields

    def payload_array(self):
        """The payload as a host ``numpy.uint8`` array (a device payload is copied: this waits)."""
        p = self.payload
        if is_tensor(p):
            p = p.detach().cpu().numpy()
        return np.ascontiguousarray(p)

    def to_bytes(self):
        """Header and payload as one ``bytes`` value."""
        p = self.payload_array()
        if p.dtype != np.uint8 or p.size != self.fields["payload_bytes"]:
            raise ValueError("the payload is not the uint8 array the header describes")
        return self.header + p.tobytes()

    @classmethod
    def from_bytes(cls, b):
        """The state ``to_bytes`` wrote. ValueError for a truncated or padded value, an unknown magic word or version."""
        b = bytes(b)
        fields = cls.unpack_header(b[:cls.HEADER_BYTES])
        if len(b) != cls.HEADER_BYTES + fields["payload_bytes"]:
            raise ValueError(f"the stream state has {len(b) - cls.HEADER_BYTES} payload bytes, its header says {fields['payload_bytes']}")
        return cls(b[:cls.HEADER_BYTES], np.frombuffer(b, dtype=np.uint8, offset=cls.HEADER_BYTES).copy())


def _state_sizes(handle):
    hb, pb = C.c_int64(), C.c_int64()
    check(lib().repet_online_stream_state_size(handle, C.byref(hb), C.byref(pb)))
    if hb.value != StreamState.HEADER_BYTES:
        raise RuntimeError("librepet_hip.so writes another stream state header than this binding reads")
    return hb.value, pb.value


def _export_state(handle, slot, device=None):
    """export_stream of ``slot``: a host payload (device None), or a tensor on cuda:``device`` behind its current stream."""
    hb, pb = _state_sizes(handle)
    header = C.create_string_buffer(hb)
    payload, = read_back(
        device, device is not None, [pb], [np.uint8],
        lambda p: lib().repet_online_export_stream(handle, slot, header, ptr(p)),
        lambda p, stream: lib().repet_online_export_stream_device(handle, slot, header, C.c_void_p(p.data_ptr()), stream))
    return StreamState(header.raw, payload)


def _import_state(handle, slot, state, device):
    """import_stream of ``state`` into ``slot`` of a handle on cuda:``device``; returns the header's fields. Everything the
    Python layer can refuse (header, payload dtype and size) is refused here, the rest by the library, before any launch."""
    if not isinstance(state, StreamState):
        raise ValueError("import_stream takes the StreamState that export_stream returned")
    fields = StreamState.unpack_header(state.header)
    _, pb = _state_sizes(handle)
    payload = state.payload
    if is_tensor(payload):
        if str(payload.dtype) != "torch.uint8":
            raise ValueError(f"the payload is a uint8 tensor, not {payload.dtype}")
        size = payload.numel()
    else:
        payload = np.asarray(payload)
        if payload.dtype != np.uint8:
            raise ValueError(f"the payload is a uint8 array, not {payload.dtype}")
        size = payload.size
    if size != fields["payload_bytes"] or size != pb:
        raise ValueError(f"the payload has {size} bytes, the header says {fields['payload_bytes']} and the handle takes {pb}")
    if is_device_tensor(payload):
        import torch
        dev = torch.device("cuda", device)
        # a payload on another GPU: a peer (or staged) copy into the handle's device, ordered by torch on the current streams
        payload = payload.reshape(-1).to(dev, non_blocking=True).contiguous()
        stream = torch.cuda.current_stream(dev)
        check(lib().repet_online_import_stream_device(handle, slot, state.header, C.c_void_p(payload.data_ptr()),
                                                      _stream_handle(stream)))
        payload.record_stream(stream)
    else:
        if is_tensor(payload):
            payload = payload.numpy()
        payload = np.ascontiguousarray(payload).reshape(-1)
        check(lib().repet_online_import_stream(handle, slot, state.header, ptr(payload)))
    return fields


def _last_levels(handle, device, shape, out, on_device):
    """``last_levels`` of a live handle whose record has ``shape``: see ``OnlineStreams.last_levels``."""
    n = C.c_int64()
    return read_back(
        device, out is not None or on_device, [shape], [np.float64],
        lambda r: lib().repet_online_last_levels(handle, ptr(r), r.size, C.byref(n)),
        lambda t, stream: lib().repet_online_last_levels_device(handle, C.c_void_p(t.data_ptr()), stream),
        None if out is None else (levels_out(out, shape, device),))[0]


def _frame_range(handle):
    first, count = C.c_int64(), C.c_int64()
    check(lib().repet_online_last_frame_range(handle, C.byref(first), C.byref(count)))
    return first.value, count.value


def band_edge_array(bands):
    """``bands=`` of ``last_frames`` as the int32 array the library takes: ``n_bands + 1`` integers. ValueError for anything
    else; their order and range are the library's to check."""
    try:
        edges = np.asarray(bands)
        if edges.ndim != 1 or edges.size < 2 or edges.dtype.kind not in "iu":
            raise ValueError
        wide = edges.astype(np.int64)
        if (np.abs(wide) > 2 ** 31 - 1).any():
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("bands is a sequence of n_bands + 1 integer bin edges") from None
    return np.ascontiguousarray(wide.astype(np.int32))


MAX_BANDS = 128                # REPET_MAX_BANDS
FRAME_SIGNALS = ("mixture", "background", "foreground")


def result_frame_count(algo, params, number_samples):
    """Frames of the spectra a tensor call of ``algo`` hands out for clips of ``number_samples`` samples
    (repet_result_frame_count): host arithmetic, no device. ValueError for "extended" (no single frame grid)."""
    if algo not in ALGO_IDS:
        raise ValueError(f"unknown algorithm {algo!r}")
    t = lib().repet_result_frame_count(ALGO_IDS[algo], params, int(number_samples))
    if t < 0:
        raise ValueError(lib().repet_last_error().decode(errors="replace"))
    return int(t)


def frames_request(algo, params, frames, frame_bands, frames_out, shape, device):
    """``frames=`` / ``frame_bands=`` / ``frames_out=`` of ``repet.separate`` for an input of ``shape`` on ``device``, checked on
    the host alone: None when nothing is asked, else ``(frames, edges or None, frames_out or None, result shape)``. ValueError for
    everything the call refuses."""
    if frames is None:
        if frame_bands is not None or frames_out is not None:
            raise ValueError("frame_bands and frames_out go with frames")
        return None
    if not isinstance(frames, str) or frames not in FRAME_SIGNALS:
        raise ValueError(f'frames is "mixture", "background" or "foreground", not {frames!r}')
    if algo == "extended":
        raise ValueError('frames: the segments of "extended" overlap and cross-fade, there is no single spectrogram to hand out')
    bins = params.window_length // 2 + 1
    edges = None
    if frame_bands is not None:
        edges = band_edge_array(frame_bands)
        if edges.size - 1 > MAX_BANDS:
            raise ValueError(f"frame_bands: at most {MAX_BANDS} bands")
        if edges[0] < 0 or edges[-1] > bins or (np.diff(edges.astype(np.int64)) < 0).any():
            raise ValueError(f"frame_bands: band edges are ascending bins in [0, {bins}]")
    shape = tuple(int(d) for d in shape)
    if len(shape) not in (2, 3):
        raise ValueError("audio_signal must be (number_samples, number_channels) or a batch of such clips")
    count = result_frame_count(algo, params, shape[-2])
    result_shape = shape[:-2] + (count, shape[-1], bins if edges is None else edges.size - 1)
    if frames_out is not None:
        name = "torch.float32" if edges is None else "torch.float64"
        if not is_tensor(frames_out):
            raise ValueError(f"frames_out must be a {name} tensor on the input's device")
        if frames_out.device != device:
            raise ValueError(f"frames_out must be a tensor on {device}")
        if str(frames_out.dtype) != name:
            raise ValueError(f"the frames are {name}, frames_out is {frames_out.dtype}")
        if tuple(frames_out.shape) != result_shape:
            raise ValueError(f"frames_out has shape {tuple(frames_out.shape)}, the frames {result_shape}")
        if edges is not None and not frames_out.is_contiguous():
            raise ValueError("frames_out must be dense (contiguous) for band energies")
    return frames, edges, frames_out, result_shape


def _ask_frames(handle, code, edges):
    """An empty result (a push that completed no frame): the library still refuses a bad ``which`` or ``bands`` and a stale
    record, and launches nothing."""
    n = C.c_int64()
    if edges is None:
        return lib().repet_online_last_frames(handle, code, None, 0, C.byref(n))
    return lib().repet_online_last_band_energies(handle, code, ptr(edges), edges.size - 1, None, 0, C.byref(n))


def _last_frames(handle, device, lead, bins, which, bands, out, on_device):
    """``last_frames`` of a live handle whose result has the leading dimensions ``lead`` -- (S,) or () -- before (T, C, F) or
    (T, C, n_bands): see ``OnlineStreams.last_frames``. ``lead`` plus the channel count come as ``(lead, C)``."""
    lead, channels = lead
    codes = which_codes(which)
    if len(codes) != 1:
        raise ValueError("last_frames returns one signal")
    edges = None if bands is None else band_edge_array(bands)
    _, count = _frame_range(handle)
    last = bins if edges is None else edges.size - 1
    shape = tuple(lead) + (count, channels, last)
    np_dtype = np.float32 if edges is None else np.float64
    if out is not None and not is_tensor(out):
        if not isinstance(out, np.ndarray) or out.dtype != np_dtype or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous {np.dtype(np_dtype).name} array of shape {shape}, or a tensor on the device")
    on_device = is_tensor(out) or (out is None and on_device)
    if on_device and out is not None:
        import torch
        device_out(out, shape, device, torch.float32 if edges is None else torch.float64, "the result is {want}, out is {got}",
                   dense=edges is not None)
    code, n = codes[0], C.c_int64()

    def host_call(r):
        if not r.size:
            return _ask_frames(handle, code, edges)
        if edges is None:
            return lib().repet_online_last_frames(handle, code, ptr(r), r.size, C.byref(n))
        return lib().repet_online_last_band_energies(handle, code, ptr(edges), edges.size - 1, ptr(r), r.size, C.byref(n))

    def device_call(t, stream):
        if not t.numel():
            return _ask_frames(handle, code, edges)
        if edges is None:
            strides = (0,) * (4 - t.dim()) + tuple(int(st) for st in t.stride())
            return lib().repet_online_last_frames_device(handle, code, C.c_void_p(t.data_ptr()), (C.c_int64 * 4)(*strides), stream)
        return lib().repet_online_last_band_energies_device(handle, code, ptr(edges), edges.size - 1, C.c_void_p(t.data_ptr()), stream)

    return read_back(device, on_device, [shape], [np_dtype], host_call, device_call, None if out is None else (out,))[0]


def _match_capacity(handle):
    k = C.c_int32()
    check(lib().repet_online_match_capacity(handle, C.byref(k)))
    return k.value


def match_outs(out, shapes, device):
    """``out=`` of ``last_matches`` against the three shapes of the result: a triple of dense tensors on cuda:``device``, int32,
    int32 and float32. ValueError otherwise, before anything runs."""
    import torch
    try:
        outs = tuple(out)
    except TypeError:
        outs = ()
    if len(outs) != 3:
        raise ValueError("out is a triple of tensors (count, age, similarity)")
    for name, t, shape, dtype in zip(Matches._fields, outs, shapes, (torch.int32, torch.int32, torch.float32)):
        device_out(t, shape, device, dtype, f"out: {name} is {{want}}, not {{got}}", dense=True, name=f"out: {name}")
    return outs


def _last_matches(handle, device, lead, out, on_device):
    """``last_matches`` of a live handle whose result has the leading dimensions ``lead`` -- (S,) or () -- before (T,) and
    (T, K): see ``OnlineStreams.last_matches``."""
    _, count = _frame_range(handle)
    k = _match_capacity(handle)
    shapes = (tuple(lead) + (count,), tuple(lead) + (count, k), tuple(lead) + (count, k))
    n = C.c_int64()
    # (an empty record: nothing is asked of the library)
    return Matches(*read_back(
        device, out is not None or on_device, shapes, (np.int32, np.int32, np.float32),
        lambda c, a, s: c.size and lib().repet_online_last_matches(handle, ptr(c), ptr(a), ptr(s), c.size, C.byref(n)),
        lambda c, a, s, stream: c.numel() and lib().repet_online_last_matches_device(
            handle, *(C.c_void_p(t.data_ptr()) for t in (c, a, s)), stream),
        None if out is None else match_outs(out, shapes, device)))


class OnlineSeparator:
    """Streaming online REPET-SIM: ``push(chunk)`` returns the background samples that became final,
    ``finish()`` the rest; the concatenation equals ``repet.simonline`` of the whole signal. ``which`` ("background",
    "foreground", "mixture", "both") selects the signal of those samples, see ``repet.online``. ``export_stream()`` returns
    the stream's state as a ``StreamState`` and ``import_stream(state)`` loads one, see ``repet.online_streams``."""

    def __init__(self, params, n_channels, device=0, start_frames=None):
        self._h = C.c_void_p()
        self._channels = int(n_channels)
        self._window = int(params.window_length)
        self._bins = self._window // 2 + 1
        self._device = int(device)
        if lib().repet_device_count() < 1:
            raise RuntimeError("no HIP device visible: the REPET engine has no CPU fallback")
        check(lib().repet_online_open(int(device), self._channels, C.byref(params), C.byref(self._h)))
        self._silent_frames = _silent_frames_of(params)
        _set_start_frames(self, start_frames)

    @property
    def silent_frames(self):
        """What the stream makes of frames of digital silence (``silent_frames`` of ``repet.online``): "reference" or "zero"."""
        return self._silent_frames

    @property
    def start_frames(self):
        """The stream's frame count from which it is separated (``start_length`` of ``repet.online``; buffer_frames: the reference)."""
        return _start_frames(self._h)

    def push(self, audio_chunk, which="background"):
        codes = which_codes(which)
        n, c = np.shape(audio_chunk)
        if c != self._channels:
            raise ValueError("chunk has %d channels, the stream %d" % (c, self._channels))
        a, code = as_input(audio_chunk)
        cap = n + self._window
        outs = [np.empty((cap, c), dtype=np.float64) for _ in codes]
        written = C.c_int64()
        _select_output(self._h, codes, ptr(outs[-1]))
        check(lib().repet_online_push(self._h, ptr(a), code, n, ptr(outs[0]), cap, C.byref(written)))
        outs = [o[:written.value].copy() for o in outs]
        return outs[0] if len(outs) == 1 else tuple(outs)

    def finish(self, which="background"):
        codes = which_codes(which)
        cap = 4 * self._window + 16
        while True:
            outs = [np.empty((cap, self._channels), dtype=np.float64) for _ in codes]
            written = C.c_int64()
            _select_output(self._h, codes, ptr(outs[-1]))
            rc = lib().repet_online_finish(self._h, ptr(outs[0]), cap, C.byref(written))
            if rc == ERR_BAD_ARG and b"capacity" in lib().repet_last_error():
                cap *= 4
                continue
            check(rc)
            outs = [o[:written.value].copy() for o in outs]
            return outs[0] if len(outs) == 1 else tuple(outs)

    def last_levels(self):
        """The levels (``repet.LEVELS``) of what the last ``push`` / ``finish`` emitted: a float64 array ``(C, 8)``, reduced on
        the device; see ``repet.online_streams``. ValueError once another call has followed."""
        return _last_levels(self._h, self._device, (self._channels, LEVEL_FIELDS), None, False)

    @property
    def last_frame_range(self):
        """``(first, count)``: the frames the last ``push`` / ``finish`` completed; frame ``k`` begins at pushed sample ``k *
        step_length``. ValueError once another call has followed; see ``repet.online_streams``."""
        return _frame_range(self._h)

    def last_frames(self, which="foreground", bands=None, out=None):
        """The spectra of the frames the last ``push`` / ``finish`` completed: float32 ``(T, C, F)`` magnitudes of ``which``
        ("background", "foreground", "mixture"), or with ``bands`` (``n_bands + 1`` ascending bin edges) their float64 band
        energies ``(T, C, n_bands)``. A NumPy array, or ``out`` (an array of that shape, or a tensor on the device: no host
        wait). See ``repet.online_streams``. ValueError once another call has followed."""
        return _last_frames(self._h, self._device, ((), self._channels), self._bins, which, bands, out, False)

    @property
    def match_capacity(self):
        """``K``: the most similar frames a frame can have, the last axis of ``last_matches``; see ``repet.online_streams``."""
        return _match_capacity(self._h)

    def last_matches(self, out=None):
        """The similar frames the frames of the last ``push`` / ``finish`` matched: ``repet.Matches(count, age, similarity)``,
        int32 ``(T,)``, int32 ``(T, K)`` and float32 ``(T, K)`` NumPy arrays, or ``out`` (a triple of dense tensors on the device:
        no host wait). See ``repet.online_streams``. ValueError once another call has followed."""
        return _last_matches(self._h, self._device, (), out, False)

    def set_background_gain(self, gain):
        """Keep ``gain`` (in [0, 1]) of the background in the foreground from the next emission on, see ``repet.online``."""
        g = background_gains(gain)
        check(lib().repet_online_set_background_gain(self._h, None, 0, ptr(g)))

    def background_gain(self):
        """The background gain last set (0: the plain foreground)."""
        out = C.c_float()
        check(lib().repet_online_background_gain(self._h, 0, C.byref(out)))
        return out.value

    def set_background_band_gains(self, gains, edges=None):
        """Keep a share of the background in the foreground band by band: ``gains`` in [0, 1], one per band of ``edges``
        (``n_bands + 1`` ascending bin edges) or, without ``edges``, one per bin. See ``repet.online_streams``."""
        _set_band_gains(lambda: self._h, None, 0, gains, edges, self._bins, None)

    def background_band_gains(self):
        """The per-bin gains last set, float32 ``(F,)`` (zeros: the plain foreground). A host copy: no device work."""
        return _get_band_gains(self._h, 0, self._bins)

    def clear_background_band_gains(self):
        """Back to the plain foreground: every bin's gain 0."""
        _set_band_gains(lambda: self._h, None, 0, np.zeros(self._bins, dtype=np.float32), None, self._bins, None)

    def export_stream(self):
        """A snapshot of the stream's state (a ``StreamState`` with a host payload); the stream goes on untouched. ValueError
        unless the samples pushed so far are a multiple of the hop."""
        return _export_state(self._h, 0)

    def import_stream(self, state):
        """Drop what the separator has heard and go on as the stream ``state`` was exported from (any handle opened with
        the same parameters). ValueError, with nothing changed, for a state of other parameters or off the hop grid."""
        _import_state(self._h, 0, state, self._device)

    def close(self):
        if self._h:
            lib().repet_online_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class OnlineStreams:
    """S live streams of one sampling frequency and channel count in one streaming handle (``repet.online_streams``), pushed
    in lockstep: every ``push`` brings ``(S, n, C)`` samples, and each stream's concatenated output equals ``repet.simonline``
    of its concatenated input. Host chunks (NumPy arrays, lists, CPU tensors) return float64 ``(S, n_emit, C)`` arrays; ROCm
    tensors return a float64 tensor on their device (or fill ``out``), ordered on its current stream with no host wait.

    The S streams are S *slots*: ``restart(slots)`` begins a new stream in each named slot at the handle's current sample (a
    multiple of the hop), ``finish_stream(slot)`` ends one and returns its tail, ``release(slots)`` drops them without output.
    An idle slot ignores what the lockstep chunks carry for it and emits zeros. A slot's output from its restart on, followed
    by its ``finish_stream`` (or ``finish``) tail, equals ``repet.simonline`` of the samples pushed into it in between.

    ``which`` of ``push`` / ``finish`` / ``finish_stream`` selects the signal of the emitted samples: "background" (default),
    "foreground" (input - background), "mixture" (the input, aligned with the emission) or "both": the pair (background,
    foreground) from one pass, with ``out=`` a pair of tensors. ``last_emission(which)`` returns another signal of the samples
    the last of these calls emitted.

    ``hold(slots)`` lets live slots sit out the pushes that follow and ``resume(slots)`` lets them go on: a held slot ignores
    its share of the chunks, emits zeros and keeps all it holds, so its stream goes on bit for bit as if those pushes had not
    been made (``repet.online_streams``).

    ``enable_feed(capacity_samples)`` gives every slot an inbox: ``feed(slots, chunk, counts=None)`` then takes packets of any
    size per slot and ``tick(hops=1)`` is the push, made of the slots that have ``hops`` hops queued while the others sit it
    out as held slots do (``queued``, ``pad_feed``, ``clear_feed``, ``last_consumed``; see ``repet.online_streams``)."""

    def __init__(self, params, n_channels, n_streams, device=0, max_push_samples=0, start_frames=None):
        self._h = C.c_void_p()
        self._channels = int(n_channels)
        self._streams = int(n_streams)
        self._bins = int(params.window_length) // 2 + 1
        self._device = int(device)
        self._last_on_device = False
        if self._streams < 1 or self._channels < 1:
            raise ValueError("at least one stream and one channel")
        if lib().repet_device_count() < 1:
            raise RuntimeError("no HIP device visible: the REPET engine has no CPU fallback")
        check(lib().repet_online_open_streams(self._device, self._streams, self._channels, C.byref(params),
                                              int(max_push_samples or 0), C.byref(self._h)))
        self._silent_frames = _silent_frames_of(params)
        _set_start_frames(self, start_frames)
        self._pushed = 0                              # samples per slot pushed so far
        self._emitted_shape = (self._streams, 0, self._channels)
        self._tail_emitted = False                    # the last emitting call was a finish_stream: one slot's record
        self._begun = [0] * self._streams             # handle sample at which each slot's stream began (None: idle)
        self._held = set()                            # slots that sit out the pushes: their beginnings move along with them
        self._hop = int(params.step_length)
        self._feed_cap = 0                            # samples per channel of every slot's inbox (enable_feed)
        self._feed_on_device = False                  # the last feed was a device tensor: ticks return tensors
        self._consumed = np.zeros(self._streams, dtype=bool)

    @property
    def shape(self):
        """(number_streams, number_channels)"""
        return self._streams, self._channels

    @property
    def silent_frames(self):
        """What every slot makes of frames of digital silence (``silent_frames`` of ``repet.online_streams``): "reference" or
        "zero". The handle's, for every slot and every restart; ``import_stream`` refuses a state exported under the other rule."""
        return self._silent_frames

    @property
    def start_frames(self):
        """Frames of its own after which every slot's stream is separated (``start_length`` of ``repet.online_streams``;
        buffer_frames: the reference). The handle's, for every slot and every restart."""
        return _start_frames(self._handle())

    def _handle(self):
        if not self._h:
            raise ValueError("the stream handle is closed")
        return self._h

    def emit_count(self, number_samples, finishing=False):
        """Samples per stream the next push of ``number_samples`` (or the finish) will return."""
        n = C.c_int64()
        check(lib().repet_online_emit_count(self._handle(), int(number_samples), int(bool(finishing)), C.byref(n)))
        return n.value

    def _check_shape(self, shape):
        if len(shape) != 3:
            raise ValueError("a chunk is (number_streams, number_samples, number_channels)")
        if shape[0] != self._streams:
            raise ValueError(f"chunk has {shape[0]} streams, the handle {self._streams}")
        if shape[2] != self._channels:
            raise ValueError(f"chunk has {shape[2]} channels, the streams {self._channels}")

    def _device_outs(self, out, n_emit, codes, shape=None, dtype=None):
        """The destination tensor(s) of a device call: (tensors, dtype code, list of strides); a pair for "both". Fresh ones
        are of ``dtype`` (None: float64), which an ``out`` given beside it must have."""
        outs = [out] if len(codes) == 1 else list(out_pair(out))
        dtype = emit_dtype(dtype, outs)
        checked = [self._device_out(o, n_emit, shape, dtype) for o in outs]
        if len({c[1] for c in checked}) != 1:
            raise ValueError("the two tensors of out have one dtype")
        return [c[0] for c in checked], checked[0][1], [c[2] for c in checked]

    def _device_out(self, out, n_emit, shape=None, dtype=None):
        import torch
        shape = shape or (self._streams, n_emit, self._channels)
        if out is None:
            out = torch.empty(shape, dtype=dtype or torch.float64, device=torch.device("cuda", self._device))
        else:
            device_out(out, shape, self._device)
        return out, emit_tensor_code(out), tuple(int(st) for st in out.stride())

    def _emit(self, codes, n_emit, on_device, out, dtype, host_call, device_call, shape=None):
        """The results of an emitting call for ``codes`` -- float64 host arrays, or tensors on the device (``out``, or fresh ones
        of ``dtype``) -- with the second output armed and the C call made: ``host_call(pointer, n_emit, written)`` or
        ``device_call(pointer, dtype code, strides, stream handle, written)``, each for the first result. Returns
        ``(results, stream)``, the torch stream the device call was ordered on (None: host)."""
        written = C.c_int64()
        if not on_device:
            results = [np.empty(shape or (self._streams, n_emit, self._channels), dtype=np.float64) for _ in codes]
            _select_output(self._handle(), codes, ptr(results[-1]))
            check(host_call(ptr(results[0]), n_emit, C.byref(written)))
            return results, None
        import torch
        results, code, strides = self._device_outs(out, n_emit, codes, shape, dtype)
        stream = torch.cuda.current_stream(results[0].device)
        lead = (0,) * (3 - len(strides[-1]))          # (a finish_stream tail is (n, C): no stream axis)
        _select_output(self._handle(), codes, C.c_void_p(results[-1].data_ptr() or None), code, _strides(lead + strides[-1]))
        check(device_call(C.c_void_p(results[0].data_ptr() or None), code, strides[0], _stream_handle(stream), C.byref(written)))
        return results, stream

    def push(self, chunk, out=None, which="background", dtype=None):
        """Feed ``(S, n, C)`` more samples; returns the ``(S, n_emit, C)`` samples that became final: their background, or
        the signal ``which`` names (a pair of arrays / tensors for "both"). Device chunks: ``out`` (float64, float32, int16,
        float16 or bfloat16) is filled, or a fresh tensor of ``dtype`` (None: float64) returned; see ``repet.online_streams``."""
        codes = which_codes(which)
        on_device = is_device_tensor(chunk)
        if on_device:
            if chunk.device.index != self._device:
                raise ValueError(f"tensor is on {chunk.device}, the streams on device {self._device}")
            if chunk.dim() != 3:
                raise ValueError("a chunk is (number_streams, number_samples, number_channels)")
            self._check_shape(tuple(chunk.shape))
            x, code, shape, strides = tensor_layout(chunk, batched=True)
            source = C.c_void_p(x.data_ptr() or None)
        else:
            if out is not None:
                raise ValueError("out is for device chunks (a host chunk returns a new array)")
            if dtype is not None:
                raise ValueError("dtype is for device chunks (a host chunk returns a float64 array)")
            if is_tensor(chunk):
                chunk = chunk.numpy()
            x, code = as_input(chunk)
            self._check_shape(x.shape)
            shape, source = x.shape, ptr(x)
        n = shape[1]
        h = self._handle()
        results, stream = self._emit(
            codes, self.emit_count(n), on_device, out, dtype,
            lambda dst, cap, written: lib().repet_online_push_streams(h, source, code, n, dst, cap, written),
            lambda dst, dst_code, dst_strides, stream, written: lib().repet_online_push_device(
                h, source, code, n, _strides(strides), stream, dst, dst_code, _strides(dst_strides), stream, written))
        if on_device:
            # the current stream waits for the push (an event behind the egress, which is behind the ingest): with the chunk
            # recorded on it, the caching allocator hands its block out again only once the ingest has read it
            x.record_stream(stream)
        self._count_push(n)
        self._last_on_device = on_device
        self._emitted_shape = tuple(results[0].shape)
        self._tail_emitted = False
        return results[0] if len(results) == 1 else tuple(results)

    def _count_push(self, n):
        self._pushed += n
        for s in self._held:                          # time does not pass for a held slot
            self._begun[s] += n

    def last_emission(self, which="foreground", out=None, dtype=None):
        """Another signal ("background", "foreground", "mixture") of exactly the samples the last ``push`` / ``finish`` /
        ``finish_stream`` emitted: a float64 array, or a tensor on the device (``out``, or a fresh one of ``dtype``, None:
        float64) when ``out`` is given or the last push was a device chunk. ValueError once a push, finish, restart or release
        has followed, and for ``dtype`` where the result is a host array."""
        codes = which_codes(which)
        if len(codes) != 1:
            raise ValueError("last_emission returns one signal")
        self._check_dtype(dtype, out)
        n = C.c_int64()
        # (a call without a destination only asks: its refusal tells a stale emission from one that needs room)
        rc = lib().repet_online_last_emission(self._handle(), codes[0], None, 1 << 62, C.byref(n))
        if rc != ERR_BAD_ARG or b"capacity" not in lib().repet_last_error():
            check(rc)
        shape, h = self._emitted_shape, self._handle()
        on_device = out is not None or self._last_on_device
        outs, out_code, strides = self._device_outs(out, shape[1], codes, shape, dtype) if on_device else (None, F64, None)
        return read_back(
            self._device, on_device, [shape], [np.float64],
            lambda r: lib().repet_online_last_emission(h, codes[0], ptr(r), shape[1], C.byref(n)),
            lambda t, stream: lib().repet_online_last_emission_device(
                h, codes[0], C.c_void_p(t.data_ptr() or None), out_code, _strides(strides[0]), stream, C.byref(n)),
            outs)[0]

    def last_levels(self, out=None):
        """The levels (``repet.LEVELS``, eight float64 values per stream and channel) of exactly the samples the last ``push`` /
        ``finish`` emitted, ``(S, C, 8)``, or of the tail the last ``finish_stream`` returned, ``(C, 8)``: a NumPy array, or a
        tensor on the device (``out``, a dense float64 tensor of that shape, or a fresh one) when ``out`` is given or the last
        push was a device chunk -- then with no host wait. Reduced on the device on demand; see ``repet.online_streams``.
        ValueError for a wrong ``out`` (before anything runs) and once a push, finish, restart or release has followed."""
        shape = (self._channels, LEVEL_FIELDS) if self._tail_emitted else (self._streams, self._channels, LEVEL_FIELDS)
        return _last_levels(self._handle(), self._device, shape, out, self._last_on_device)

    @property
    def last_frame_range(self):
        """``(first, count)``: the frames the last ``push`` / ``finish`` completed, handle frames ``[first, first + count)``;
        frame ``k`` begins at pushed sample ``k * step_length``. From the host's record, no device work. ValueError once a
        push, finish, finish_stream, restart, release, import, hold or resume has followed."""
        return _frame_range(self._handle())

    def last_frames(self, which="foreground", bands=None, out=None):
        """The spectra of the ``T`` frames the last ``push`` / ``finish`` completed (``last_frame_range``): float32 ``(S, T, C,
        F)`` magnitudes of ``which`` ("background", "foreground", "mixture"), ``F = window_length / 2 + 1``; with ``bands``
        (a sequence of ``n_bands + 1`` ascending bin edges in [0, F], at most 128 bands, see ``repet.band_edges``) the float64
        sums of their squares per band, ``(S, T, C, n_bands)``. A NumPy array (``out``: a C-contiguous array of that shape and
        dtype), or a tensor on the handle's device -- ``out``, with any non-overlapping strides for the frames and dense for
        the bands, or a fresh one -- when ``out`` is a tensor or the last push was a device chunk: then with no host wait.
        One launch on demand; see ``repet.online_streams``. ValueError for a wrong ``which``, ``bands`` or ``out`` (before
        anything runs) and once a push, finish, finish_stream, restart, release, import, hold or resume has followed."""
        return _last_frames(self._handle(), self._device, ((self._streams,), self._channels), self._bins, which, bands, out,
                            self._last_on_device)

    @property
    def match_capacity(self):
        """``K = min(similarity_number, ceil(buffer_frames / (similarity_distance_frames + 1)))``: the most similar frames a
        frame can have, the last axis of ``last_matches``. From the handle's parameters, no device work."""
        return _match_capacity(self._handle())

    def last_matches(self, out=None):
        """The similar frames that the ``T`` frames of the last ``push`` / ``finish`` (``last_frame_range``) matched, as the
        handle used them for the mask: ``repet.Matches(count, age, similarity)`` -- ``count`` int32 ``(S, T)``, the length of a
        frame's list; ``age`` int32 ``(S, T, K)``, how many of the stream's own frames back each similar frame lies, 0 the frame
        itself, strictly ascending, -1 behind the list; ``similarity`` float32 ``(S, T, K)``, the cosine similarity of the pair
        as the peak picking read it, 0 behind the list. ``K`` is ``match_capacity``. NumPy arrays, or tensors on the handle's
        device with no host wait when ``out`` is a triple of dense tensors of those dtypes and shapes (which is filled and
        returned) or the last push was a device chunk. One launch on demand; see ``repet.online_streams``. ValueError for a
        wrong ``out`` (before anything runs) and once a push, finish, finish_stream, restart, release, import, hold or resume
        has followed."""
        return _last_matches(self._handle(), self._device, (self._streams,), out, self._last_on_device)

    def _check_dtype(self, dtype, out):
        """``dtype=`` of a call whose result goes to the host unless ``out`` is given or the last push was a device chunk."""
        if dtype is not None and out is None and not self._last_on_device:
            raise ValueError("dtype is for device results (after host chunks the result is a float64 array)")

    @property
    def samples_pushed(self):
        """Samples per slot pushed into the handle so far."""
        return self._pushed

    def stream_samples(self, slot):
        """Samples of the stream that lives in ``slot`` so far (None: the slot is idle): what the stream itself was fed, without
        the pushes it sat out while it was held."""
        begun = self._begun[self._slot(slot)]
        return None if begun is None else self._pushed - begun

    def _slot(self, slot):
        slot = int(slot)
        if not 0 <= slot < self._streams:
            raise ValueError(f"slot {slot} of a handle of {self._streams}")
        return slot

    def _slot_list(self, slots):
        slots = [self._slot(s) for s in ([slots] if np.isscalar(slots) else slots)]
        return slots, (C.c_int32 * max(len(slots), 1))(*slots)

    def set_background_gain(self, gain, slots=None):
        """Keep ``gain`` (in [0, 1]) of the background in the foreground of the named slots (None: every slot): a scalar, or
        one value per named slot. The next emission fades to it over at most one hop; see ``repet.online_streams``. No host
        wait. ValueError, with nothing changed, for a value outside [0, 1] (NaN included) or a slot out of range."""
        if slots is None:
            g = background_gains(gain)
            check(lib().repet_online_set_background_gain(self._handle(), None, 0, ptr(g)))
            return
        slots, arr = self._slot_list(slots)
        g = background_gains(gain, len(slots))
        check(lib().repet_online_set_background_gain(self._handle(), arr, len(slots), ptr(g)))

    def background_gain(self, slot):
        """The background gain last set for ``slot`` (0: the plain foreground)."""
        out = C.c_float()
        check(lib().repet_online_background_gain(self._handle(), self._slot(slot), C.byref(out)))
        return out.value

    def set_background_band_gains(self, gains, edges=None, slots=None):
        """Keep a share of the background in the foreground of the named slots (None: every slot) band by band. ``gains`` in
        [0, 1]: ``(n_bands,)`` for all named slots or ``(len(slots), n_bands)``; ``edges``: ``n_bands + 1`` ascending bin edges
        in [0, F] (``repet.band_edges`` fits), or None for one gain per bin. A set replaces the slot's whole table; bins outside
        the edges get 0. Frames completed from the next push on are shaped with it; see ``repet.online_streams``. At most one
        small launch, no host wait. ValueError, with nothing changed, for a value outside [0, 1] (NaN included), bad edges, a
        wrong size or a slot out of range."""
        if slots is None:
            _set_band_gains(self._handle, None, 0, gains, edges, self._bins, self._streams)
            return
        slots, arr = self._slot_list(slots)
        _set_band_gains(self._handle, arr, len(slots), gains, edges, self._bins, len(slots))

    def background_band_gains(self, slot):
        """The per-bin gains last set for ``slot``, float32 ``(F,)`` (zeros: the plain foreground). A host copy: no device
        work, no wait."""
        slot = self._slot(slot)
        return _get_band_gains(self._handle(), slot, self._bins)

    def clear_background_band_gains(self, slots=None):
        """Back to the plain foreground for the named slots (None: every slot): every bin's gain 0."""
        self.set_background_band_gains(np.zeros(self._bins, dtype=np.float32), None, slots)

    def restart(self, slots):
        """Begin a new stream in every named slot: its sample 0 is the handle's sample ``samples_pushed``, which must be a
        multiple of the hop (ValueError otherwise, nothing changes). What lived in the slots is discarded. No host wait."""
        slots, arr = self._slot_list(slots)
        check(lib().repet_online_restart_streams(self._handle(), arr, len(slots)))
        for s in slots:
            self._begun[s] = self._pushed
            self._held.discard(s)

    def hold(self, slots):
        """The named live slots sit out the pushes that follow: their share of every chunk is ignored (NaN included), their
        share of everything emitted is zero, and all they hold stays as it is. Only where ``samples_pushed`` is a multiple of
        the hop, and while a slot is held every push is a whole number of hops (ValueError otherwise, nothing changes).
        ValueError for an idle slot; a slot that is held already stays held. ``last_emission`` becomes stale. No host wait."""
        slots, arr = self._slot_list(slots)
        check(lib().repet_online_hold_streams(self._handle(), arr, len(slots)))
        self._held.update(slots)

    def resume(self, slots):
        """The named held slots go on from here as if the pushes since their ``hold`` had not been made; a slot that is not
        held is left alone. Only where ``samples_pushed`` is a multiple of the hop. ``last_emission`` becomes stale. No host
        wait."""
        slots, arr = self._slot_list(slots)
        check(lib().repet_online_resume_streams(self._handle(), arr, len(slots)))
        self._held.difference_update(slots)

    def held(self, slot):
        """True while ``slot`` is held."""
        out = C.c_int32()
        check(lib().repet_online_stream_held(self._handle(), self._slot(slot), C.byref(out)))
        return bool(out.value)

    def enable_feed(self, capacity_samples):
        """Give every slot an inbox of ``capacity_samples`` (at least one hop) samples per channel in device memory, ``S *
        capacity * C * 8`` bytes in all: from here on ``feed`` fills the slots at their own pace and ``tick`` is the push. Once
        per handle, where ``samples_pushed`` is a multiple of the hop (ValueError otherwise, nothing changes)."""
        check(lib().repet_online_enable_feed(self._handle(), int(capacity_samples)))
        self._feed_cap = int(capacity_samples)

    @property
    def feed_capacity(self):
        """Samples per channel every slot's inbox holds (0: ``enable_feed`` has not been called)."""
        return self._feed_cap

    def feed(self, slots, chunk, counts=None):
        """Append samples to the inboxes of live slots. One slot (an int) takes ``(n, C)``; several take ``(len(slots), n, C)``
        and optionally ``counts``, one per slot with ``counts[i] <= n``: row ``i`` brings its first ``counts[i]`` samples and
        the rest of the row is never read. Host arrays (float32 / float64 / int16) or ROCm tensors (those and float16 /
        bfloat16, any strides); a device packet is copied on the current stream's order with no host wait and may be
        overwritten afterwards. All or nothing: ValueError, with nothing enqueued or changed, for a slot out of range, named
        twice or idle, a count outside ``[0, n]``, an inbox that would overflow, and a handle without inboxes or finished. A
        held slot may be fed."""
        single = np.isscalar(slots)
        slots, arr = self._slot_list(slots)
        on_device = is_device_tensor(chunk)
        if on_device:
            if chunk.device.index != self._device:
                raise ValueError(f"tensor is on {chunk.device}, the streams on device {self._device}")
            x = chunk
        else:
            x, code = as_input(chunk.numpy() if is_tensor(chunk) else chunk)
        if single:
            if len(x.shape) != 2:
                raise ValueError("a packet for one slot is (number_samples, number_channels)")
            x = x.unsqueeze(0) if on_device else x[None]
        if len(x.shape) != 3 or x.shape[0] != len(slots) or x.shape[2] != self._channels:
            raise ValueError(f"packets for {len(slots)} slots are ({len(slots)}, number_samples, {self._channels})")
        n = int(x.shape[1])
        cnt = None
        if counts is not None:
            counts = [int(k) for k in ([counts] if np.isscalar(counts) else counts)]
            if len(counts) != len(slots):
                raise ValueError("one count per slot named")
            cnt = (C.c_int64 * max(len(counts), 1))(*counts)
        if on_device:
            import torch
            x, code, shape, strides = tensor_layout(x, batched=True)
            stream = torch.cuda.current_stream(x.device)
            check(lib().repet_online_feed_device(self._handle(), arr, cnt, len(slots), C.c_void_p(x.data_ptr() or None), code, n,
                                                 _strides(strides), _stream_handle(stream), _stream_handle(stream)))
            x.record_stream(stream)
        else:
            check(lib().repet_online_feed(self._handle(), arr, cnt, len(slots), ptr(x), code, n))
        self._feed_on_device = on_device

    def queued(self, slot=None):
        """Samples waiting in the inbox of ``slot``, or of every slot as an int64 ``(S,)`` array. Host counters: no device work."""
        if slot is not None:
            out = C.c_int64()
            check(lib().repet_online_queued(self._handle(), self._slot(slot), C.byref(out)))
            return out.value
        out = np.zeros(self._streams, dtype=np.int64)
        check(lib().repet_online_queued(self._handle(), -1, ptr(out)))
        return out

    def pad_feed(self, slots=None):
        """Feed each named slot (None: every live slot) ``(-queued) % step_length`` zeros, so that its queue ends on the hop
        grid, and return the pad counts (an int for one slot, an int64 array otherwise; ``(S,)`` for None). For a stream that
        ends with a sub-hop remainder: after the ticks that drain the queue, ``finish_stream(slot)[:-pad]`` is its true tail."""
        if slots is None:
            pads = np.zeros(self._streams, dtype=np.int64)
            check(lib().repet_online_pad_feed(self._handle(), None, 0, ptr(pads)))
            return pads
        single = np.isscalar(slots)
        slots, arr = self._slot_list(slots)
        pads = np.zeros(max(len(slots), 1), dtype=np.int64)
        check(lib().repet_online_pad_feed(self._handle(), arr, len(slots), ptr(pads)))
        return int(pads[0]) if single else pads[:len(slots)]

    def clear_feed(self, slots=None):
        """Empty the inboxes of the named slots (None: of all): what was queued is dropped. No device work."""
        if slots is None:
            check(lib().repet_online_clear_feed(self._handle(), None, 0))
            return
        slots, arr = self._slot_list(slots)
        check(lib().repet_online_clear_feed(self._handle(), arr, len(slots)))

    def tick(self, hops=1, out=None, which="background", dtype=None):
        """The lockstep push of ``hops * step_length`` samples whose chunk the handle assembles from the inboxes. Every live
        slot that is not held and has that many samples queued is *ready* and its oldest samples are consumed; every other
        live slot that is not held is *starved*: held for this push, so it emits zeros and its stream goes on bit for bit
        later. Returns what ``push`` returns (``out``, ``which``, ``dtype`` as there): a tensor when ``out`` is a tensor or the
        last ``feed`` was a device tensor, else NumPy. With nobody ready nothing runs, None is returned and the handle, its
        last emission and its records stay as they were. ``last_consumed`` says who took part. ValueError unless
        ``samples_pushed`` is a multiple of the hop. No host wait on the device path; nothing is read back."""
        codes = which_codes(which)
        on_device = out is not None or self._feed_on_device
        if dtype is not None and not on_device:
            raise ValueError("dtype is for device results (after host packets the result is a float64 array)")
        if self._feed_cap <= 0:
            raise ValueError("the handle has no inboxes: enable_feed comes first")
        hops = int(hops)
        if hops < 1:
            raise ValueError("a tick is at least one hop")
        n = hops * self._hop
        n_emit = self.emit_count(n)
        consumed = np.zeros(self._streams, dtype=np.uint8)
        h = self._handle()
        results, _ = self._emit(
            codes, n_emit, on_device, out, dtype,
            lambda dst, cap, written: lib().repet_online_tick(h, hops, dst, cap, ptr(consumed), written),
            lambda dst, code, strides, stream, written: lib().repet_online_tick_device(
                h, hops, dst, code, _strides(strides), stream, ptr(consumed), written))
        self._consumed = consumed.astype(bool)
        if not self._consumed.any():
            return None
        self._pushed += n
        for s in range(self._streams):                # time does not pass for a slot that sat the tick out
            if self._begun[s] is not None and not self._consumed[s]:
                self._begun[s] += n
        self._last_on_device = on_device
        self._emitted_shape = tuple(results[0].shape)
        self._tail_emitted = False
        return results[0] if len(results) == 1 else tuple(results)

    @property
    def last_consumed(self):
        """bool ``(S,)``: the slots whose samples the last ``tick`` consumed (all False where nobody was ready)."""
        return self._consumed.copy()

    def release(self, slots):
        """The named slots become idle without output: they ignore their share of the chunks and emit zeros."""
        slots, arr = self._slot_list(slots)
        check(lib().repet_online_release_streams(self._handle(), arr, len(slots)))
        for s in slots:
            self._begun[s] = None
            self._held.discard(s)

    @property
    def stream_state_nbytes(self):
        """Bytes of the payload of a ``StreamState`` of this handle (they depend on the sampling frequency, the buffer
        length and the channel count alone)."""
        return _state_sizes(self._handle())[1]

    def export_stream(self, slot, device=False):
        """A snapshot of the stream that lives in ``slot`` as a ``StreamState``; the slot lives on untouched and
        ``last_emission`` stays valid (migration is ``export_stream`` + ``release``; a snapshot imported twice is a fork).
        ``device=True``: the payload is a ``torch.uint8`` tensor on the handle's device, ordered on the current torch stream
        with no host wait; otherwise a ``numpy.uint8`` array (this form waits for its copy). ValueError for an idle slot or
        unless ``samples_pushed`` is a multiple of the hop."""
        return _export_state(self._handle(), self._slot(slot), self._device if device else None)

    def import_stream(self, slot, state):
        """Load ``state`` (a ``StreamState`` of a handle opened with the same parameters) into ``slot``, dropping what lived
        there as ``restart`` does: the slot goes on bit for bit as the exporting one would have. The payload may be a host
        array or a ROCm tensor on any device (a device payload enqueues only). ValueError, before any launch and with nothing
        changed, unless ``samples_pushed`` is a multiple of the hop, and for a state of another geometry or other
        parameters, a payload of the wrong size or dtype, or an unknown magic word or version. ``last_emission`` becomes
        stale."""
        slot = self._slot(slot)
        fields = _import_state(self._handle(), slot, state, self._device)
        self._begun[slot] = self._pushed - fields["length_samples"]
        self._held.discard(slot)

    def stream_emit_count(self, slot):
        """Samples ``finish_stream(slot)`` will return. ValueError for an idle slot or a stream shorter than the buffer."""
        n = C.c_int64()
        check(lib().repet_online_stream_emit_count(self._handle(), self._slot(slot), C.byref(n)))
        return n.value

    def finish_stream(self, slot, out=None, which="background", dtype=None):
        """End the stream of one slot where the handle stands: its ``(n_rest, C)`` tail, as ``finish`` returns for all (a
        tensor on the device when ``out`` is given or the last push was a device chunk; the signal ``which`` names, a pair
        for "both"). The other slots and the handle's counters are untouched and the slot is idle afterwards. ValueError for
        an idle slot, or for a stream shorter than the buffer (the slot then stays as it was). ``dtype``: as ``push``'s, for a
        result on the device."""
        codes = which_codes(which)
        self._check_dtype(dtype, out)
        slot = self._slot(slot)
        n_emit = self.stream_emit_count(slot)
        h = self._handle()
        results, _ = self._emit(
            codes, n_emit, out is not None or self._last_on_device, out, dtype,
            lambda dst, cap, written: lib().repet_online_finish_stream(h, slot, dst, cap, written),
            lambda dst, code, strides, stream, written: lib().repet_online_finish_stream_device(
                h, slot, dst, code, (C.c_int64 * 2)(*strides), stream, written),
            shape=(n_emit, self._channels))
        self._begun[slot] = None
        self._held.discard(slot)
        self._tail_emitted = True
        return results[0] if len(results) == 1 else tuple(results)

    def finish(self, out=None, which="background", dtype=None):
        """End every stream: the remaining samples, ``(S, n_rest, C)`` -- a float64 tensor on the device when ``out`` is given
        or the last push was a device chunk, a NumPy array otherwise; the signal ``which`` names, a pair for "both". ValueError
        if the handle has seen fewer samples than the buffer holds. Every live slot ends with its own length; idle slots
        return zeros. ``dtype``: as ``push``'s, for a result on the device."""
        codes = which_codes(which)
        self._check_dtype(dtype, out)
        n_emit = self.emit_count(0, finishing=True)
        h = self._handle()
        results, _ = self._emit(
            codes, n_emit, out is not None or self._last_on_device, out, dtype,
            lambda dst, cap, written: lib().repet_online_finish_streams(h, dst, cap, written),
            lambda dst, code, strides, stream, written: lib().repet_online_finish_device(h, dst, code, _strides(strides), stream, written))
        self._held.clear()
        self._emitted_shape = tuple(results[0].shape)
        self._tail_emitted = False
        return results[0] if len(results) == 1 else tuple(results)

    def close(self):
        if self._h:
            lib().repet_online_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
