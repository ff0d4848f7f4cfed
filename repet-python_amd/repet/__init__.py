"""repet -- MI355X-native REPET (REpeating Pattern Extraction Technique), drop-in for zafarrafii/REPET-Python.

Same call surface as the reference module ``repet.py``::

    background_signal = repet.original(audio_signal, sampling_frequency)    # repet.py:67
    background_signal = repet.extended(audio_signal, sampling_frequency)    # repet.py:205
    background_signal = repet.adaptive(audio_signal, sampling_frequency)    # repet.py:422
    background_signal = repet.sim(audio_signal, sampling_frequency)         # repet.py:571
    background_signal = repet.simonline(audio_signal, sampling_frequency)   # repet.py:712

``audio_signal`` is ``(number_samples, number_channels)``; the result is a fresh float64 array of the
same shape. A torch tensor on a ROCm device is separated where it lies: the result is a float64 tensor on the same
device, ordered on that device's current stream without a host wait (``separate`` also takes batches and ``out=``). The nine module-level parameters below have the reference's names and defaults
(repet.py:42-63) and are read at call time, so ``repet.period_range = [1, 5]`` before a call behaves as
it does there. All arithmetic runs in hand-written HIP kernels for gfx950 behind ``librepet_hip.so``
(``include/repet_hip.h``); this module only validates, derives the integer sizes with the reference's
own rounding rules, and crosses the C ABI. There is no NumPy/CPU implementation of the separation
path here: without the library or a GPU the calls raise.
"""
import functools

import numpy as np

from . import _native
from ._native import Context  # noqa: F401  (device-resident API used by bench.py)
from ._native import OnlineSeparator as _OnlineSeparator
from ._native import StreamState  # noqa: F401  (what export_stream returns and import_stream takes)
from ._native import LEVELS  # noqa: F401  (the eight fields of a level record, in index order)
from ._native import Matches  # noqa: F401  (what last_matches of a live handle returns: count, age, similarity)

# ---- public parameters (repet.py:42-63) ----------------------------------------------------------------
cutoff_frequency = 100
period_range = [1, 10]
segment_length = 10
segment_step = 5
filter_order = 5
similarity_threshold = 0
similarity_distance = 1
similarity_number = 100
buffer_length = 10

# Not a parameter of the reference: what to do with samples that are NOT FINITE. repet.py computes on (a NaN sample makes the
# frames that hold it NaN; repet.py:125 has no input check). True (default since round 6: the reference's behaviour): the
# samples are let through and every variant returns what the reference returns for NaN samples (``sim`` / ``simonline``: NaN
# on the samples of the affected frames only; the period family: also at the same position of every period, and the period
# ``period_range[0] + 1``); an infinite sample is treated as NaN. False: such input raises ValueError
# (REPET_FLAG_REFUSE_NONFINITE). Read at call time like the others.
strict_reference = True

_device = 0  # HIP device used by the one-shot calls


def set_device(index):
    """Select the HIP device for subsequent calls (the reference has no such notion)."""
    global _device
    _device = int(index)


def device_host_cpus(device=None):
    """CPUs of the NUMA node the device hangs off, among those this process may use ([] when unknown or nothing to choose)."""
    import ctypes as C
    dev = _device if device is None else int(device)
    n = C.c_int32()
    buf = (C.c_int32 * 4096)()
    _native.check(_native.lib().repet_device_host_cpus(dev, buf, 4096, C.byref(n)))
    return [int(buf[i]) for i in range(min(n.value, 4096))]


def bind_host_to_device(device=None):
    """Bind the calling process (thread) to the CPUs of the device's NUMA node -- what ``numactl --cpunodebind`` would do for a
    GPU job. Arrays first touched afterwards live there too. Returns the previous affinity mask (``os.sched_setaffinity(0,
    previous)`` undoes it), or None when there is nothing to choose. Not done implicitly: the affinity of the caller's
    threads is the caller's business (the library pins only its own conversion threads)."""
    import os
    cpus = device_host_cpus(device)
    if not cpus:
        return None
    previous = os.sched_getaffinity(0)
    os.sched_setaffinity(0, cpus)
    return previous


# ---- sizes derived exactly as the reference derives them ---------------------------------------------------
def _window_length(sampling_frequency):
    return pow(2, int(np.ceil(np.log2(0.04 * sampling_frequency))))  # repet.py:130


def derive_params(sampling_frequency):
    """Snapshot the module parameters into the integer ``repet_params`` of the C ABI.

    Python ``round`` and ``np.round`` are half-to-even; every expression below is the one the reference
    evaluates (line cited), so e.g. an 8 kHz clip gets a 312-frame online buffer (``round(312.5)``).
    """
    fs = sampling_frequency
    w = _window_length(fs)
    h = int(w / 2)                                                            # repet.py:132
    pr = np.round(np.array(period_range) * fs / h).astype(int)                # repet.py:165
    p = _native.Params()
    p.window_length = w
    p.step_length = h
    p.period_lo = int(pr[0])
    p.period_hi = int(pr[1])
    p.cutoff_bins = int(round(cutoff_frequency * w / fs))                     # repet.py:173
    p.filter_order = int(filter_order)
    p.seg_len_frames = int(round(segment_length * fs / h))                    # repet.py:519
    p.seg_step_frames = int(round(segment_step * fs / h))                     # repet.py:520
    p.sim_distance_frames = int(round(similarity_distance * fs / h))          # repet.py:670
    p.sim_number = int(similarity_number)
    p.buffer_frames = int(round((buffer_length * fs) / h))                    # repet.py:787
    p.seg_len_samples = int(round(segment_length * fs))                       # repet.py:266
    p.seg_step_samples = int(round(segment_step * fs))                        # repet.py:267
    p.sim_threshold = float(similarity_threshold)
    p.flags = 0 if strict_reference else _native.FLAG_REFUSE_NONFINITE
    return p


def release_workspaces():
    """Free the device workspaces the one-shot calls of THIS thread keep between calls (the reference has no such
    notion: its arrays die with the call). Worth calling after a one-off long ``sim``: the similarity matrix of a
    10-minute clip is several GB of HBM."""
    _native.check(_native.lib().repet_release_thread_ctx())
    _native.release_tensor_contexts()


def _separate_tensor(algo, audio_signal, sampling_frequency, out=None, batched=False, which="background", background_gain=None,
                     levels=False, dtype=None, band_gains=None, flags=0, lengths=None, frames=None):
    """A torch tensor on a ROCm device: ingest, run and egress on the tensor's own device, ordered on its current stream by
    events (no host wait; the refusal mode ``strict_reference = False`` waits once, for the non-finite check). ``which``
    selects what the egress writes; "both" is two egress launches behind one run. ``background_gain``: a float that ``separate``
    has checked, or None. ``levels``: also the level record of the result (one reduction launch more, two for a long clip), under
    the same gain. ``band_gains``: ``(edges, g)`` that ``separate`` has checked with ``band_gain_rows``, or None. ``flags``: bits
    ``separate`` adds to this call's ``Params.flags`` (``silent_frames``). ``lengths``: what ``_native.clip_lengths`` made of
    ``separate``'s, or None; a clip too short for ``algo`` is refused here, before the context is touched. ``frames``: what
    ``_native.frames_request`` made of ``separate``'s ``frames`` / ``frame_bands`` / ``frames_out``, or None; the spectra are
    armed on the context in front of the run and returned behind the result (and the levels)."""
    import torch
    names = ("background", "foreground") if which == "both" else (which,)
    _native.which_codes(which)
    params = derive_params(sampling_frequency)
    params.flags |= flags
    layout = _native.tensor_layout(audio_signal, batched)
    x, shape = layout[0], layout[2]
    result_shape = shape if x.dim() == 3 else shape[1:]
    outs = _native.out_pair(out) if which == "both" else (out,)
    _native.emit_dtype(dtype, outs)
    for o in outs:
        if o is None:
            continue
        if not _native.is_device_tensor(o) or o.device != x.device:
            raise ValueError(f"out must be a tensor on {x.device}")
        if tuple(o.shape) != result_shape:
            raise ValueError(f"out has shape {tuple(o.shape)}, the result {result_shape}")
        _native.emit_tensor_code(o)
    if lengths is not None:
        _native.check_clip_lengths(algo, params, lengths)
    ctx = _native.tensor_context(x.device.index)
    ctx.set_strict_reference(strict_reference)
    stream = torch.cuda.current_stream(x.device)
    ctx.upload_layout(*layout, stream=stream, lengths=lengths)
    record = None
    # gains: on this thread's cached context for this call alone -- later calls are the plain foreground again, whatever
    # happens here. The band table shapes the run it is set in front of; the scalar gain acts in the egress.
    try:
        if band_gains is not None:
            ctx.set_background_band_gains(band_gains[1], band_gains[0], window_length=params.window_length)
        if frames is not None:
            signal, edges, spectra, spectra_shape = frames
            if spectra is None:
                spectra = torch.empty(spectra_shape, dtype=torch.float32 if edges is None else torch.float64, device=x.device)
            ctx.request_frames(algo, params, signal, spectra, bands=edges, stream=stream)
        ctx.execute_async(algo, params)
        if background_gain is not None:
            ctx.set_background_gain(background_gain)
        results = tuple(ctx.download_tensor(o, stream, name, dtype) for o, name in zip(outs, names))
        if levels:
            record = ctx.result_levels(stream=stream)
    finally:
        if background_gain is not None:
            ctx.set_background_gain(0.0)
        if band_gains is not None:
            ctx.clear_background_band_gains()
        if frames is not None:
            ctx.clear_requests()                  # (dropped by the execute; still armed only where the call failed before it)
    results = results if which == "both" else results[0]
    extras = ((record,) if levels else ()) + ((spectra,) if frames is not None else ())
    return (results,) + extras if extras else results


def _separate(algo, audio_signal, sampling_frequency):
    if _native.is_device_tensor(audio_signal):
        return _separate_tensor(algo, audio_signal, sampling_frequency)
    number_samples, number_channels = np.shape(audio_signal)   # 1-D input: ValueError, like repet.py:125
    params = derive_params(sampling_frequency)
    signal, code = _native.as_input(audio_signal)
    background_signal = _native.result_array((number_samples, number_channels))
    lib = _native.lib()
    if lib.repet_device_count() < 1:
        raise RuntimeError("no HIP device visible: the REPET engine has no CPU fallback")
    _native.check(lib.repet_run(_native.ALGO_IDS[algo], _native.ptr(signal), code, number_samples,
                                number_channels, params, _native.ptr(background_signal), _device, None))
    return background_signal


def original(audio_signal, sampling_frequency):
    """Original REPET: one repeating period, period-median model (repet.py:67-202)."""
    return _separate("original", audio_signal, sampling_frequency)


def extended(audio_signal, sampling_frequency):
    """REPET extended: ``original`` on 10-s segments with triangular cross-fades (repet.py:205-419)."""
    return _separate("extended", audio_signal, sampling_frequency)


def adaptive(audio_signal, sampling_frequency):
    """Adaptive REPET: time-varying period from a beat spectrogram (repet.py:422-568)."""
    return _separate("adaptive", audio_signal, sampling_frequency)


def sim(audio_signal, sampling_frequency):
    """REPET-SIM: repeating frames found through the cosine self-similarity matrix (repet.py:571-709)."""
    return _separate("sim", audio_signal, sampling_frequency)


def simonline(audio_signal, sampling_frequency):
    """Online REPET-SIM over a circular buffer of past frames (repet.py:712-911)."""
    return _separate("simonline", audio_signal, sampling_frequency)


def _separate_surface(algo, audio_signal, sampling_frequency, out=None, which="background", background_gain=None, levels=False, dtype=None,
                      silent_frames="reference", background_band_gains=None, band_edges=None):
    """``algo`` ("original", "extended", "adaptive", "sim", "simonline") of a torch tensor on a ROCm device: ``(N, C)`` or a
    batch ``(B, N, C)`` of equal clips -- or, with ``lengths``, of clips of unequal lengths -- (``simonline`` runs every stage once
    over all of them, the others work through the clips one after another). Returns a float64 tensor on the tensor's device -- one of ``dtype``, where given -- or fills
    ``out``, a float64 / float32 / int16 / float16 / bfloat16 tensor of the same shape with any strides, and returns it. Every
    clip's result is what the one-clip call returns, bit for bit; the work is ordered on the device's current stream with no
    host wait (see ``_separate_tensor``).

    A destination dtype is the inverse of the same source dtype: a cast of the float64 value the egress forms, never a rescale,
    rounded once. float16 / bfloat16: the nearest value, ties to even, straight from float64 (``result.to(torch.bfloat16)`` of
    a float64 result rounds twice), inf beyond the largest finite value. int16: rounded to nearest, ties to even, saturated to
    [-32768, 32767], NaN 0 -- int16 PCM in, int16 PCM out in the same units; a +-1.0 float signal written as int16 is 0 / +-1.
    ``dtype`` beside an ``out`` of another dtype, and a pair of two dtypes, are a ValueError before anything runs.

    ``which``: "background" (default), "foreground" -- ``audio_signal - background`` written by the egress itself, in float64
    from the samples as the engine holds them (exact for float32 / float16 / bfloat16 / int16 tensors; 48 bits of a float64
    sample, so within ``2**-47 * max(|x|, |background|)`` of the float64 subtraction), rounded once more for a float32
    ``out`` --, "mixture" (the input as the engine holds it) or "both": the pair ``(background, foreground)``, with ``out`` a
    pair of tensors that share no memory.

    ``background_gain`` (a number in [0, 1], with ``which="foreground"`` or ``"both"`` only): keep that share of the background,
    ``foreground = x - float32(1 - background_gain) * background``, rounded once in float64 by the same egress (-12 dB of
    background: ``10 ** (-12 / 20)``; 0 is the plain foreground, 1 the input). For this call alone. ValueError for a value
    outside [0, 1] (NaN included) or with another ``which``.

    ``background_band_gains`` (with ``which="foreground"`` or ``"both"`` only): keep a share of the background BAND BY BAND.
    ``(n_bands,)`` gains in [0, 1], or ``(B, n_bands)`` for a batch (one row per clip); ``band_edges`` the ``n_bands + 1``
    ascending bin edges in ``[0, window_length / 2 + 1]`` (:func:`band_edges` fits) or None for one gain per bin. The foreground
    is formed from a SHAPED background: the variant's own inverse STFT of the masked spectrum with bin ``k`` multiplied by
    ``float32(1 - g[k])`` (a second inverse launch behind each plain one), so a gain of 1 over the bass bins gives the bass the
    high-pass rule hands to the background back to the foreground. The returned background, the mixture and their levels keep
    their bits; ``background_gain`` multiplies on top; ``levels=True`` measures the shaped foreground; all zeros is the plain
    call bit for bit. For this call alone. ValueError, before the library is touched, for gains outside [0, 1] (NaN included),
    bad edges, a wrong size or another ``which``; windows above 4096 samples (sampling frequencies above 102.4 kHz) are refused
    by the library.

    ``levels=True`` returns ``(result, levels)``: the level record of the call (``repet.LEVELS``: per channel the sums of squares
    and the largest magnitudes of mixture, background and foreground, the samples and those whose mixture is not finite), a
    float64 tensor ``(C, 8)`` -- ``(B, C, 8)`` for a batch -- on the tensor's device, reduced there from the float64 values the
    egress forms (whatever ``which`` and the dtype of ``out`` are, under this call's ``background_gain``), with no host wait.
    Deterministic: the same call returns the same bits. See :func:`online_streams` for the fields.

    ``silent_frames`` (``algo="simonline"`` only): "reference" (default) answers a frame of digital silence with NaN, as the
    reference does; "zero" separates through it, see :func:`online`. For this call alone. ValueError, before the library is
    touched, for any other string and for "zero" with another ``algo``. Pass it, and the band gains behind it, by keyword.

    ``lengths`` (keyword only, with a ``(B, N, C)`` tensor only): a RAGGED batch -- clips of unequal lengths, padded to ``N``
    (``torch.nn.utils.rnn.pad_sequence(clips, batch_first=True)`` makes one). A sequence of ``B`` integers in ``[0, N]`` on the
    HOST: a list, a NumPy integer array or a CPU tensor. Clip ``b`` is ``audio_signal[b, :lengths[b]]``; the samples behind it
    are never read -- they may hold NaN, infinities or stale memory, do not trip ``strict_reference = False`` and reach no
    result. The result has the shape of the input: ``result[b, :lengths[b]]`` equals, as values, what the one-clip call
    ``separate(algo, audio_signal[b, :lengths[b]], ...)`` returns -- for every ``which``, ``out`` / ``dtype``, gain and
    ``silent_frames`` (the sign of a zero may differ) --, ``result[b, lengths[b]:]`` is zero. With ``levels=True`` clip ``b``'s
    record is that of its own ``lengths[b]`` samples, bit for bit. ``simonline`` still runs every stage once over all clips
    (plus one launch that clears the frames behind each clip's end); ``sim``, ``adaptive``, ``extended`` AND ``original`` -- which
    gives up its batched form here -- work through the clips one by one. Padding the clips and calling without ``lengths`` is
    not the same thing: the zeros become frames every variant hears. TypeError for ``lengths`` on a device (the call must not
    wait for it) or not integers; ValueError for a wrong count, a value outside ``[0, N]`` or a 2-D tensor -- all before the
    library is touched --, and, before anything is uploaded or enqueued, for a clip too short for ``algo``: the one-clip call's
    message with the clip named in front (a clip of no samples is too short for every variant). Lengths that all equal ``N``
    are the equal-length call, bit for bit.

    ``frames`` (keyword only): "mixture", "background" or "foreground" -- also return the SPECTRA the call decided, as a tensor
    behind the result: the order is ``result[, levels][, frames]``. float32 ``(T, C, F)`` for an ``(N, C)`` input, ``(B, T, C,
    F)`` for a batch, ``F = window_length / 2 + 1``, ``T = repet.frame_count(algo, N, sampling_frequency)``, on the input's
    device, ordered as the result is: no second STFT, no host wait, no readback. The contract is the live handles'
    (``last_frames``): the mixture is the magnitude spectrogram as the forward transform stored it, bit for bit; the background
    is the magnitude of the masked bin as the variant's inverse STFT fetches it, so it equals the mixture to the bit in the
    high-pass bins ``1 .. cutoff``; the foreground is mixture - background, 0 where a rounding makes that negative, NaN where
    either is NaN. "original", "adaptive" and "sim" frame ``j`` begins at sample ``j * H - W / 2``; "simonline" frame ``j`` at
    ``j * H``, and its warm-up frames (``j < buffer_frames - 1``) have background 0 and foreground = mixture. With ``lengths``,
    clip ``b``'s frames at or past ``repet.frame_count(algo, lengths[b], ...)`` are zero in all three signals. The gains do not
    change the spectra. One launch more per pass of the variant's pipeline (one per clip where the clips are worked through
    one by one); a call without ``frames`` enqueues what it always did.
    ``frame_bands`` (with ``frames``): ``n_bands + 1`` ascending bin edges in ``[0, F]``, at most 128 bands
    (``repet.band_edges(fs, 32)`` fits): float64 band energies ``(..., T, C, n_bands)`` instead, each the sum of
    ``float64(m) ** 2`` over the band's bins, reduced in a fixed order (the same call returns the same bits).
    ``frames_out`` (with ``frames``): the destination, a float32 tensor of the frames' shape with any non-overlapping strides --
    float64 and dense for bands -- on the input's device; it is returned in the frames' place.
    ValueError, before the library is touched, for an unknown ``frames``, ``frame_bands`` or ``frames_out`` without ``frames``,
    bad edges, a destination of the wrong shape, dtype or device, and ``algo="extended"`` (its segments overlap and cross-fade:
    there is no single spectrogram)."""
    raise NotImplementedError("the documented surface of repet.separate: the call itself is _separate_checked")


def _separate_checked(algo, audio_signal, sampling_frequency, out=None, which="background", background_gain=None, levels=False, dtype=None,
                      silent_frames="reference", background_band_gains=None, band_edges=None, lengths=None, frames=None,
                      frame_bands=None, frames_out=None):
    if algo not in _native.ALGO_IDS:
        raise ValueError(f"unknown algorithm {algo!r}")
    if frames is not None or frame_bands is not None or frames_out is not None:
        frames = _native.frames_request(algo, derive_params(sampling_frequency), frames, frame_bands, frames_out,
                                        getattr(audio_signal, "shape", ()), getattr(audio_signal, "device", None))
    if lengths is not None:
        lengths = _native.clip_lengths(lengths, getattr(audio_signal, "shape", ()))
    flags = _native.silent_frames_flag(silent_frames, algo)
    _native.which_codes(which)
    if background_gain is not None:
        if which not in ("foreground", "both"):
            raise ValueError('background_gain changes the foreground: it goes with which="foreground" or "both"')
        background_gain = float(_native.background_gains(background_gain)[0])
    band_gains = None
    if background_band_gains is not None:
        if which not in ("foreground", "both"):
            raise ValueError('background_band_gains change the foreground: they go with which="foreground" or "both"')
        shape = tuple(getattr(audio_signal, "shape", ()))
        band_gains = _native.band_gain_rows(background_band_gains, band_edges, derive_params(sampling_frequency).window_length // 2 + 1,
                                            int(shape[0]) if len(shape) == 3 else None)
    elif band_edges is not None:
        raise ValueError("band_edges go with background_band_gains")
    if not _native.is_device_tensor(audio_signal):
        raise TypeError("separate takes a torch tensor on a ROCm device (host arrays: repet.<algo>, repet.run_batch)")
    return _separate_tensor(algo, audio_signal, sampling_frequency, out=out, batched=True, which=which,
                            background_gain=background_gain, levels=bool(levels), dtype=dtype, band_gains=band_gains, flags=flags,
                            lengths=lengths, frames=frames)


# ``lengths`` is keyword-only. The positional parameters of ``separate`` are a published list that ends in ``silent_frames`` and
# the band-gain pair (callers and checks go by those positions), so the keyword is taken off in front of that list, not appended
# to it: ``inspect.signature(repet.separate)`` and ``help`` show the list as it was, the docstring describes ``lengths``.
# ``frames``, ``frame_bands`` and ``frames_out`` are keyword-only in the same way.
@functools.wraps(_separate_surface)
def separate(*args, lengths=None, frames=None, frame_bands=None, frames_out=None, **kwargs):
    return _separate_checked(*args, lengths=lengths, frames=frames, frame_bands=frame_bands, frames_out=frames_out, **kwargs)


def frame_count(algo, number_samples, sampling_frequency):
    """Frames ``T`` of the spectra ``separate(..., frames=...)`` returns for clips of ``number_samples`` samples at
    ``sampling_frequency``: ``ceil(N / H) + 1`` for "original", "adaptive" and "sim" (the reference's centred STFT, frame ``j``
    begins at sample ``j * H - W / 2``), the online count for "simonline" (frame ``j`` begins at ``j * H``). Host arithmetic: no
    device is needed. ValueError for "extended", which has no single frame grid."""
    return _native.result_frame_count(algo, derive_params(sampling_frequency), number_samples)


def online(sampling_frequency, number_channels, start_length=None, silent_frames="reference"):
    """Streaming form of :func:`simonline` (the reference needs the whole signal up front): returns an object with
    ``push(chunk) -> newly final background samples`` and ``finish() -> the remaining ones``. The module parameters are
    snapshotted now; the concatenated output equals ``simonline`` of the concatenated input.

    ``push(chunk, which=...)`` / ``finish(which=...)``: "background" (default), "foreground" -- the input minus the background
    of exactly the emitted samples (the output runs behind the input; the handle keeps the delay line) --, "mixture" (those
    input samples themselves) or "both", the pair ``(background, foreground)``. The concatenated foreground equals
    ``x - simonline(x)``; during the 10-s warm-up, where ``simonline`` is silent, it is the input itself.

    ``export_stream()`` returns the stream's state as a :class:`StreamState` (a snapshot; only where the samples pushed so
    far are a multiple of the hop) and ``import_stream(state)`` loads one into this separator, which then goes on as the
    exporting stream would have: see :func:`online_streams`.

    ``set_background_gain(gain)`` keeps ``gain`` (in [0, 1]) of the background in the foreground, ``x - float32(1 - gain) *
    background``, fading to it over at most one hop; ``background_gain()`` reads it back: see :func:`online_streams`.
    ``set_background_band_gains(gains, edges=None)``, ``background_band_gains()`` and ``clear_background_band_gains()`` keep a
    share of the background band by band, as :func:`online_streams` describes (here without ``slots``).

    ``last_frames(which="foreground", bands=None, out=None)`` returns the spectra of the frames the last ``push`` / ``finish``
    completed (``last_frame_range`` tells which), float32 magnitudes ``(T, number_channels, window_length / 2 + 1)`` or, with
    ``bands``, float64 band energies ``(T, number_channels, n_bands)``: see :func:`online_streams`.

    ``last_matches(out=None)`` returns the similar frames those frames matched, ``Matches(count, age, similarity)`` of shapes
    ``(T,)``, ``(T, match_capacity)`` and ``(T, match_capacity)``: see :func:`online_streams`.

    ``start_length`` (seconds; None: ``buffer_length``, the reference): separate before the buffer has filled. The reference
    writes nothing until its buffer holds ``buffer_length`` (10 s) of frames; with ``start_frames = min(buffer_frames, max(1,
    round(start_length * fs / step_length)))`` (the ``start_frames`` property) a stream's frame ``j >= start_frames - 1`` is
    separated on the ``min(buffer_frames, j + 1)`` frames it has heard so far -- exactly what the reference computes for its
    first processed frame with a buffer of ``j + 1`` frames -- and from frame ``buffer_frames - 1`` on nothing changes, bit for
    bit. Below ``start_length`` the foreground is still the input, as today, and a stream can be finished once it has
    ``(start_frames - 2) * step_length + window_length`` samples. While ``j <= similarity_distance`` (in frames) a young
    frame's only similar frame is itself: its mask is 1, so the whole input counts as background and the foreground is
    silent. A sensible ``start_length`` is therefore at least two or three times ``similarity_distance``.

    ``silent_frames`` ("reference", the default, or "zero"; the ``silent_frames`` property): what the stream makes of whole
    frames of digital silence -- a muted microphone, a decoder that writes exact zeros, the lead-in of a file. The reference
    divides such a frame's mean magnitude row by its norm, 0 / 0: the frame's samples come out NaN (background, foreground,
    ``last_levels``, ``last_frames``; only an int16 destination hides it), and while the frame sits in the 10-s buffer no frame
    within ``similarity_distance`` of it can be anybody's similar frame. "zero": a frame whose float32 norm is exactly 0 (exact
    zeros; magnitudes below about 4e-23 count too; a frame with a NaN sample does not) gets the unit row 0, so its similarity
    with every frame, itself included, is 0; it has no similar frames (``last_matches``: count 0, ages -1, similarities 0), is
    in no other frame's list, and adds 0 to the overlap-add (``last_frames`` is 0 there in all three signals, the frames around
    it ring into its samples as usual); every other frame is the reference's on a similarity vector with zeros in the silent
    columns. A stream without a silent frame gives the same bits under either rule. A frame whose list is empty for another
    reason (a NaN sample, an exact tie) stays NaN. The rule belongs to the handle: ``import_stream`` refuses a state exported
    under the other one. Any other string is a ValueError."""
    params = derive_params(sampling_frequency)
    params.flags |= _native.silent_frames_flag(silent_frames)
    return _OnlineSeparator(params, number_channels, _device, _native.start_frames_for(params, sampling_frequency, start_length))


def online_streams(sampling_frequency, number_channels, number_streams, max_push_samples=None, start_length=None,
                   silent_frames="reference"):
    """Many live streams at once: ``number_streams`` streams of ``number_channels`` channels at one sampling frequency in ONE
    streaming handle on the device of :func:`set_device`, pushed in lockstep. ``push(chunk, out=None)`` takes a chunk
    ``(number_streams, n, number_channels)`` -- a host array, or a ROCm tensor (the dtypes :func:`separate` takes, any strides)
    -- and returns the ``(number_streams, n_emit, number_channels)`` background samples that became final: a float64 array
    for a host chunk; for a tensor a float64 tensor on its device (``dtype=``: one of that torch dtype), or ``out`` (float64 /
    float32 / int16 / float16 / bfloat16, any strides) filled, ordered on the current stream with no host wait. A destination
    dtype is the inverse of the same source dtype -- a cast of the float64 value of the emission, never a rescale, rounded once
    to nearest, ties to even, by the launch that writes it (int16 saturates, NaN 0; the 16-bit floats go to inf beyond their
    largest finite value): int16 hops in, int16 hops out, at the launches a float32 ``out`` costs. ``finish``,
    ``finish_stream`` and ``last_emission`` take ``dtype=`` likewise; with a host chunk, or beside an ``out`` of another dtype,
    it is a ValueError. ``last_levels`` measures the float64 values before that store, whatever the dtype. ``finish(out=None)`` returns the rest, ``close()`` frees the device state. Each
    stream's concatenated output equals ``simonline`` of its concatenated input, bit for bit. ``max_push_samples`` sizes the
    device buffers at open (pushes up to that size then never grow them); the module parameters are snapshotted now.

    Streams need not start and end together: the handle's streams are *slots*. ``restart(slots)`` begins a new stream in each
    named slot at the handle's current sample (``samples_pushed``, which must be a multiple of the hop); ``finish_stream(slot,
    out=None)`` ends one stream wherever the handle stands and returns its ``(n_rest, number_channels)`` tail
    (``stream_emit_count(slot)`` tells its size; ValueError for an idle slot or a stream shorter than the buffer);
    ``release(slots)`` drops streams without output. An idle slot ignores its share of every chunk, NaN included, and emits
    zeros. Pushes stay in lockstep and none of these calls waits for the device (``finish_stream`` to the host waits for its
    result). A slot's output from its ``restart`` on, followed by its ``finish_stream`` (or ``finish``) tail, equals
    ``simonline`` of the samples pushed into it in between, bit for bit: zeros while it warms up, then its own buffer only.
    ``stream_samples(slot)`` is the length of a slot's stream so far (None when idle). A server loop: open with
    ``max_push_samples``, ``release`` every slot, ``restart`` a free slot when a call arrives, ``finish_stream`` it when the
    call ends.

    ``push``, ``finish`` and ``finish_stream`` take ``which="background"`` (default) / ``"foreground"`` / ``"mixture"`` /
    ``"both"``: the foreground is the input minus the background OF THE EMITTED SAMPLES -- the output runs behind the input
    (``n_emit != n``), and the handle subtracts from its own copy of them, per slot, at no extra launch. ``"mixture"`` is
    that delay-compensated input; ``"both"`` returns ``(background, foreground)`` from one pass (``out=`` then takes a pair
    of tensors of one dtype that share no memory). Per life the foreground equals ``x - simonline(x)`` bit for bit (float64
    input that is not float32 + float32 exact: within ``2**-47 * max(|x|, |background|)``); while a stream warms up its
    foreground is its input (nothing is removed before there is evidence); idle slots and the hop before a ``restart`` are
    zero in every signal, whatever the chunk held there. ``last_emission(which, out=None)`` returns another signal of the
    samples the last ``push`` / ``finish`` emitted, until the next push, finish, restart or release.

    ``set_background_gain(gain, slots=None)`` keeps a share ``gain`` in [0, 1] of the background in the foreground of the named
    slots (None: all; a scalar, or one value per named slot): ``foreground = x - a * background`` with ``a = float32(1 -
    gain)``, rounded once in float64 by the same launch, wherever "foreground" is delivered ("both" and ``last_emission``
    included). 0 is the default and the plain foreground bit for bit, 1 returns the input (except where the background is NaN
    or infinite), -12 dB of background is ``10 ** (-12 / 20)``. A change is a fade: the next emission moves ``a`` linearly
    from the old value to the new one over its first ``min(step_length, n_emit)`` samples and is at the new value from there
    on. The gain is the slot's, not the stream's -- ``restart``, ``release``, ``finish_stream`` and ``import_stream`` leave it,
    and an exported state does not carry it --; ``background_gain(slot)`` reads it back. No host wait; a push in steady state
    costs the launches it always cost. ValueError for a value outside [0, 1] (NaN included) or a slot out of range.

    ``set_background_band_gains(gains, edges=None, slots=None)`` keeps a share of the background BAND BY BAND: ``gains`` in [0, 1],
    ``(n_bands,)`` for all named slots or ``(len(slots), n_bands)``, one per band of ``edges`` (``n_bands + 1`` ascending bin
    edges in ``[0, window_length / 2 + 1]``; ``repet.band_edges`` fits) or, with ``edges=None``, one per bin; a set replaces the
    slot's whole table and bins outside the edges get 0. The masked spectrum of every frame is multiplied by ``a[k] = float32(1
    - g[k])`` where the inverse STFT fetches it, into a second, shaped background, and the foreground is ``x - a_s *
    shaped_background`` with ``a_s`` the scalar gain above: the two multiply. The background, the mixture, ``last_frames``, the
    mixture's and background's levels and an exported state do not change by a bit; 1 on every bin returns the input. A frame is
    shaped, whole, with the table its slot had when the push (or finish) that completed it was made, so a change cross-fades
    through the analysis window over one frame, and the frame carried over from the push before keeps its own table; a set on
    a held slot applies from the frames after its ``resume``; a frame that arrives with ``import_stream`` takes the importing
    slot's table. The table is the slot's, like the scalar gain. ``background_band_gains(slot)`` returns the float32 ``(F,)``
    table last set (a host copy), ``clear_background_band_gains(slots=None)`` sets zeros. A set may come at any time: one
    small launch, no host wait, ``last_emission`` stays valid. A handle that never set a table costs what it always cost; while
    one is set a push enqueues one inverse-STFT launch more. Window lengths up to 4096 (sampling rates below about 100 kHz).

    ``last_levels(out=None)`` tells what the handle just did to every slot without pulling a signal to the host: for the
    samples the last ``push`` / ``finish`` emitted, per stream and channel the eight float64 values ``repet.LEVELS`` names --
    the sums of squares and the largest magnitudes of mixture, background and foreground (the float64 values of the emission
    itself, its gain and fade included, whatever ``which`` was), the live samples and the live samples whose mixture is NaN or
    infinite -- as ``(number_streams, number_channels, 8)``: a NumPy array, or a float64 tensor on the device (no host wait)
    when ``out`` is given or the last push was a device chunk. Samples that are not live (idle slots, the hop before a
    ``restart``) add nothing and are not counted; while a stream warms up its background energy is 0 and its foreground
    fields equal its mixture fields; energies are plain sums (NaN and inf propagate), peaks skip NaN. A background energy of 0
    says nothing repeating was found (bypass, or drive ``set_background_gain`` as a ducker); a peak above 1 clips in PCM.
    Reduced by one launch on demand (two for an emission longer than 4096 samples, none for an empty one: all zeros), in a
    fixed order: repeated calls return identical bits, and a push that nobody asks about costs what it always cost. After
    ``finish_stream`` it returns that tail's ``(number_channels, 8)`` -- the call measures its tail itself, since it drops the
    slot's samples, on a handle that ``last_levels`` has been called on before; ValueError otherwise, and once a push,
    finish, restart or release has followed.

    ``last_frames(which="foreground", bands=None, out=None)`` hands out what a push decided in the time-frequency plane, for the
    ``T`` frames the last ``push`` / ``finish`` completed (``last_frame_range`` is ``(first, T)``; frame ``k`` begins at pushed
    sample ``k * step_length``): the float32 magnitudes ``(number_streams, T, number_channels, window_length / 2 + 1)`` of the
    mixture (``|STFT|``, as the handle stored it), the background (the magnitude of the masked spectrum: equal to the mixture
    bit for bit on the high-pass bins ``1 .. cutoff_bins``) or the foreground (mixture - background, never negative) -- what a
    recogniser or a VAD would otherwise re-STFT the foreground for. With ``bands`` (``n_bands + 1`` ascending bin edges, at
    most 128 bands, e.g. :func:`band_edges`) the result is the float64 energy per band, ``(number_streams, T,
    number_channels, n_bands)``: a spectrum display or a per-band meter, summed on the device in a fixed order (identical bits
    from repeated calls). A NumPy array, or a tensor on the device (``out``, any strides for the frames, or a fresh one) when
    ``out`` is a tensor or the last push was a device chunk, then with no host wait. Idle and held slots and the frame that
    straddles a ``restart`` are zero, whatever the chunk carried; a warm-up frame has background 0 and foreground = mixture.
    One launch on demand: a push that nobody asks about costs what it always cost. ValueError once a push, finish,
    finish_stream, restart, release, import, hold or resume has followed (the frames of a ``finish_stream`` tail are not
    served). ``repet.online`` has the same calls without the stream axis.

    ``last_matches(out=None)`` reports the decision behind those spectra: which earlier frames of its stream's buffer each of
    the ``T`` frames resembles -- the frames its mask is the median of. A :class:`Matches` ``(count, age, similarity)``:
    ``count`` int32 ``(number_streams, T)``, the length of the frame's list (the frame itself included: its similarity with
    itself is 1); ``age`` int32 ``(number_streams, T, K)``, how many of the stream's own frames back each similar frame lies
    (0 the frame itself, 1 the frame before), strictly ascending, ``-1`` behind the list; ``similarity`` float32 of the same
    shape, the cosine similarity of the pair as the handle's peak picking read it, 0 behind the list. ``K`` is
    ``match_capacity``, ``min(similarity_number, ceil(buffer_frames / (similarity_distance_frames + 1)))``. Own frames are the
    stream's: a frame that passed while the slot was held does not exist for it, and an imported stream's ages go on from the
    exporting handle's. Idle and held slots, the frame that straddles a ``restart``, warm-up frames and a frame with a NaN
    sample have ``count`` 0. How many matches there are, how far apart and how alike says whether anything repeats: hold
    music shows as evenly spaced ages, a stationary noise does not. NumPy arrays, or tensors on the device, with no host wait,
    when ``out`` is a triple of dense tensors of these dtypes and shapes or the last push was a device chunk. One launch on
    demand, valid exactly where ``last_frames`` is; ``repet.online`` has the same without the stream axis.

    A stream can move between handles: ``export_stream(slot, device=False)`` returns a snapshot of the slot's state as a
    :class:`StreamState` -- ``header``, a small ``bytes`` value the host knows at once, and ``payload``, a ``numpy.uint8``
    array or (``device=True``, no host wait) a ``torch.uint8`` tensor on the handle's device, ``stream_state_nbytes`` bytes
    -- and ``import_stream(slot, state)`` loads it into any slot of any handle opened with the same parameters, on this GPU,
    another one (a tensor on another device is copied over first) or, through ``state.to_bytes()`` /
    ``StreamState.from_bytes(b)``, another process or a later day. The exporting slot lives on untouched, so migration is
    ``export_stream`` + ``release``, and a snapshot imported twice is a fork. Both calls need ``samples_pushed`` on the hop
    grid; ``import_stream`` drops what lived in the slot, as ``restart`` does, and raises ValueError before anything runs
    for a state of another sampling frequency, channel count or parameter set, a payload of the wrong size or dtype, or an
    unknown magic word or version. What the exporting slot emitted before the export, then what the importing slot emits
    in lockstep, then its ``finish_stream`` / ``finish`` tail, equal ``simonline`` of the stream's whole input bit for bit
    -- on a handle of any age, other live slots undisturbed; the foreground's delay line moves with the stream. (A handle
    on which nothing was pushed holds no sample yet, the state one hop that was never emitted: the first push after such
    an import emits that hop, which is a hop of zeros in front of every other slot's own output.)

    A stream can sit out pushes -- silence suppression, a lost or late packet, a caller whose clock lags: ``hold(slots)`` holds
    live slots from the handle's current sample on and ``resume(slots)`` lets them go on (``held(slot)`` tells). While a slot
    is held, time does not pass for its stream: its share of every chunk is ignored, NaN and inf included; its share of every
    emitted signal -- background, foreground, mixture, both of "both", every dtype -- is zero; ``last_levels`` counts nothing
    for it; and its similarity buffer, its overlap-add tail and its held samples stay as they are while the other slots'
    slide. Per slot, the output pieces of the pushes during which it was not held, in order, then its ``finish_stream`` /
    ``finish`` tail, equal ``simonline`` of the input pieces of those same pushes, bit for bit, whatever the other slots do
    and whatever the held chunks carried. The output runs one hop behind the input, so the hop that belongs to the last
    input before a hold comes out of the first push after the resume; nothing is emitted twice or dropped, and
    ``stream_samples(slot)`` counts only what the stream itself was fed. Both calls need ``samples_pushed`` on the hop grid,
    and while any slot is held a push must be a whole number of hops (ValueError before anything runs, nothing changes).
    ValueError for an idle slot or a slot out of range; holding a held slot or resuming one that is not held does nothing.
    ``restart``, ``release``, ``import_stream`` and ``finish_stream`` on a held slot do what they always do and end the hold;
    ``finish`` ends held slots like the others; ``export_stream`` of a held slot returns the stream as it stands. Both make
    ``last_emission`` / ``last_levels`` stale, as ``restart`` does. A gain set during a hold is in force, its fade elapsed
    unheard, at the resume. One small launch each, no host wait; a handle with no slot held pushes at the launches it always
    cost, and so does a push with held slots (``repet.online``, one stream, needs neither: not pushing is its hold).

    Slots can be fed at their own pace -- packets of 10, 20 or 30 ms that never match the hop, with jitter, bursts and gaps.
    ``enable_feed(capacity_samples)`` (once, on the hop grid; ``feed_capacity``) gives every slot an inbox of that many samples
    per channel in device memory (``S * capacity * C * 8`` bytes), held as the handle holds samples, so that what reaches the
    stream is bit for bit what a push of the same values would have written. ``feed(slots, chunk, counts=None)`` appends to
    the inboxes of live slots: one slot takes ``(n, C)``, several ``(len(slots), n, C)`` with an optional ``counts[i] <= n``
    per row, behind which nothing is read; host arrays or ROCm tensors of any ingest dtype and stride, all or nothing
    (ValueError, nothing changed, for a slot out of range, named twice or idle, a bad count, an overflow, a handle without
    inboxes or finished), no host wait on the device path, and the packet may be overwritten afterwards. ``tick(hops=1)`` is
    the lockstep push of ``hops`` hops that the handle assembles itself: the live slots that are not held and have that much
    queued (``queued(slot=None)``) are consumed, oldest samples first; the other live slots that are not held are *starved*,
    which is ``hold`` for the length of that push, written to the device only when a slot's state changes. So the guarantee
    is ``hold``'s: per slot, the pieces of the ticks that consumed it, then its tail, equal ``simonline`` of the samples it
    consumed, bit for bit, in whatever packets they came and whatever the others did. ``tick`` returns what ``push``
    returns (``out``, ``which``, ``dtype``; a tensor when ``out`` is one or the last ``feed`` was a device tensor), or None,
    with nothing run and every record as it was, when nobody is ready; ``last_consumed`` is the bool ``(S,)`` of who took
    part. ``pad_feed(slots=None)`` zero-pads queues to the hop grid and returns the pad counts: after the ticks that drain
    the queue ``finish_stream(slot)[:-pad]`` is a stream's true tail. ``clear_feed(slots=None)`` empties inboxes, and so do
    ``restart``, ``release`` and ``import_stream`` for their slots; ``finish_stream`` / ``finish`` refuse while a slot they end
    has queued samples; a plain ``push`` is refused while any inbox holds samples and otherwise resumes the starved slots
    first; ``held`` reports the caller's holds only; ``export_stream`` returns the stream as consumed; ``stream_samples``
    counts consumed samples (``repet.online``, one stream, needs none of this: its ``push`` takes any ``n``).

    ``start_length`` (seconds; None: ``buffer_length``, the reference) lets every slot separate before its 10-s buffer has
    filled, from its own frame ``start_frames - 1`` on (see :func:`online`; the ``start_frames`` property), after every
    ``restart`` too: each life then equals the one-stream handle's output with the same ``start_length``, a stream of
    ``(start_frames - 2) * step_length + window_length`` samples can be finished, and a push costs the launches it always
    cost. While a young frame's number is at most ``similarity_distance`` (in frames) its only similar frame is itself: the
    mask is 1, the whole input counts as background and the foreground is silent, so a sensible ``start_length`` is at least
    two or three times ``similarity_distance``; below ``start_length`` the foreground is still the input. The value belongs
    to the handle, not to a stream: an imported stream goes on under the importing handle's.

    ``silent_frames`` ("reference", the default, or "zero"; the ``silent_frames`` property): what every slot makes of whole
    frames of digital silence, see :func:`online`. Under "zero" a muted slot emits a finite background and foreground,
    ``last_levels`` stays finite, ``last_frames`` and the background shaped by band gains are 0 on the silent frames,
    ``last_matches`` reports count 0 there, and the mute does not keep the frames around it out of the other frames' lists;
    ``hold``, ``feed`` / ``tick``, ``restart``, ``export_stream`` / ``import_stream`` and ``start_length`` work as they do
    without it, at the same launches per push. A stream moves only between handles opened with the same rule."""
    params = derive_params(sampling_frequency)
    params.flags |= _native.silent_frames_flag(silent_frames)
    return _native.OnlineStreams(params, number_channels, number_streams, _device, max_push_samples or 0,
                                 _native.start_frames_for(params, sampling_frequency, start_length))


def band_edges(sampling_frequency, number_bands, f_min=0.0, f_max=None):
    """Bin edges for ``last_frames(bands=...)`` of a live handle at ``sampling_frequency``: ``number_bands + 1`` ascending
    integers from ``round(f_min * W / fs)`` to ``round(f_max * W / fs) + 1`` (``W`` the window length; ``f_max`` None: ``fs /
    2``, so that the defaults cover every bin), equally spaced on the mel scale ``2595 * log10(1 + f / 700)``, rounded to bins
    and forced non-decreasing (at low frequencies neighbouring edges may coincide: an empty band, energy 0). A convenience,
    nothing more: any ascending edges will do."""
    fs = float(sampling_frequency)
    n = int(number_bands)
    if n < 1:
        raise ValueError("at least one band")
    f_max = fs / 2 if f_max is None else float(f_max)
    f_min = float(f_min)
    if not 0 <= f_min <= f_max <= fs / 2:
        raise ValueError("0 <= f_min <= f_max <= sampling_frequency / 2")
    w = _window_length(sampling_frequency)
    lo, hi = int(round(f_min * w / fs)), int(round(f_max * w / fs)) + 1
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    f = 700.0 * (10.0 ** (np.linspace(mel(lo * fs / w), mel(hi * fs / w), n + 1) / 2595.0) - 1.0)
    edges = np.clip(np.round(f * w / fs).astype(np.int64), lo, hi)
    edges[0], edges[-1] = lo, hi
    return [int(e) for e in np.maximum.accumulate(edges)]


def run_batch(algo, audio_signals, sampling_frequency, n_devices=1, transport="host", device=None, depth=None):
    """Separate a list of independent clips, dealt longest-first over ``n_devices`` GPUs of this process. ``transport``:
    "host" -- every device moves its own clips over its own PCIe link; "rccl" -- the clips enter through device 0 and
    travel to their devices (and the results back) as grouped ncclSend / ncclRecv over xGMI. ``device`` / ``depth``: the clips
    one after another through that ONE device with ``depth`` (default 2) of them in flight -- upload, kernels and download of
    neighbouring clips side by side (``repet_run_stream``); every result is what the one-shot call returns, bit for bit."""
    import ctypes as C
    params = derive_params(sampling_frequency)
    ins, outs, ns, cs, code = [], [], [], [], None
    for a in audio_signals:
        n, c = np.shape(a)
        arr, k = _native.as_input(a)
        if code is None:
            code = k
        elif k != code:
            arr, k = np.ascontiguousarray(arr, dtype=np.float64), _native.F64
            if code != _native.F64:
                ins = [np.ascontiguousarray(x, dtype=np.float64) for x in ins]
                code = _native.F64
        ins.append(arr)
        outs.append(np.empty((n, c), dtype=np.float64))
        ns.append(n)
        cs.append(c)
    count = len(ins)
    in_ptrs = (C.c_void_p * count)(*[x.ctypes.data for x in ins])
    out_ptrs = (C.c_void_p * count)(*[x.ctypes.data for x in outs])
    if device is not None or depth is not None:
        _native.check(_native.lib().repet_run_stream(
            _native.ALGO_IDS[algo], count, in_ptrs, code if code is not None else _native.F64,
            (C.c_int64 * count)(*ns), (C.c_int32 * count)(*cs), params, out_ptrs, int(_device if device is None else device),
            int(2 if depth is None else depth)))
        return outs
    entry = _native.lib().repet_run_batch_rccl if transport == "rccl" else _native.lib().repet_run_batch
    _native.check(entry(
        _native.ALGO_IDS[algo], count, in_ptrs, code if code is not None else _native.F64,
        (C.c_int64 * count)(*ns), (C.c_int32 * count)(*cs), params, out_ptrs, int(n_devices)))
    return outs


def last_batch_info():
    """What this thread's last ``run_batch`` did: transport, clips that went through send / receive, clips whose fp32
    remainder plane was resident when they were separated, RCCL groups completed."""
    import ctypes as C
    out = (C.c_int64 * 4)()
    _native.check(_native.lib().repet_last_batch_info(out))
    return {"transport": "rccl" if out[0] == 1 else "host", "clips_sent": int(out[1]), "clips_with_remainders": int(out[2]), "rccl_groups": int(out[3])}


# ---- private helpers of the reference, kept callable (README.md:79 uses repet._stft) -----------------------
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _stft(audio_signal, window_function, step_length):
    """STFT of one channel, ``(window_length, number_frames)`` complex with all bins (repet.py:1001-1060)."""
    x = _f32(audio_signal)
    window = _f32(window_function)
    w = len(window)
    lib = _native.lib()
    t = lib.repet_frame_count(len(x), w, int(step_length), 1)
    f = w // 2 + 1
    spec = np.empty((t, f, 2), dtype=np.float32)
    _native.check(lib.repet_stft(_native.default_context(_device).handle, _native.ptr(x), len(x),
                                 _native.ptr(window), w, int(step_length), 1, _native.ptr(spec), t))
    half = (spec[..., 0] + 1j * spec[..., 1]).astype(complex).T          # (F, T)
    return np.concatenate((half, np.conj(half[-2:0:-1])), axis=0)


def _istft(audio_stft, window_function, step_length):
    """Inverse STFT by overlap-add (repet.py:1063-1105); the mirrored bins are implied by the first half."""
    window = _f32(window_function)
    w, t = np.shape(audio_stft)
    f = w // 2 + 1
    half = np.ascontiguousarray(np.asarray(audio_stft)[:f].T)
    spec = np.empty((t, f, 2), dtype=np.float32)
    spec[..., 0] = half.real
    spec[..., 1] = half.imag
    n_out = t * int(step_length) - (w - int(step_length))
    y = np.empty(n_out, dtype=np.float32)
    _native.check(_native.lib().repet_istft(_native.default_context(_device).handle, _native.ptr(spec), t,
                                            _native.ptr(window), w, int(step_length), _native.ptr(y), n_out))
    return y.astype(np.float64)


# ---- stage entries of the production FFT launchers (diagnostic exports, not part of the C ABI) ------------------------
FFT_PATHS = {"auto": 0, "block": 1, "wave": 2, "reg": 3}
_FFT_FAMILIES = {0: None, 1: "block", 2: "wave", 3: "reg"}
_stage_entries = {}


def _stage_entry(name):
    import ctypes as C
    if name not in _stage_entries:
        fn = getattr(_native.lib(), name)
        p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        fn.restype = C.c_int
        fn.argtypes = {
            "repet_debug_stft_stage": [p, p, i64, i32, p, i32, i32, i32, i64, i64, i32, i64, i32, i32, i32, i32, p] + [p] * 8 + [p, i32, p],
            "repet_debug_istft_stage": [p, p, i32, i32, i64, i32, i64, i64, i64, C.c_float, p, p, p, i32, i32, i32, i64, i64,
                                        i32, i32, i32, i32, i32, i64, i64, i32, p, i64, p, i32, p],
            "repet_debug_gram_band_stage": [p, p, i32, i64, i32, i32, i64, i32, i32, i32, i32, i32, p, p, p, p, p, i32],
            "repet_debug_band_periods_stage": [p, p, i32, i64, i32, i32, i32, i64, i64, i64, i32, i32, i32, i32, i64, i32, p, p, p],
            "repet_debug_mask_stage": [p, i32, p, p, i32, i32, i64, i32, i32, i32, i32, i32, p, i32, i32, p, p, i64, i32, i64, i32, i64, i64,
                                       i32, p, i64, i32, i32, p, p, p, p, p, p, i32, p, i32, p],
            "repet_debug_peaks_stage": [p, p, i32, i64, i32, i64, p, i64, i32, p, p, i64, i32, i32, i64, i32, i64, i64, C.c_double, i32, i32,
                                        i64, p, i32, i32, i32, i32, p, p, p, p, p, p, p, i32, p],
            "repet_debug_devio_stage": [p, i32, i32, p, p, p, p, i32, p, i32, p, i32, p],
        }[name]
        _stage_entries[name] = fn
    return _stage_entries[name]


def _launch_report(name_buf, words):
    return {"kernel": name_buf.value.decode(), "family": _FFT_FAMILIES[int(words[0])], "run": int(words[1]), "rounds": int(words[2]),
            "slots": int(words[3]), "workgroups": int(words[4]), "units": int(words[5]), "launches": int(words[6])}


def _stft_stage(audio, window_function, step_length, centred=True, sample_offset=0, n_samples=None, n_batch=1,
                batch_sample_stride=0, path="auto", want=(), fix_infinite=False, prefill=0):
    """``launch_stft`` as the pipelines call it. ``audio`` (n_total, C) fp32 interleaved; ``n_batch`` clips of ``n_samples``
    samples, the first at ``sample_offset``, ``batch_sample_stride`` apart. ``want``: any of "Vm", "Vn", "P", "Vh", "Ph"
    ("Ph" brings "Ph_inv"). Returns a dict of the buffers exactly as the kernel left them -- X (B, C, rows, FS) complex64 and
    V with the pad bins and pad rows, the means (B, Tpad, FS), the f16 planes (B, Tpad, 2 FS) as float16 -- every one filled
    with the byte ``prefill`` before the launch, plus "T", "F", "FS", "Tpad" and "launch": the kernel that ran, its family,
    the frames per workgroup and the resident slots they were fitted to. A family that does not take the shape raises
    RuntimeError (REPET_ERR_LIMIT)."""
    import ctypes as C
    x = _f32(audio)
    if x.ndim == 1:
        x = x[:, None]
    window = _f32(window_function)
    n_total, ch = x.shape
    n = n_total - sample_offset if n_samples is None else n_samples
    bits = sum({"Vm": 1, "Vn": 2, "P": 4, "Vh": 8, "Ph": 16}[k] for k in want)
    geo = (C.c_int64 * 6)()
    words = (C.c_int64 * 8)()
    name = C.create_string_buffer(64)
    fn = _stage_entry("repet_debug_stft_stage")
    ctx = _native.default_context(_device).handle

    def call(outs):
        _native.check(fn(ctx, _native.ptr(x), n_total, ch, _native.ptr(window), len(window), int(step_length), int(bool(centred)),
                         int(sample_offset), int(n), int(n_batch), int(batch_sample_stride), FFT_PATHS[path], bits,
                         int(bool(fix_infinite)), int(prefill), geo, *outs, name, len(name), words))

    call([None] * 8)
    t, tpad, rows, f, fs, _ = (int(v) for v in geo)
    b = int(n_batch)
    X = np.empty((b, ch, rows, fs), dtype=np.complex64)
    V = np.empty((b, ch, rows, fs), dtype=np.float32)
    means = {k: np.empty((b, tpad, fs), dtype=np.float32) for k in ("Vm", "Vn", "P") if k in want}
    planes = {k: np.empty((b, tpad, 2 * fs), dtype=np.float16) for k in ("Vh", "Ph") if k in want}
    ph_inv = np.empty((b, tpad), dtype=np.float32) if "Ph" in want else None
    opt = lambda a: None if a is None else _native.ptr(a)
    call([_native.ptr(X), _native.ptr(V), opt(means.get("Vm")), opt(means.get("Vn")), opt(means.get("P")), opt(planes.get("Vh")),
          opt(planes.get("Ph")), opt(ph_inv)])
    out = {"X": X, "V": V, "T": t, "F": f, "FS": fs, "Tpad": tpad, "launch": _launch_report(name, words)}
    out.update(means)
    out.update(planes)
    if ph_inv is not None:
        out["Ph_inv"] = ph_inv
    return out


def _istft_stage(spectra, window_length, out, trim, n_out, out_offset=0, scale=1.0, mask=None, model=None, periods=None, cutoff=0,
                 accumulate_weighted=0, fade_in=0, fade_out=0, batch=None, path="auto"):
    """``launch_istft_ola`` as the pipelines call it. ``spectra`` (n_spec, C, T, F) complex half spectra; ``out`` (out_len, C)
    the pre-filled output buffer, returned whole as the kernel left it (the argument is not changed). ``mask`` (n_spec, C, T, F)
    or ``model`` (n_spec, C, rows, F) + ``periods`` (n_spec,) + ``cutoff``. ``batch``: dict of n_batch, batch_first, batch_step,
    batch_total, batch_local0, batch_out_stride, overlap. Returns (out, launch report)."""
    import ctypes as C
    y = np.ascontiguousarray(spectra, dtype=np.complex64)
    n_spec, ch, t, f = y.shape
    assert f == window_length // 2 + 1
    buf = np.array(out, dtype=np.float32, order="C", copy=True)
    if buf.ndim == 1:
        buf = buf[:, None]
    assert buf.shape[1] == ch
    m = None if mask is None else _f32(mask)
    w = None if model is None else _f32(model)
    per = None if periods is None else np.ascontiguousarray(periods, dtype=np.int32)
    assert m is None or m.shape == y.shape
    assert w is None or (w.shape[:2] == (n_spec, ch) and w.shape[3] == f and per is not None and per.shape == (n_spec,))
    bt = dict(n_batch=0, batch_first=0, batch_step=0, batch_total=0, batch_local0=0, batch_out_stride=0, overlap=0)
    bt.update(batch or {})
    words = (C.c_int64 * 8)()
    name = C.create_string_buffer(64)
    opt = lambda a: None if a is None else _native.ptr(a)
    _native.check(_stage_entry("repet_debug_istft_stage")(
        _native.default_context(_device).handle, _native.ptr(y), n_spec, ch, t, int(window_length), int(trim), int(n_out), int(out_offset),
        float(scale), opt(m), opt(w), opt(per), 0 if w is None else w.shape[2], int(cutoff), int(accumulate_weighted), int(fade_in),
        int(fade_out), int(bt["n_batch"]), int(bt["batch_first"]), int(bt["batch_step"]), int(bt["batch_total"]), int(bt["batch_local0"]),
        int(bt["batch_out_stride"]), int(bt["overlap"]), FFT_PATHS[path], _native.ptr(buf), buf.shape[0], name, len(name), words))
    return buf, _launch_report(name, words)


GRAM_BAND_FORMS = {"auto": 0, "f32": 1, "f16_rows": 2, "f16_unit": 3, "f16_unit_lookback": 4}
_GRAM_BAND_FORM_NAMES = {v: k for k, v in GRAM_BAND_FORMS.items()}


def _gram_band_stage(rows, n_lags, clip_stride=None, form="auto", unit_rows=False, lookback=False, planes_ready=False, prefill=0,
                     choice_only=False):
    """The banded Gram as the pipelines run it (``exec_gram_band``, the second half of ``run_gram_band``). ``rows`` (B, T, F) or
    (T, F) fp32; ``clip_stride`` in rows, at least round_up(T, 128) (the default). ``form``: "auto" (what ``gram_band_form``
    picks from ``unit_rows`` / ``lookback`` / ``planes_ready``), "f32", "f16_rows", "f16_unit", "f16_unit_lookback". Returns a
    dict: "band" (B, clip_stride, LP) exactly as the kernel left it over the byte ``prefill``; for the f16 forms "planes"
    (B, Tpad, 2 FS) float16, for "f16_rows" also "inv" (B, Tpad); "form" (the one that ran), "band_on_f16", "band_lookback",
    "kernel", "n_tiles", "Tpad", "FS", "LP". ``choice_only``: nothing runs, only "form" (what would run) and the sizes come back;
    ``rows`` may then be a (B, T, F) shape."""
    import ctypes as C
    if choice_only and isinstance(rows, tuple):
        x, (b, t, f) = None, rows
    else:
        x = _f32(rows)
        if x.ndim == 2:
            x = x[None]
        b, t, f = x.shape
    tpad = -(-t // 128) * 128
    stride = tpad if clip_stride is None else int(clip_stride)
    geo = (C.c_int64 * 8)()
    name = C.create_string_buffer(64)
    fn = _stage_entry("repet_debug_gram_band_stage")
    ctx = _native.default_context(_device).handle

    def call(band, planes, inv):
        opt = lambda a: None if a is None else _native.ptr(a)
        _native.check(fn(ctx, opt(x), b, t, f, int(n_lags), stride, GRAM_BAND_FORMS[form], int(bool(unit_rows)), int(bool(lookback)),
                         int(bool(planes_ready)), int(prefill), geo, opt(band), opt(planes), opt(inv), name, len(name)))

    call(None, None, None)
    _, fs, lp, ran = (int(v) for v in geo[:4])
    out = {"form": _GRAM_BAND_FORM_NAMES[ran], "Tpad": tpad, "FS": fs, "LP": lp, "n_tiles": int(geo[6])}
    if choice_only:
        return out
    band = np.empty((b, stride, lp), dtype=np.float32)
    planes = np.empty((b, tpad, 2 * fs), dtype=np.float16) if ran != 1 else None
    inv = np.empty((b, tpad), dtype=np.float32) if ran == 2 else None
    call(band, planes, inv)
    out.update(band=band, form=_GRAM_BAND_FORM_NAMES[int(geo[3])], band_on_f16=bool(geo[4]), band_lookback=bool(geo[5]),
               kernel=name.value.decode())
    if planes is not None:
        out["planes"] = planes
    if inv is not None:
        out["inv"] = inv
    return out


GRAM_FULL_FORMS = {"auto": 0, "f32": 1, "f16_128": 2, "f16_256": 3}
_GRAM_FULL_FORM_NAMES = {v: k for k, v in GRAM_FULL_FORMS.items()}
_GRAM_RECORD_SOURCES = {0: None, 1: "epilogue", 2: "pass"}


def _gram_full_stage(rows, form="auto", records=0, normalise=False, prefill=0, choice_only=False):
    """The similarity matrix of ``sim`` as the pipeline runs it (``exec_gram_full``, the second half of ``run_gram_full``;
    ``repet_debug_gram_full_stage``). ``rows`` (T, F) fp32, taken as unit rows as they are; ``normalise``: made unit rows on the
    device first ("Vn" (Tpad, FS) brings them back). ``form``: "auto" (what ``gram_full_form`` picks for T), "f32", "f16_128",
    "f16_256" (both at any T). ``records``: 0 none, 1 as ``sim`` gets them (the epilogue of "f16_256", a pass over S otherwise),
    2 always by the pass over S. Returns a dict: "S" (T, TS) the whole pitched image as the kernel left it over the byte
    ``prefill``; with records "top", "second" (float32) and "at" (int32), each (T, seg_pitch); for the f16 forms "planes"
    (round_up(T, tile), 2 FS) float16; "form" (the one that ran), "records" (None, "epilogue" or "pass"), "kernel", "n_tiles",
    "tile", "Tpad", "FS", "TS", "seg_pitch". ``choice_only``: nothing runs, only what would and the sizes come back; ``rows`` may
    then be a (T, F) shape."""
    import ctypes as C
    if choice_only and isinstance(rows, tuple):
        x, (t, f) = None, rows
    else:
        x = _f32(rows)
        t, f = x.shape
    geo = (C.c_int64 * 8)()
    name = C.create_string_buffer(64)
    fn = _native.lib().repet_debug_gram_full_stage
    ctx = _native.default_context(_device).handle
    opt = lambda a: None if a is None else _native.ptr(a)

    def call(s, top, second, at, planes, vn):
        _native.check(fn(ctx, opt(x), t, f, GRAM_FULL_FORMS.get(form, form), int(records), int(bool(normalise)), int(prefill), geo, opt(s), opt(top),
                         opt(second), opt(at), opt(planes), opt(vn), name, len(name)))

    call(None, None, None, None, None, None)
    tpad, fs, ts, seg_pitch, ran, source, n_tiles, tile = (int(v) for v in geo)
    out = {"form": _GRAM_FULL_FORM_NAMES[ran], "records": _GRAM_RECORD_SOURCES[source], "n_tiles": n_tiles, "tile": tile, "Tpad": tpad,
           "FS": fs, "TS": ts, "seg_pitch": seg_pitch}
    if choice_only:
        return out
    s = np.empty((t, ts), dtype=np.float32)
    top, second = (np.empty((t, seg_pitch), dtype=np.float32) for _ in range(2)) if records else (None, None)
    at = np.empty((t, seg_pitch), dtype=np.int32) if records else None
    planes = np.empty((-(-t // tile) * tile, 2 * fs), dtype=np.float16) if ran != 1 else None
    vn = np.empty((tpad, fs), dtype=np.float32) if normalise else None
    call(s, top, second, at, planes, vn)
    out.update(S=s, kernel=name.value.decode())
    for key, value in (("top", top), ("second", second), ("at", at), ("planes", planes), ("Vn", vn)):
        if value is not None:
            out[key] = value
    return out


def _band_periods_stage(band, n_freq, start0, step, length, n_windows, lo, hi, n_lags_for_clamp, n_lags=None, t_expand=0, prefill=0):
    """``run_band_window_sum`` -> ``launch_periods`` -> (``t_expand`` > 0) ``launch_expand_periods`` on a band (B, T, LP) or
    (T, LP) fp32, LP a multiple of 64 (``n_lags`` defaults to LP): window w covers frames [start0 + w step, + length). Returns
    (beat rows (B, n_windows, LP) over the byte ``prefill``, window periods (B, n_windows), frame periods (t_expand,) of the first
    clip or None)."""
    x = _f32(band)
    if x.ndim == 2:
        x = x[None]
    b, t, lp = x.shape
    beat = np.empty((b, int(n_windows), lp), dtype=np.float32)
    win = np.empty((b, int(n_windows)), dtype=np.int32)
    frames = np.empty(int(t_expand), dtype=np.int32) if t_expand else None
    _native.check(_stage_entry("repet_debug_band_periods_stage")(
        _native.default_context(_device).handle, _native.ptr(x), b, t, lp, lp if n_lags is None else int(n_lags), int(n_freq), int(start0),
        int(step), int(length), int(n_windows), int(lo), int(hi), int(n_lags_for_clamp), int(t_expand), int(prefill), _native.ptr(beat),
        _native.ptr(win), None if frames is None else _native.ptr(frames)))
    return beat, win, frames


MASK_KINDS = {"period": 0, "adaptive": 1, "sim": 2}
MEDIAN_PATHS = {"float": 0, "rank": 1, "bits": 2, "bits+nyquist": 3}


def _mask_stage(kind, V, X=None, want=("mask",), cutoff=0, prefill=0, period=None, periods=None, min_period=1, order=1, idx=None,
                cnt=None, first_frame=0, max_count=None, frame0=0, frame_end=0, parts=3, slot_start=None, slot_bias=0, idx_pitch=None,
                median_path="float"):
    """One of ``launch_mask_period`` / ``launch_mask_adaptive`` / ``launch_mask_sim`` as the pipelines call them, on buffers laid
    out as ``make_geo`` lays them out (``repet_debug_mask_stage``). ``V`` (B, C, T, F) fp32, ``X`` (B, C, T, F) complex64 or None.
    ``want``: any of "mask", "X" -- or "model" alone (period). ``kind`` "period": ``period`` (host) or ``periods`` (B,) device
    periods + ``min_period``; "adaptive": ``periods`` (T,) + ``order``; "sim": ``idx`` (B, rows, width), ``cnt`` (B, rows),
    ``first_frame``, ``max_count`` (default width), ``frame0``, ``frame_end`` (0: T), ``parts`` 1 main bins / 2 Nyquist bin / 3 both,
    ``slot_start`` (B,) + ``slot_bias``, ``idx_pitch`` (default max(width, 128)), ``median_path`` "float" / "rank" / "bits" /
    "bits+nyquist" (the bit-sliced path with the Nyquist bin in the ranked column of bin 1, as ``exec_sim`` runs it: ``cutoff`` >= 1,
    ``parts`` 1).
    Returns a dict: "mask" (B, C, rows, FS), "X" (B, C, rows, FS) complex64, "model" (B, C, T // 3 + 2, FS), "codes" (C, rows, FS)
    uint32 (bit-sliced path) -- each whole, as the kernel left it over the byte ``prefill`` --, "Tpad", "rows", "FS" and "launch":
    the kernel of the main bins ("kernel", e.g. "mask_sim_kernel<10, true>", with "name", "net", "flag", "parts", "grid"), of the
    Nyquist bin ("nyquist", "nyquist_net", "nyquist_preload", "nyquist_grid") and "lookups" (mask_from_codes_kernel ran). Input
    that would index out of range raises ValueError; a shape the median path does not take RuntimeError."""
    import ctypes as C
    v = _f32(V)
    assert v.ndim == 4
    b, ch, t, f = v.shape
    x = None if X is None else np.ascontiguousarray(X, dtype=np.complex64)
    assert x is None or x.shape == v.shape
    bits = sum({"mask": 1, "X": 2, "model": 4}[k] for k in want)
    fs, tpad = -(-f // 32) * 32, -(-t // 128) * 128
    rows_all, model_rows = tpad + 8, t // 3 + 2
    per = None if periods is None else np.ascontiguousarray(periods, dtype=np.int32)
    if kind == "period":
        assert (per is None) != (period is None) and (per is None or per.shape == (b,))
    elif kind == "adaptive":
        assert per is not None and per.shape == (t,)
    ix = nn = ss = None
    n_list_rows = width = 0
    if kind == "sim":
        ix, nn = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(cnt, dtype=np.int32)
        assert ix.ndim == 3 and ix.shape[0] == b and nn.shape == ix.shape[:2]
        n_list_rows, width = ix.shape[1:]
        max_count = width if max_count is None else max_count
        idx_pitch = max(width, 128) if idx_pitch is None else idx_pitch
        if slot_start is not None:
            ss = np.ascontiguousarray(slot_start, dtype=np.int64)
            assert ss.shape == (b,)
    mask = np.empty((b, ch, rows_all, fs), dtype=np.float32) if bits & 1 else None
    xo = np.empty((b, ch, rows_all, fs), dtype=np.complex64) if bits & 2 else None
    model = np.empty((b, ch, model_rows, fs), dtype=np.float32) if bits & 4 else None
    codes = np.empty((ch, rows_all, fs), dtype=np.uint32) if kind == "sim" and median_path in ("bits", "bits+nyquist") else None
    geo, words = (C.c_int64 * 8)(), (C.c_int64 * 16)()
    name, nyq = C.create_string_buffer(64), C.create_string_buffer(64)
    opt = lambda a: None if a is None else _native.ptr(a)
    _native.check(_stage_entry("repet_debug_mask_stage")(
        _native.default_context(_device).handle, MASK_KINDS[kind], _native.ptr(v), opt(x), b, ch, t, f, int(cutoff), int(prefill), bits,
        int(period or 0), opt(per), int(min_period), int(order), opt(ix), opt(nn), n_list_rows, width, int(first_frame), int(max_count or 0),
        int(frame0), int(frame_end), int(parts), opt(ss), int(slot_bias), int(idx_pitch or 0), MEDIAN_PATHS[median_path], geo, opt(mask),
        opt(xo), opt(model), opt(codes), name, len(name), nyq, len(nyq), words))
    assert (int(geo[0]), int(geo[1]), int(geo[2]), int(geo[4])) == (tpad, rows_all, fs, model_rows)
    w = [int(k) for k in words]
    main = name.value.decode()
    if main == "mask_sim_kernel":
        full = "%s<%d, %s>" % (main, w[0], "true" if w[1] else "false")
    elif main == "mask_sim_bits_kernel":
        full = "%s<%d, %d>" % (main, w[0], w[1])
    else:
        full = "%s<%d>" % (main, w[0]) if main else ""
    nyquist = "%s<%d, %s>" % (nyq.value.decode(), w[6], "true" if w[7] else "false") if nyq.value else ""
    out = {"Tpad": tpad, "rows": rows_all, "FS": fs,
           "launch": {"kernel": full, "name": main, "net": w[0], "flag": w[1], "parts": w[2], "grid": tuple(w[3:6]), "nyquist": nyquist,
                      "nyquist_net": w[6], "nyquist_preload": bool(w[7]), "nyquist_grid": tuple(w[8:11]), "lookups": bool(w[11])}}
    for key, a in (("mask", mask), ("X", xo), ("model", model), ("codes", codes)):
        if a is not None:
            out[key] = a
    return out


PEAK_REFINE_STATS = ("rows_refined", "near_tied", "decisions_changed", "flat_rows", "rows_to_level2", "level2_cursor", "elements_level2",
                     "rows_changed_level2", "level2_max_diff_1e12", "unit_rows_f64", "frames_queued", "queue_cursor", "rows_recorded",
                     "record_cursor", "rows_handed_on")


def _peaks_stage(M, n_cols=None, pitch=None, mode=0, row0=0, n_rows=None, min_value=0.0, d=1, number=1, shift=0, origin=None, start=0,
                 with_scratch=False, refine=0, unit=None, hi=None, lo=None, W=0, frame_sample0=0, prefill=0):
    """The peak picking as ``exec_sim``, ``exec_simonline`` and the live handles run it (``repet_debug_peaks_stage``):
    ``launch_segment_maxima`` where the launcher will use the records, ``make_refine``, ``launch_local_maxima`` and -- ``refine`` 2
    -- ``run_exact_rows``. ``M`` (n_batch, m_rows, n_cols) or (m_rows, n_cols) fp32: matrix rows (mode 0) or the band (modes 1, 2),
    copied to rows of ``pitch`` floats (default round_up(n_cols, 64)). ``unit`` (n_batch, n_frames, F) fp32 unit rows (``refine``
    >= 1), ``hi`` / ``lo`` (n_batch, n_samples, C) fp32 audio with ``W`` and ``frame_sample0`` (``refine`` 2). ``origin`` (n_batch,)
    int64 or None and ``start``: ``PeakBatch``. Returns a dict: "idx" (n_batch, n_rows + 1, KP) and "count" (n_batch, n_rows + 1)
    whole, as the kernels left them over the byte ``prefill`` (the last row of every clip belongs to no launch), "KP", "stats" (the
    32 counters) and "counters" (the named ones), "delta", "delta2", "u64" (n_batch, n_frames, FS) float64 and "stamped" (n_batch,
    n_frames) bool (``refine`` 2), and "launch": "family" ("wave", "wave+records", "block", "block two-stage"), "qmax", "rd",
    "unit_rows_variant" (0: not launched), "lite", "exact_fft" (0: the general kernel was not launched). Input that would index
    out of range raises ValueError."""
    import ctypes as C
    m = _f32(M)
    if m.ndim == 2:
        m = m[None]
    nb, m_rows, cols = m.shape
    assert n_cols is None or n_cols == cols
    pitch = -(-cols // 64) * 64 if pitch is None else int(pitch)
    n_rows = m_rows - row0 if n_rows is None else int(n_rows)
    u = h = l = org = None
    n_frames = f = n_samples = ch = 0
    if refine:
        u = _f32(unit)
        if u.ndim == 2:
            u = u[None]
        assert u.ndim == 3 and u.shape[0] == nb
        n_frames, f = u.shape[1:]
    if refine == 2:
        h = _f32(hi)
        assert h.ndim == 3 and h.shape[0] == nb
        n_samples, ch = h.shape[1:]
        if lo is not None:
            l = _f32(lo)
            assert l.shape == h.shape
    if origin is not None:
        org = np.ascontiguousarray(origin, dtype=np.int64)
        assert org.shape == (nb,)
    kp = max(int(number), 128)
    fs = -(-f // 32) * 32
    idx = np.empty((nb, n_rows + 1, kp), dtype=np.int32)
    cnt = np.empty((nb, n_rows + 1), dtype=np.int32)
    u64 = np.empty((nb, n_frames, fs), dtype=np.float64) if refine == 2 else None
    stamped = np.empty((nb, n_frames), dtype=np.int32) if refine == 2 else None
    stats, delta, words = (C.c_int64 * 32)(), (C.c_double * 2)(), (C.c_int64 * 8)()
    family = C.create_string_buffer(32)
    opt = lambda a: None if a is None else _native.ptr(a)
    _native.check(_stage_entry("repet_debug_peaks_stage")(
        _native.default_context(_device).handle, _native.ptr(m), nb, m_rows, cols, pitch, opt(u), n_frames, f, opt(h), opt(l), n_samples, ch,
        int(W), int(frame_sample0), int(mode), int(row0), n_rows, float(min_value), int(d), int(number), int(shift), opt(org), int(start),
        int(bool(with_scratch)), int(refine), int(prefill), _native.ptr(idx), _native.ptr(cnt), stats, delta, opt(u64), opt(stamped),
        family, len(family), words))
    w = [int(k) for k in words]
    assert w[5] == kp and (not refine or w[6] == fs)
    st = [int(k) for k in stats]
    out = {"idx": idx, "count": cnt, "KP": kp, "stats": st, "counters": dict(zip(PEAK_REFINE_STATS, st)), "delta": float(delta[0]),
           "delta2": float(delta[1]),
           "launch": {"family": family.value.decode(), "qmax": w[0], "rd": w[1], "unit_rows_variant": w[2], "lite": bool(w[3]), "exact_fft": w[4]}}
    if refine == 2:
        out["u64"], out["stamped"] = u64, stamped.astype(bool)
    return out


DEVIO_OPS = {name: k for k, name in enumerate((
    "ingest", "egress", "emit", "levels", "tail_clear", "append", "row_copies", "slide_held", "slot_set", "feed", "take", "slot_reset",
    "slot_export", "slot_import", "gain_fill", "gain_set", "gain_commit", "band_expand", "band_commit"))}
DEVIO_GUARD = 512            # bytes of prefill returned in front of and behind every arena


def _devio_stage(op, arenas, words, floats=(), shifts=None, prefill=0xA5):
    """One production launcher of csrc/devio.hip on device buffers the caller describes (``repet_debug_devio_stage``; the words of
    every ``op`` are listed where engine_stages.hip reads them). ``arenas``: NumPy arrays, each uploaded into an allocation of its
    own with its first byte ``shifts[k]`` (0, 4, 8 or 12; 2 for 16-bit elements) bytes behind a 256-byte boundary and the byte ``prefill`` everywhere
    else; a pointer argument is the pair of words (arena, element offset), arena -1 for null. Returns ``(outs, report)``:
    ``outs[k]`` the bytes of arena k as the launch left them with ``DEVIO_GUARD`` bytes of guard on either side (uint8), and what the
    launcher decided -- ``launches``, the last ``grid``, ``dense`` per destination, ``src_vec`` / ``dst_vec`` / ``held_vec`` per
    part, -1 where the launcher decides no such thing. ValueError where the launch would index outside an arena, or the launcher
    refuses its arguments; nothing is launched then."""
    import ctypes as C
    held = [np.ascontiguousarray(a) for a in arenas]
    n = len(held)
    shifts = [0] * n if shifts is None else [int(v) for v in shifts]
    assert len(shifts) == n
    outs = [np.empty(a.nbytes + 2 * DEVIO_GUARD, dtype=np.uint8) for a in held]
    # (an empty array has no address NumPy would vouch for: a byte of its own stands in)
    pad = np.zeros(16, dtype=np.uint8)
    ins = (C.c_void_p * n)(*[(a if a.nbytes else pad).ctypes.data for a in held])
    out_p = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    sizes = (C.c_int64 * n)(*[a.nbytes for a in held])
    sh = (C.c_int32 * n)(*shifts)
    iv = [int(v) for v in words]
    fv = [float(v) for v in floats]
    ivs, fvs = (C.c_int64 * max(1, len(iv)))(*iv), (C.c_double * max(1, len(fv)))(*fv)
    rep = (C.c_int64 * 24)()
    _native.check(_stage_entry("repet_debug_devio_stage")(_native.default_context(_device).handle, DEVIO_OPS[op], n, ins, sizes, sh, out_p,
                                                          int(prefill), ivs, len(iv), fvs, len(fv), rep))
    r = [int(v) for v in rep]
    return outs, {"launches": r[0], "grid": tuple(r[1:4]), "dense": tuple(r[4:6]), "src_vec": tuple(r[6:11]), "dst_vec": tuple(r[11:16]),
                  "held_vec": tuple(r[16:21])}


def _selfsimilaritymatrix(data_matrix):
    """Cosine self-similarity between the columns (repet.py:1209-1225)."""
    rows = _f32(np.asarray(data_matrix).T)
    t, f = rows.shape
    s = np.empty((t, t), dtype=np.float32)
    _native.check(_native.lib().repet_selfsim(_native.default_context(_device).handle, _native.ptr(rows), t, f,
                                              _native.ptr(s)))
    return s.astype(np.float64)


def _selfsimilarity_records(data_matrix):
    """(similarity matrix, largest, second largest, offset of the largest) per row and aligned run of 32 columns: the segment
    records the peak picking of ``sim`` works from (``repet_selfsim_records``)."""
    rows = _f32(np.asarray(data_matrix).T)
    t, f = rows.shape
    n_seg = -(-t // 32)
    s = np.empty((t, t), dtype=np.float32)
    top, second, at = (np.empty((t, n_seg), dtype=np.float32), np.empty((t, n_seg), dtype=np.float32), np.empty((t, n_seg), dtype=np.int32))
    _native.check(_native.lib().repet_selfsim_records(_native.default_context(_device).handle, _native.ptr(rows), t, f, _native.ptr(s),
                                                      _native.ptr(top), _native.ptr(second), _native.ptr(at)))
    return s, top, second, at


def _similaritymatrix(data_matrix1, data_matrix2):
    """Cosine similarity between the columns of two matrices (repet.py:1228-1246)."""
    a = _f32(np.asarray(data_matrix1).T)
    b = _f32(np.asarray(data_matrix2).T)
    out = np.empty((a.shape[0], b.shape[0]), dtype=np.float32)
    _native.check(_native.lib().repet_similarity(_native.default_context(_device).handle, _native.ptr(a), a.shape[0],
                                                 _native.ptr(b), b.shape[0], a.shape[1], _native.ptr(out)))
    return out.astype(np.float64)


def _acorr(data_matrix):
    """Unbiased autocorrelation of every column (repet.py:1108-1139)."""
    x = _f32(data_matrix)
    out = np.empty_like(x)
    _native.check(_native.lib().repet_acorr(_native.default_context(_device).handle, _native.ptr(x), x.shape[0],
                                            x.shape[1], _native.ptr(out)))
    return out.astype(np.float64)


def _beatspectrum(audio_spectrogram):
    """Beat spectrum of an (already squared) spectrogram (repet.py:1142-1158)."""
    rows = _f32(np.asarray(audio_spectrogram).T)
    t, f = rows.shape
    beat = np.empty(t, dtype=np.float32)
    _native.check(_native.lib().repet_beat_spectrum(_native.default_context(_device).handle, _native.ptr(rows),
                                                    t, f, _native.ptr(beat), t))
    return beat.astype(np.float64)


def _beatspectrogram(audio_spectrogram, segment_length, segment_step):
    """Sliding beat spectrum, ``(segment_length, number_times)`` (repet.py:1161-1206)."""
    rows = _f32(np.asarray(audio_spectrogram).T)
    t, f = rows.shape
    out = np.empty((t, int(segment_length)), dtype=np.float32)
    _native.check(_native.lib().repet_beat_spectrogram(_native.default_context(_device).handle,
                                                       _native.ptr(rows), t, f, int(segment_length),
                                                       int(segment_step), _native.ptr(out)))
    return out.T.astype(np.float64)


def _periods(beat_spectrogram, period_range):
    """Repeating period(s): arg-max lag + 1 + period_range[0] (repet.py:1249-1291)."""
    b = np.asarray(beat_spectrogram)
    cols = _f32(b[np.newaxis, :] if b.ndim == 1 else b.T)
    n_cols, n_lags = cols.shape
    out = np.empty(n_cols, dtype=np.int32)
    _native.check(_native.lib().repet_periods(_native.default_context(_device).handle, _native.ptr(cols),
                                              n_cols, n_lags, int(period_range[0]), int(period_range[1]),
                                              _native.ptr(out)))
    return int(out[0]) if b.ndim == 1 else out.astype(int)


def _local_maxima_rows(rows, minimum_value, minimum_distance, number_values):
    rows = _f32(rows)
    n_rows, n_cols = rows.shape
    idx = np.empty((n_rows, int(number_values)), dtype=np.int32)
    cnt = np.empty(n_rows, dtype=np.int32)
    _native.check(_native.lib().repet_local_maxima(_native.default_context(_device).handle, _native.ptr(rows),
                                                   n_rows, n_cols, float(minimum_value), int(minimum_distance),
                                                   int(number_values), _native.ptr(idx), _native.ptr(cnt)))
    return idx, cnt


def _localmaxima(data_vector, minimum_value, minimum_distance, number_values):
    """Values and indices of the top local maxima of a vector (repet.py:1294-1345)."""
    v = np.asarray(data_vector, dtype=float)
    idx, cnt = _local_maxima_rows(v[np.newaxis, :], minimum_value, minimum_distance, number_values)
    keep = idx[0, :cnt[0]].astype(int)
    return v[keep], keep


def _indices(similarity_matrix, similarity_threshold, similarity_distance, similarity_number):
    """Similar-frame indices of every frame: column i of the matrix is scanned (repet.py:1348-1383)."""
    idx, cnt = _local_maxima_rows(np.asarray(similarity_matrix).T, similarity_threshold, similarity_distance,
                                  similarity_number)
    return [idx[i, :cnt[i]].astype(int) for i in range(len(cnt))]


def _mask(audio_spectrogram, repeating_period):
    """Period-median repeating mask (repet.py:1386-1458)."""
    rows = _f32(np.asarray(audio_spectrogram).T)
    t, f = rows.shape
    out = np.empty((t, f), dtype=np.float32)
    _native.check(_native.lib().repet_mask_period(_native.default_context(_device).handle, _native.ptr(rows), t,
                                                  f, int(repeating_period), _native.ptr(out)))
    return out.T.astype(np.float64)


def _adaptivemask(audio_spectrogram, repeating_periods, filter_order):
    """Local-period median mask (repet.py:1461-1508)."""
    rows = _f32(np.asarray(audio_spectrogram).T)
    t, f = rows.shape
    per = np.ascontiguousarray(repeating_periods, dtype=np.int32)
    out = np.empty((t, f), dtype=np.float32)
    _native.check(_native.lib().repet_mask_adaptive(_native.default_context(_device).handle, _native.ptr(rows),
                                                    t, f, _native.ptr(per), int(filter_order), _native.ptr(out)))
    return out.T.astype(np.float64)


def _simmask(audio_spectrogram, similarity_indices):
    """Similarity-median mask from per-frame index lists (repet.py:1511-1545)."""
    rows = _f32(np.asarray(audio_spectrogram).T)
    t, f = rows.shape
    width = max(1, max((len(ix) for ix in similarity_indices), default=1))
    idx = np.full((t, width), -1, dtype=np.int32)
    cnt = np.zeros(t, dtype=np.int32)
    for i, ix in enumerate(similarity_indices):
        idx[i, :len(ix)] = ix
        cnt[i] = len(ix)
    out = np.empty((t, f), dtype=np.float32)
    _native.check(_native.lib().repet_mask_sim(_native.default_context(_device).handle, _native.ptr(rows), t, f,
                                               _native.ptr(idx), _native.ptr(cnt), width, _native.ptr(out)))
    return out.T.astype(np.float64)


def _simmask_ranked(audio_spectrogram, similarity_indices, path="bits", want_codes=False):
    """``_simmask`` the way ``sim`` computes it on clips of more than 1 024 frames: through the rank transform of every bin
    (``_rank_columns``) and the packed 16-bit selection network (``path="rank"``) or the bit-sliced selection (``"bits"``).
    ``(F, T)`` with ``F - 1`` a multiple of 128 (a power of two for ``"bits"``); ``want_codes``: also the ``uint32 (F - 1, T)``
    words the bit-sliced selection leaves (lower median's rank | flag << 15 | upper median's rank << 16)."""
    rows = _f32(np.asarray(audio_spectrogram).T)
    t, f = rows.shape
    width = max(2, max((len(ix) for ix in similarity_indices), default=2))
    idx = np.full((t, width), -1, dtype=np.int32)
    cnt = np.zeros(t, dtype=np.int32)
    for i, ix in enumerate(similarity_indices):
        idx[i, :len(ix)] = ix
        cnt[i] = len(ix)
    out = np.empty((t, f), dtype=np.float32)
    codes = np.empty((t, f - 1), dtype=np.uint32) if want_codes else None
    _native.check(_native.lib().repet_mask_sim_ranked(_native.default_context(_device).handle, _native.ptr(rows), t, f,
                                                      _native.ptr(idx), _native.ptr(cnt), width, {"rank": 1, "bits": 2}[path],
                                                      _native.ptr(out), _native.ptr(codes) if want_codes else None))
    return (out.T.astype(np.float64), codes.T) if want_codes else out.T.astype(np.float64)


def _rank_columns(audio_spectrogram):
    """Rank transform behind the median of ``sim`` (no counterpart in the reference: np.median at repet.py:1535 only
    needs the order of a bin's magnitudes). ``(F, T)`` -> (codes ``(n, T)`` uint16 = 0x0400 + number of strictly smaller
    magnitudes of the bin, sorted ``(n, T)``) for the first ``n = F // 128 * 128`` bins."""
    rows = _f32(np.asarray(audio_spectrogram).T)
    t, f = rows.shape
    n = f // 128 * 128
    codes = np.empty((t, n), dtype=np.uint16)
    ordered = np.empty((n, t), dtype=np.float32)
    _native.check(_native.lib().repet_rank_columns(_native.default_context(_device).handle, _native.ptr(rows), t, f,
                                                   _native.ptr(codes), _native.ptr(ordered)))
    return codes.T, ordered


# ---- file / display utilities of the reference (host side, off the hot path) --------------------------------
def wavread(audio_file):
    """Read a WAVE file, integers scaled to [-1, 1) by their bit depth (repet.py:914-931): the array SciPy would return,
    divided by ``2 ** (8 * itemsize - 1)`` -- 24-bit PCM counts as int32 (sample in the top three bytes), 8-bit PCM is
    unsigned, and float files are divided too (a quirk of the reference, kept). The header is parsed by the library
    (``repet_wav_parse``); formats it does not handle go through ``scipy.io.wavfile`` like the reference."""
    image = np.fromfile(audio_file, dtype=np.uint8)
    info = _native.WavInfo()
    lib = _native.lib()
    if lib.repet_wav_parse(_native.ptr(image), image.size, info) != 0:
        import scipy.io.wavfile
        sampling_frequency, samples = scipy.io.wavfile.read(audio_file)
        return samples / pow(2, samples.itemsize * 8 - 1), sampling_frequency
    count = info.n_samples * info.n_channels
    width = info.bytes_per_sample
    raw = image[info.data_offset:info.data_offset + count * width]
    if info.format == 3:
        samples = raw.view("<f4" if width == 4 else "<f8")
    elif width == 1:
        samples = raw
    elif width == 3:                                          # packed 24-bit -> int32 with the sample in the top bytes
        wide = np.zeros((count, 4), dtype=np.uint8)
        wide[:, 1:] = raw.reshape(count, 3)
        samples = wide.view("<i4").ravel()
    else:
        samples = raw.view("<i2" if width == 2 else "<i4")
    samples = samples.reshape(info.n_samples, info.n_channels) if info.n_channels > 1 else samples.reshape(info.n_samples)
    return samples / pow(2, samples.itemsize * 8 - 1), int(info.sampling_frequency)


def wavwrite(audio_signal, sampling_frequency, audio_file):
    """Write a WAVE file with the dtype as given (repet.py:934-946): byte for byte what ``scipy.io.wavfile.write``
    produces for float64 / float32 (IEEE-float format: 18-byte fmt chunk, fact chunk) and int16 / int32 / uint8 (PCM)
    arrays; other dtypes go to SciPy (which raises for most of them, as in the reference)."""
    import struct
    data = np.asarray(audio_signal)
    if data.dtype.name not in ("float64", "float32", "int16", "int32", "uint8") or data.ndim not in (1, 2) or data.nbytes > 0xFFFFFF00:
        import scipy.io.wavfile
        scipy.io.wavfile.write(audio_file, sampling_frequency, audio_signal)
        return
    channels = 1 if data.ndim == 1 else data.shape[1]
    item = data.dtype.itemsize
    is_float = data.dtype.kind == "f"
    fmt = struct.pack("<HHIIHH", 3 if is_float else 1, channels, int(sampling_frequency), int(sampling_frequency) * item * channels,
                      channels * item, item * 8) + (b"\x00\x00" if is_float else b"")
    head = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    if is_float:
        head += b"fact" + struct.pack("<II", 4, data.shape[0])
    head += b"data" + struct.pack("<I", data.nbytes)
    body = np.ascontiguousarray(data.astype(data.dtype.newbyteorder("<"), copy=False))
    with open(audio_file, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", 4 + len(head) + data.nbytes) + b"WAVE" + head)
        body.tofile(fh)


def separate_file(algo, audio_file, background_file=None, foreground_file=None, dtype=np.float64):
    """``wavread`` -> ``algo`` -> ``wavwrite`` of the README example (README.md:62-72) without the samples visiting host
    arrays in between: the file's raw PCM goes to the device, is decoded and normalised there, separated, and the
    background / foreground (``audio - background``) come back as finished file images. Returns the sampling frequency.
    The files equal ``wavwrite(algo(*wavread(audio_file)))`` resp. the same for ``audio - background``."""
    ctx = _native.default_context(_device)
    sampling_frequency = ctx.upload_wav(audio_file)
    ctx.execute(algo, derive_params(sampling_frequency))
    if background_file is not None:
        ctx.write_wav(background_file, "background", dtype)
    if foreground_file is not None:
        ctx.write_wav(foreground_file, "foreground", dtype)
    return sampling_frequency


def specshow(audio_spectrogram, time_duration, maximum_frequency, xtick_step=1, ytick_step=1000):
    """Show a spectrogram in dB with second / Hz ticks (repet.py:949-997)."""
    import matplotlib.pyplot as plt
    number_frequencies, number_times = np.shape(audio_spectrogram)
    per_second = number_times / time_duration
    per_hertz = number_frequencies / maximum_frequency
    plt.imshow(20 * np.log10(audio_spectrogram), aspect="auto", cmap="jet", origin="lower")
    plt.xticks(ticks=np.arange(xtick_step * per_second, number_times, xtick_step * per_second),
               labels=np.arange(xtick_step, time_duration, xtick_step).astype(int))
    plt.yticks(ticks=np.arange(ytick_step * per_hertz, number_frequencies, ytick_step * per_hertz),
               labels=np.arange(ytick_step, maximum_frequency, ytick_step).astype(int))
    plt.xlabel("Time (s)")
    plt.ylabel("Frequency (Hz)")
