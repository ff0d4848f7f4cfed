"""Float64 NumPy statement of the SHAPED background of a tensor call with band gains (include/repet_hip.h:
repet_ctx_set_background_band_gains), and the cases tests/test_gpu_tensor_band_gains.py compares with it -- in a module of their
own so that tests/test_band_gains_offline_reference.py can hold every one of them to its sensitivity condition without a GPU.

``shaped_background(algo, x, fs, a)``: for ``original``, ``extended``, ``adaptive`` and ``sim`` the oracle's own run with
``orc.resynthesize`` replaced, for the length of the call, by one that multiplies the mask's rows by ``a[:, None]`` -- bin
``N - k`` takes bin ``k``'s factor through the mirror of the mask, and ``extended`` inherits it through its segments, cross-fade
included. For ``simonline`` it is ``band_gains_reference.band_gains_from`` with the one table on every frame and the reference's
``start_frames`` (the buffer length). ``a`` is ``band_gains_reference.factor(g)``, ``(F,)``.

``plain_background(algo, x, fs)`` is the oracle's background itself."""
import functools

import numpy as np

import repet
from oracle import repet_oracle as orc

import band_gains_cases as cases
import band_gains_reference as bgr

ALGOS = ("original", "extended", "adaptive", "sim", "simonline")


def buffer_frames(fs):
    _, _, h = orc.stft_geometry(fs)
    return round((orc.Params().buffer_length * fs) / h)


def shaped_background(algo, x, fs, a):
    a = np.asarray(a, dtype=np.float64)
    if algo == "simonline":
        t = bgr.frame_count(len(x), fs)
        return bgr.band_gains_from(x, fs, buffer_frames(fs), np.tile(a, (t, 1)))[1]
    plain = orc.resynthesize

    def shaped(mask, spec_c, window, h, n):
        return plain(mask * a[:, np.newaxis], spec_c, window, h, n)

    orc.resynthesize = shaped
    try:
        return getattr(orc, algo)(x, fs)
    finally:
        orc.resynthesize = plain


def plain_background(algo, x, fs):
    return getattr(orc, algo)(x, fs)


def bins(fs):
    w, _, _ = orc.stft_geometry(fs)
    return w // 2 + 1


# ---- the cases -----------------------------------------------------------------------------------------------------------
def samples(seconds, fs):
    return round(seconds * fs) + 77


def _mel24(fs):
    return repet.band_edges(fs, 24), np.round(np.linspace(0.1, 0.9, 24) * 32) / 32


# name -> (edges, gains); the 24-band tables of the further cases are per sampling frequency
TABLES = dict(cases.TABLES)
TABLES.update({"mel16k": _mel24(16000), "mel96k": _mel24(96000)})

# (name of the signal, fs, seconds, channels, seed, variants, tables)
ROWS = [
    # W = 512, block kernels, three `extended` segments so that one segment fades at both ends
    ("8k-stereo", 8000, 21, 2, 31, ALGOS, ("bass", "speech-only", "duck", "one-bin", "per-bin", "all")),
    # a channel count the wave kernel does not take
    ("8k-three", 8000, 16, 3, 32, ("sim", "extended"), ("duck", "per-bin")),
    # W = 2048: the register kernels, the model form for original / extended, two segments
    ("44k-stereo", 44100, 16, 2, 35, ALGOS, ("mel44", "per-bin44")),
    # W = 1024
    ("16k-mono", 16000, 14, 1, 36, ("sim", "adaptive"), ("mel16k",)),
    # W = 4096
    ("96k-mono", 96000, 11, 1, 37, ("sim", "original"), ("mel96k",)),
    # the channel-group split of the block kernel (13 channels of W = 2048 do not fit one workgroup's LDS)
    ("44k-thirteen", 44100, 6, 13, 38, ("original",), ("mel44",)),
]

# every (row name, variant, table) that is compared with the model
USES = [(row[0], algo, table) for row in ROWS for algo in row[5] for table in row[6]]
ROW_BY_NAME = {row[0]: row for row in ROWS}


def row_signal(name):
    _, fs, seconds, ch, seed, _, _ = ROW_BY_NAME[name]
    return cases.signal(seed, samples(seconds, fs), fs, ch), fs


def table_gains(name, fs):
    """The per-bin float32 gains ``g`` (F,) of a named table at ``fs``."""
    edges, gains = TABLES[name]
    return bgr.table(bins(fs), edges, gains)


@functools.lru_cache(maxsize=None)
def plain_of(name, algo):
    x, fs = row_signal(name)
    out = plain_background(algo, x, fs)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _simonline_state(name):
    x, fs = row_signal(name)
    return bgr.masks_of(x, fs, buffer_frames(fs))


@functools.lru_cache(maxsize=None)
def shaped_of(name, algo, table):
    x, fs = row_signal(name)
    a = bgr.factor(table_gains(table, fs))
    if algo == "simonline":                        # (the spectra and masks once per signal, whatever the table)
        state = _simonline_state(name)
        out = bgr.shaped_from(state, np.tile(a, (state["t"], 1)))[1]
    else:
        out = shaped_background(algo, x, fs, a)
    out.setflags(write=False)
    return out


def rms(v):
    return float(np.sqrt(np.mean(np.square(np.asarray(v, dtype=np.float64)))))
