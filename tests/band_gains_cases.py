"""The signals and tables of tests/test_gpu_online_band_gains.py, in a module of their own so that the CPU test of the model
(tests/test_band_gains_reference.py) can hold every one of them to its sensitivity conditions without a GPU.

Signals: ``signal(seed, n, fs, ch)`` of tests/test_gpu_online_start.py (restated here, the GPU file asserts that the two agree):
fp32-exact synthetic mixtures. 8 kHz: W 512, H 256, B 312, F 257, cutoff 6; 44.1 kHz: W 2048, H 1024, B 431, F 1025.

Tables, as ``(edges, gains)`` for ``set_background_band_gains`` (edges None: per bin). The bands lie where these signals have
energy in their background (the test of the model checks that, table by table and signal by signal)."""
import functools

import numpy as np

import repet
from repet_synth import synth

FS = 8000
W, H, B, F, CUT = 512, 256, 312, 257, 6
M_YOUNG = 33                                   # start_frames of the young cases: similarity_distance is 31 frames
N8 = (B + 80) * H + 77                         # 12.55 s, an odd finish tail

FS44 = 44100
W44, H44, F44 = 2048, 1024, 1025
M44 = 3 * 43 + 1                               # just above 3 x similarity_distance (43 frames)
N44 = 151 * H44 + 333                          # 3.5 s


@functools.lru_cache(maxsize=None)
def signal(seed, n, fs, ch):
    x = synth(n / fs + 0.01, fs, ch, seed)[:n].astype(np.float32).astype(np.float64)
    x.setflags(write=False)
    return x


def _per_bin(f, seed):
    rs = np.random.RandomState(seed)
    return np.round(rs.uniform(0, 1, size=f) * 64) / 64


DUCK = 10 ** (-12 / 20)
TABLES = {
    # keep the bass in the foreground: the high-pass bins and DC
    "bass": ([0, CUT + 1], [1.0]),
    # remove the background only between 300 Hz and 3.4 kHz
    "speech-only": ([0, 19, 218, F], [1.0, 0.0, 1.0]),
    # duck by 12 dB in the speech band, fully elsewhere
    "duck": ([19, 218], [DUCK]),
    # two one-bin bands side by side, and an empty band between edges that coincide
    "one-bin": ([12, 13, 13, 14], [1.0, 0.5, 0.25]),
    # one gain per bin
    "per-bin": (None, _per_bin(F, 5)),
    # every bin kept: the foreground is the input
    "all": ([0, F], [1.0]),
    # 44.1 kHz
    "mel44": (repet.band_edges(FS44, 24), np.round(np.linspace(0.1, 0.9, 24) * 32) / 32),
    "per-bin44": (None, _per_bin(F44, 6)),
    "one-bin44": ([40, 41, 42], [1.0, 0.5]),
}

# (table, seed, n, fs, channels, start_frames) of every run of the GPU file that is compared with the model
USES = [
    ("speech-only", 31, N8, FS, 2, M_YOUNG), ("per-bin", 31, N8, FS, 1, B), ("duck", 31, N8, FS, 3, M_YOUNG),
    ("bass", 32, N8, FS, 2, M_YOUNG), ("one-bin", 32, N8, FS, 2, M_YOUNG), ("duck", 32, N8, FS, 2, M_YOUNG),
    ("per-bin", 32, N8, FS, 2, M_YOUNG), ("speech-only", 32, N8, FS, 2, M_YOUNG),
    ("bass", 33, N8, FS, 2, M_YOUNG), ("duck", 33, N8, FS, 2, M_YOUNG), ("one-bin", 33, N8, FS, 2, M_YOUNG),
    ("mel44", 34, N44, FS44, 1, M44), ("per-bin44", 35, N44, FS44, 2, M44), ("one-bin44", 35, N44, FS44, 2, M44),
]
