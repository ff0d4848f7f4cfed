"""The inverse STFT of every offline pipeline goes through one function (csrc/engine.hip: enqueue_istft): the plain launches, the
"istft_ola" timing mark, under band gains the shaped twin of every launch, the "istft_ola_shaped" mark. The marks are events on the
stream, so the stage names a timed execute reports show the order. The lists below were recorded from the commit before the five
hand-written copies became that function, and pin it.

8 kHz stereo (window 512, hop 256), the module parameters shrunk to segments of 2 s every 1 s and a buffer of 2 s. N samples are
just enough for three ``extended`` segments: two equal ones as one batch, in two residue classes of which the first stores, and
the longer last one on the auxiliary context (its stages are not listed; "last_segment" stands for it). The same clip twice is
the equal batch, the pair with one shorter length the ragged one. A batch a variant works through clip by clip reports "clips"
only."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import repet
from repet_synth import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FS = 8000
N = 33000                    # segments [0, 16000), [8000, 24000), [16000, 33000)
SHORT = 32100                # still three segments
ALGOS = ("original", "extended", "adaptive", "sim", "simonline")
CASES = ("one", "equal", "ragged")
SHRUNK = {"segment_length": 2, "segment_step": 1, "buffer_length": 2, "period_range": [0.1, 0.5]}

# (case, algo) -> the names the parent commit reported, without a table and with one
PERIOD = ["stft", "gram_band", "beat_period", "mask_period"]
ONLINE = ["stft", "similarity_band_f16x3", "local_maxima", "mask_sim"]
PLAIN = {
    ("one", "original"): PERIOD + ["istft_ola"],
    ("one", "extended"): PERIOD + ["istft_ola", "last_segment"],
    ("one", "adaptive"): ["stft", "gram_band", "beat_periods", "mask_adaptive", "istft_ola"],
    ("one", "sim"): ["stft", "similarity_gemm_f16x3", "segment_maxima", "local_maxima", "mask_sim", "istft_ola"],
    ("one", "simonline"): ONLINE + ["istft_ola"],
    ("equal", "original"): PERIOD + ["istft_ola"],
    ("equal", "extended"): ["clips"],
    ("equal", "adaptive"): ["clips"],
    ("equal", "sim"): ["clips"],
    ("equal", "simonline"): ONLINE + ["istft_ola"],
    ("ragged", "original"): ["clips"],
    ("ragged", "extended"): ["clips"],
    ("ragged", "adaptive"): ["clips"],
    ("ragged", "sim"): ["clips"],
    ("ragged", "simonline"): ONLINE + ["tail_clear", "istft_ola"],
}
SHAPED = {
    ("one", "original"): PERIOD + ["istft_ola", "istft_ola_shaped"],
    ("one", "extended"): PERIOD + ["istft_ola", "istft_ola_shaped", "last_segment"],
    ("one", "adaptive"): ["stft", "gram_band", "beat_periods", "mask_adaptive", "istft_ola", "istft_ola_shaped"],
    ("one", "sim"): ["stft", "similarity_gemm_f16x3", "segment_maxima", "local_maxima", "mask_sim", "istft_ola", "istft_ola_shaped"],
    ("one", "simonline"): ONLINE + ["istft_ola", "istft_ola_shaped"],
    ("equal", "original"): PERIOD + ["istft_ola", "istft_ola_shaped"],
    ("equal", "extended"): ["clips"],
    ("equal", "adaptive"): ["clips"],
    ("equal", "sim"): ["clips"],
    ("equal", "simonline"): ONLINE + ["istft_ola", "istft_ola_shaped"],
    ("ragged", "original"): ["clips"],
    ("ragged", "extended"): ["clips"],
    ("ragged", "adaptive"): ["clips"],
    ("ragged", "sim"): ["clips"],
    ("ragged", "simonline"): ONLINE + ["tail_clear", "istft_ola", "istft_ola_shaped"],
}


@pytest.fixture(scope="module", autouse=True)
def shrunk_parameters():
    saved = {k: getattr(repet, k) for k in SHRUNK}
    for k, v in SHRUNK.items():
        setattr(repet, k, v)
    yield
    for k, v in saved.items():
        setattr(repet, k, v)


_clip = {}


def clips(case):
    """The tensor of a case and its ``lengths``."""
    if not _clip:
        _clip["x"] = torch.from_numpy(synth(N / FS, FS, 2, 5)).to(DEV)
    x = _clip["x"]
    if case == "one":
        return x, None
    return torch.stack([x, x]), ([N, SHORT] if case == "ragged" else None)


def one_gain():
    g = np.zeros(repet.derive_params(FS).window_length // 2 + 1, dtype=np.float32)
    g[3] = 0.5
    return g


def stage_names(case, algo, table):
    x, lengths = clips(case)
    p = repet.derive_params(FS)
    c = repet.Context(0)
    try:
        c.upload_tensor(x, lengths=lengths)
        if table:
            c.set_background_band_gains(one_gain(), window_length=p.window_length)
        return [s["name"] for s in c.execute(algo, p, timing=True)["stages"]]
    finally:
        c.close()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@pytest.mark.parametrize("algo", ALGOS)
def test_stage_names_are_the_parents(algo):
    for case in CASES:
        plain, shaped = stage_names(case, algo, False), stage_names(case, algo, True)
        print(case, algo, plain, shaped)
        assert plain == PLAIN[(case, algo)], case
        assert shaped == SHAPED[(case, algo)], case
        if plain == ["clips"]:                       # a loop over clips lists no stage, with or without a table
            assert shaped == ["clips"], case
            continue
        assert plain.count("istft_ola") == 1 and "istft_ola_shaped" not in plain, case
        at = plain.index("istft_ola")
        assert shaped == plain[:at + 1] + ["istft_ola_shaped"] + plain[at + 1:], case


@pytest.mark.parametrize("algo", ALGOS)
def test_results_do_not_depend_on_what_is_asked_for(algo):
    zeros = np.zeros_like(one_gain())
    for case in CASES:
        x, lengths = clips(case)
        bg, fg = repet.separate(algo, x, FS, which="both", lengths=lengths)
        assert same_bits(bg, repet.separate(algo, x, FS, which="background", lengths=lengths)), case
        assert same_bits(fg, repet.separate(algo, x, FS, which="foreground", lengths=lengths)), case
        zbg, zfg = repet.separate(algo, x, FS, which="both", background_band_gains=zeros, lengths=lengths)
        assert same_bits(zbg, bg) and same_bits(zfg, fg), case
        assert bool(torch.isfinite(bg).all()) and float(bg.abs().max()) > 0, case
