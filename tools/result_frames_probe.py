"""Calls of repet.separate(algo, x, fs[, frames=...]) on a ROCm torch tensor, for the evidence of the spectra of a tensor call
(profiles/result_frames_dispatches.txt, profiles/result_frames_ab.txt).
--calls K: K calls and nothing else (for a `rocprofv3 --kernel-trace --stats` run of exactly those calls, one process per
variation). Without --calls: the wall time of a call without a request and with one (host clock around call +
torch.cuda.synchronize(), median of --reps after a warm-up), one JSON line per row.
--frames mixture|background|foreground, --bands N (repet.band_edges(fs, N)), --clips B (a batch of B equal clips), --seconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "repet-python_amd"), ROOT]

import torch  # noqa: E402

import repet  # noqa: E402
from repet_synth import synth  # noqa: E402


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts) * 1e3), 4), round(float(np.min(ts) * 1e3), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", default="sim")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--clips", type=int, default=1)
    ap.add_argument("--frames", default=None)
    ap.add_argument("--bands", type=int, default=0)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    fs = 44100
    x = torch.from_numpy(np.stack([synth(args.seconds, fs, 2, seed) for seed in range(args.clips)])).cuda()
    if args.clips == 1:
        x = x[0]
    kw = {}
    if args.frames:
        kw["frames"] = args.frames
        if args.bands:
            kw["frame_bands"] = repet.band_edges(fs, args.bands)
    what = f"{args.algo}, {args.clips} x {args.seconds:g} s {fs} Hz stereo float64"
    if args.calls:
        for _ in range(args.calls):
            repet.separate(args.algo, x, fs, **kw)
        torch.cuda.synchronize()
        print(json.dumps({"calls": args.calls, "what": what, "request": kw and {k: str(v)[:40] for k, v in kw.items()}}))
        return
    rows = [("no request", {})]
    for which in ("mixture", "background", "foreground"):
        rows.append((f"frames={which}", {"frames": which}))
    rows.append(("frames=background, 32 bands", {"frames": "background", "frame_bands": repet.band_edges(fs, 32)}))
    for label, kw in rows:
        med, best = median_ms(lambda: repet.separate(args.algo, x, fs, **kw), args.reps)
        print(json.dumps({"row": label, "what": what, "median_ms": med, "min_ms": best}))
    print(json.dumps({"reps": args.reps, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
