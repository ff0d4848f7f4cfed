"""Wall time of repet.sim on a ROCm torch tensor (float64 and float32 input) at BASELINE config 2 (one 180-s 44.1 kHz stereo
clip), beside the NumPy drop-in call and the device step (timing series of a resident context) measured in the same run.
Host clock around call + torch.cuda.synchronize(); medians over --reps calls after a warm-up. One JSON line per row.
--kernels: only a few tensor calls of each dtype (for a `rocprofv3 --kernel-trace --stats` run of the ingest / egress
kernels, devio_ingest_* and devio_egress_*).
--which foreground [--bands N]: only repet.separate("sim", tensor, which="foreground") on the float64 and the float32 tensor,
without a table or with N band gains (repet.band_edges(fs, N), gains from 0.1 to 0.9), and the device stages of the same run on
a resident context (the inverse STFT and, under a table, its shaped twin side by side). --calls K with --which: K calls and
nothing else (for a kernel trace of exactly those calls)."""
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
    return float(np.median(ts) * 1e3), float(np.min(ts) * 1e3)


def probe_which(args, fs, x64, x32):
    kw = {}
    if args.bands:
        kw = {"background_band_gains": np.round(np.linspace(0.1, 0.9, args.bands) * 32) / 32,
              "band_edges": repet.band_edges(fs, args.bands)}
    label = f"{args.which}, {args.bands} bands" if args.bands else f"{args.which}, no table"
    if args.calls:
        for _ in range(args.calls):
            repet.separate("sim", x64, fs, which=args.which, **kw)
        torch.cuda.synchronize()
        print(json.dumps({"calls": args.calls, "what": label}))
        return
    for name, t in (("f64", x64), ("f32", x32)):
        med, best = median_ms(lambda: repet.separate("sim", t, fs, which=args.which, **kw), args.reps)
        print(json.dumps({"row": f"tensor_{name}_ms", "what": label, "median_ms": round(med, 4), "min_ms": round(best, 4)}))
    p = repet.derive_params(fs)
    ctx = repet.Context(0)
    ctx.upload_tensor(x64)
    if args.bands:
        ctx.set_background_band_gains(kw["background_band_gains"], kw["band_edges"], window_length=p.window_length)
    ctx.execute("sim", p)
    ctx.timing_series_begin(args.reps)
    for _ in range(args.reps):
        ctx.execute_async("sim", p)
    series = ctx.timing_series_end()
    ctx.close()
    stages = {st["name"]: round(st["ms"], 4) for st in series["stages"] if st["name"].startswith("istft")}
    print(json.dumps({"row": "device_step_ms", "what": label, "mean_ms": round(series["total_ms"], 4), "stages": stages}))
    print(json.dumps({"clip": f"{args.seconds:g} s {fs} Hz stereo", "reps": args.reps, "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--which", default=None)
    ap.add_argument("--bands", type=int, default=0)
    ap.add_argument("--calls", type=int, default=0)
    args = ap.parse_args()
    fs = 44100
    x = synth(args.seconds, fs, 2, 0)
    x64 = torch.from_numpy(x).cuda()
    x32 = x64.float()
    if args.which:
        return probe_which(args, fs, x64, x32)
    if args.kernels:
        for t in (x64, x32):
            for _ in range(5):
                repet.sim(t, fs)
        torch.cuda.synchronize()
        print(json.dumps({"kernels": "done", "calls": 10}))
        return
    want = repet.sim(x, fs)
    got = repet.sim(x64, fs)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want, equal_nan=True)
    # where a call's time goes: the host until the call returns (everything enqueued), and the span the caller's stream sees
    # between an event recorded right before the call and one right after it (ingest, run, egress and the event hand-offs)
    for name, t in (("f64", x64), ("f32", x32)):
        enq, span = [], []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            repet.sim(t, fs)
            e1.record()
            enq.append(time.perf_counter() - t0)
            e1.synchronize()
            span.append(e0.elapsed_time(e1))
        print(json.dumps({"row": f"tensor_{name}_breakdown", "host_enqueue_ms": round(float(np.median(enq)) * 1e3, 4),
                          "stream_span_ms": round(float(np.median(span)), 4)}))
    rows = {}
    rows["tensor_f64_ms"] = median_ms(lambda: repet.sim(x64, fs), args.reps)
    rows["tensor_f32_ms"] = median_ms(lambda: repet.sim(x32, fs), args.reps)
    rows["numpy_f64_ms"] = median_ms(lambda: repet.sim(x, fs), max(5, args.reps // 4))
    p = repet.derive_params(fs)
    ctx = repet.Context(0)
    ctx.upload(x)
    ctx.execute("sim", p)
    ctx.timing_series_begin(args.reps)
    for _ in range(args.reps):
        ctx.execute_async("sim", p)
    step = ctx.timing_series_end()["total_ms"]
    ctx.close()
    for k, (med, best) in rows.items():
        print(json.dumps({"row": k, "median_ms": round(med, 4), "min_ms": round(best, 4)}))
    print(json.dumps({"row": "device_step_ms", "mean_ms": round(step, 4)}))
    print(json.dumps({"clip": f"{args.seconds:g} s {fs} Hz stereo", "reps": args.reps, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
