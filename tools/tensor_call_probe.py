"""Wall time of repet.sim on a ROCm torch tensor (float64 and float32 input) at BASELINE config 2 (one 180-s 44.1 kHz stereo
clip), beside the NumPy drop-in call and the device step (timing series of a resident context) measured in the same run.
Host clock around call + torch.cuda.synchronize(); medians over --reps calls after a warm-up. One JSON line per row.
--kernels: only a few tensor calls of each dtype (for a `rocprofv3 --kernel-trace --stats` run of the ingest / egress
kernels, devio_ingest_* and devio_egress_*)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    fs = 44100
    x = synth(args.seconds, fs, 2, 0)
    x64 = torch.from_numpy(x).cuda()
    x32 = x64.float()
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
