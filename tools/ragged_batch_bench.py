"""What the ragged batch (``repet.separate(..., lengths=...)``) costs and saves, on an MI355X. 44.1 kHz stereo, float32 tensors on
the device, a preallocated float32 ``out``; every timed call is the call plus one ``torch.cuda.synchronize()``.

Legs (each timed ``--timed`` times after ``--warm`` untimed calls; the median is reported):

  equal_simonline   the 64 x 30 s ``simonline`` batch of equal clips, without ``lengths``: the path that must not change
  sim_one_clip      ``sim`` of one 30-s clip
  ragged_batch      64 clips with lengths spread evenly over 20 .. 30 s as ONE ragged ``simonline`` call      (this build only)
  ragged_loop       the same 64 clips as 64 one-clip calls, one synchronize behind the last                   (this build only)

Driver (the default): ``--rounds R`` rounds; in every round one fresh child process per build -- the parent commit's package
(``--parent DIR``, a directory that holds its ``repet`` package and built library) and this tree's --, in an order that flips from
round to round, each running every leg it has. Reported per leg and build: the median of every round. The equal-length legs are
accepted when every round median of this build lies inside the parent's own round-to-round range in the same session; otherwise the
document says by how much the worst round lies outside, and by how much above (a round below the range is a faster one).
``ragged_batch`` against ``ragged_loop`` is reported as a ratio of the medians of the round medians. ``--out FILE`` also writes the document there.

``--child``: one build (``REPET_PACKAGE_DIR``, default ``repet-python_amd``), its legs, one JSON line.
``--dispatch ragged|equal``: one ``simonline`` batch of that kind, three calls and nothing else: the process to put under
``rocprofv3 --kernel-trace --stats`` (profiles/ragged_batch_dispatches.txt)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

FS, CH, CLIPS, SECONDS = 44100, 2, 64, 30
EQUAL_LEGS = ("equal_simonline", "sim_one_clip")
RAGGED_LEGS = ("ragged_batch", "ragged_loop")


def batch_and_lengths():
    """(B, N, C) float32 clips from a few synthesised ones (rolled and scaled), and lengths spread evenly over 20 .. 30 s."""
    from repet_synth import synth
    base = [synth(SECONDS, FS, CH, seed) for seed in range(4)]
    x = np.stack([np.roll(base[b % 4], 997 * b, axis=0) * (1.0 - 0.001 * b) for b in range(CLIPS)]).astype(np.float32)
    n = x.shape[1]
    lengths = [int(round(n * (2.0 / 3.0 + b / (3.0 * (CLIPS - 1))))) for b in range(CLIPS)]
    lengths[-1] = n
    return x, lengths


def timed_calls(call, warm, timed):
    import torch
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    lat = []
    for _ in range(timed):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
    return round(float(np.median(lat)) * 1e3, 4)


def child(args):
    sys.path[:0] = [os.environ.get("REPET_PACKAGE_DIR", "repet-python_amd"), "."]
    import torch
    import repet
    x, lengths = batch_and_lengths()
    xd = torch.tensor(x, device="cuda:0")
    out = torch.empty_like(xd)
    has_lengths = hasattr(repet._native, "clip_lengths")         # (a build with the ragged batch)
    result = {"package": os.path.dirname(os.path.abspath(repet.__file__)), "has_lengths": has_lengths}
    if args.dispatch:
        kw = {"lengths": lengths} if args.dispatch == "ragged" else {}
        for _ in range(3):
            repet.separate("simonline", xd, FS, out=out, **kw)
        torch.cuda.synchronize()
        print(json.dumps({"dispatch": args.dispatch, "calls": 3}))
        return
    result["equal_simonline"] = timed_calls(lambda: repet.separate("simonline", xd, FS, out=out), args.warm, args.timed)
    result["sim_one_clip"] = timed_calls(lambda: repet.separate("sim", xd[0], FS, out=out[0]), args.warm, 2 * args.timed)
    if has_lengths:
        result["ragged_batch"] = timed_calls(lambda: repet.separate("simonline", xd, FS, out=out, lengths=lengths), args.warm, args.timed)

        def loop():
            for b, n in enumerate(lengths):
                repet.separate("simonline", xd[b, :n], FS, out=out[b, :n])
        result["ragged_loop"] = timed_calls(loop, 1, max(3, args.timed // 2))
    print(json.dumps(result))


def run_child(args, package):
    env = dict(os.environ, REPET_PACKAGE_DIR=package)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--timed", str(args.timed), "--warm", str(args.warm)]
    done = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.child_timeout)
    if done.returncode != 0:
        raise SystemExit(f"the child for {package} ended with status {done.returncode}: no further process is started")
    return json.loads(done.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--dispatch", choices=["ragged", "equal"], default=None)
    ap.add_argument("--parent", default=None, help="the parent commit's package directory (its repet/ and built lib/)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timed", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds one child may take")
    ap.add_argument("--label", default=None, help="recorded as `build`: the commit that was measured")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child or args.dispatch:
        return child(args)
    builds = {"this": "repet-python_amd"}
    if args.parent:
        builds["parent"] = args.parent
    rounds = {name: [] for name in builds}
    for r in range(args.rounds):
        order = list(builds) if r % 2 == 0 else list(builds)[::-1]
        for name in order:
            rounds[name].append(run_child(args, builds[name]))
            print(json.dumps({"round": r, "build": name, **rounds[name][-1]}), file=sys.stderr, flush=True)
    doc = {"fs": FS, "channels": CH, "clips": CLIPS, "seconds": SECONDS, "rounds": args.rounds, "timed_per_round": args.timed,
           "unit": "ms per call, median of a round"}
    if args.label:
        doc["build"] = args.label
    for name in builds:
        doc[name] = {leg: [c[leg] for c in rounds[name]] for leg in EQUAL_LEGS + RAGGED_LEGS if leg in rounds[name][0]}
    if "parent" in builds:
        doc["equal_length_path"] = {}
        for leg in EQUAL_LEGS:
            lo, hi = min(doc["parent"][leg]), max(doc["parent"][leg])
            worst = max(max(v - hi, lo - v, 0.0) for v in doc["this"][leg])
            slower = max(max(v - hi, 0.0) for v in doc["this"][leg])
            doc["equal_length_path"][leg] = {"parent_range": [lo, hi], "this": doc["this"][leg], "inside_parent_range": worst == 0.0,
                                             "worst_round_outside_by_ms": round(worst, 4),
                                             "worst_round_above_parent_range_by_ms": round(slower, 4),
                                             "ratio_of_medians": round(float(np.median(doc["this"][leg]) / np.median(doc["parent"][leg])), 4)}
    if "ragged_batch" in doc["this"]:
        batch, loop = float(np.median(doc["this"]["ragged_batch"])), float(np.median(doc["this"]["ragged_loop"]))
        doc["ragged_batch_against_loop"] = {"ragged_batch_ms": batch, "ragged_loop_ms": loop, "loop_over_batch": round(loop / batch, 3),
                                            "ragged_over_equal": round(batch / float(np.median(doc["this"]["equal_simonline"])), 3)}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
