"""bench.py's contract: a plain run times exactly --steps steps and measures nothing else; --dump-outputs writes what the
timed path returned in its last step (float32, at most 64 MB in all, a fixed sample of anything larger)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_or_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 400_000)
    rs = np.random.RandomState(0)
    small = rs.standard_normal((1000, 2))
    bench.dump_outputs(str(tmp_path / "a"), {"background": small})
    assert sorted(os.listdir(tmp_path / "a")) == ["background.npy"]
    got = np.load(tmp_path / "a" / "background.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.astype(np.float32))

    large = rs.standard_normal((3, 40000, 2))
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"background": large})
    assert sorted(os.listdir(tmp_path / "b")) == ["background.npy", "background_frames.npy"]
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 400_000
    frames = np.load(tmp_path / "b" / "background_frames.npy")
    sample = np.load(tmp_path / "b" / "background.npy")
    assert frames.dtype == np.float64 and np.all(np.diff(frames) > 0) and len(frames) > 10000
    assert np.array_equal(sample, large.reshape(-1, 2)[frames.astype(np.int64)].astype(np.float32))
    for f in ("background.npy", "background_frames.npy"):                  # the same sample every time
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f))


@pytest.mark.gpu
def test_plain_run_times_exactly_the_steps_and_dumps_the_last_result(tmp_path):
    import repet
    from repet_synth import synth
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--duration", "20", "--prewarm-ms", "5", "--dump-outputs", str(tmp_path / "out")],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout[-2000:]
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and len(line["series_ms_per_step"]) == 1 and line["ms_per_step"] > 0
    for key in ("cpu_baseline", "array_in_array_out", "fp32_gemm_variant", "three_clips_in_flight", "scatter_gather"):
        assert key not in line, key                                         # (--full only)
    assert os.listdir(tmp_path / "out") == ["background.npy"]
    got = np.load(tmp_path / "out" / "background.npy")
    want = repet.sim(synth(20.0, 44100, 2, seed=0), 44100)
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
