"""bench.py's plain run and its --dump-outputs files (the --full line is covered by test_gpu_dist.py's bench tests)."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bench
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_the_whole_frame_or_a_fixed_sample(tmp_path):
    rng = np.random.default_rng(5)
    small = rng.integers(0, 256, (1080, 1920, 4), dtype=np.uint8)
    d = bench.dump_outputs(str(tmp_path / "small"), small)
    got = np.load(tmp_path / "small" / "frame.npy")
    assert d["frame"] == [1080, 1920, 4] and got.dtype == np.float32 and np.array_equal(got, small)
    # config 5's frame (4096 x 4096 RGBA) is too large as float32: a seeded sample of its pixels, the same on every run
    big = rng.integers(0, 256, (4096, 4096, 4), dtype=np.uint8)
    samples = []
    for name in ("a", "b"):
        d = bench.dump_outputs(str(tmp_path / name), big)
        files = sorted(os.listdir(tmp_path / name))
        assert files == ["frame_sample.npy", "frame_sample_pixels.npy"]
        assert sum(os.path.getsize(tmp_path / name / f) for f in files) <= 64 << 20
        px = np.load(tmp_path / name / "frame_sample_pixels.npy")
        vals = np.load(tmp_path / name / "frame_sample.npy")
        assert px.dtype == np.float64 and vals.dtype == np.float32 and d["frame_sample"] == list(vals.shape)
        assert np.all(np.diff(px) > 0) and np.array_equal(vals, big.reshape(-1, 4)[px.astype(np.int64)])
        samples.append(px)
    assert np.array_equal(samples[0], samples[1])


@pytest.mark.gpu
def test_plain_bench_times_exactly_its_steps_and_dumps_the_oracle_frame(tmp_path):
    # A plain run: the headline only, ONE repetition of exactly --steps steps, and the frame its last timed step left -- which must be
    # the committed oracle vector's 1080p frame (tests/golden/oracle_vectors.json config3_1920x1080_f32).
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=util.product_env(), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, "bench.py must print exactly one line"
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 7 and d["repeats"]["n"] == 1 and d["full"] is False and d["value"] > 1000
    assert d["repeats"]["ms_per_step_each"] == [d["ms_per_step"]]
    for k in ("roofline", "flat", "configs", "frames_in_flight", "first_frame", "seam", "make_image", "cpu_baseline", "frame_crc_ok"):
        assert k not in d, "%s belongs to --full" % k
    assert d["outputs"]["frame"] == [1080, 1920, 4] and sorted(os.listdir(out)) == ["frame.npy"]
    frame = np.load(out / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (1080, 1920, 4)
    assert zlib.crc32(frame.astype(np.uint8).tobytes()) & 0xFFFFFFFF == 4168428064
