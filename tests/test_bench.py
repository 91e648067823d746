"""bench.py's own contract: a plain run prints the headline fields and nothing that needs work of its own, --full adds the other
figures without changing what the timed steps compute, and --dump-outputs writes the image of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "calibration", "kernel", "nonparity_throughput_mode", "cpu_baseline", "host_loop")


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "one JSON line"
    return json.loads(lines[0])


def test_dump_of_a_large_frame_is_a_fixed_sample(tmp_path):
    import torch
    img = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(2000, 2100, 4), dtype=np.uint8))  # 67 MB as float32
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), img)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["rgba.npy", "rgba_pixels.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64e6
    rgba, idx = np.load(tmp_path / "a" / "rgba.npy"), np.load(tmp_path / "a" / "rgba_pixels.npy")
    assert rgba.dtype == np.float32 and idx.dtype == np.float64 and np.unique(idx).size == idx.size
    assert (rgba == img.numpy().reshape(-1, 4)[idx.astype(np.int64)]).all()
    for f in files:
        assert (np.load(tmp_path / "a" / f) == np.load(tmp_path / "b" / f)).all(), "the sample is the same from run to run"
    small = img[:112, :200]
    bench.dump_outputs(str(tmp_path / "a"), small)
    assert os.listdir(tmp_path / "a") == ["rgba.npy"]
    assert (np.load(tmp_path / "a" / "rgba.npy") == small.numpy().astype(np.float32)).all()


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_last_timed_step(tmp_path, oracle):
    from mort_amd import host
    args = ["--steps", "2", "--warmup", "1", "--width", "200", "--spp", "4"]
    plain = _bench(*args, "--dump-outputs", str(tmp_path / "plain"))
    assert all(k in plain for k in HEADLINE) and plain["steps"] == 2 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert not any(k in plain for k in FULL_ONLY)
    full = _bench(*args, "--full", "--dump-outputs", str(tmp_path / "full"))
    assert all(k in full for k in HEADLINE + FULL_ONLY)
    # states persist from frame to frame: the last timed step is frame warmup + steps of the seeded sequence
    world, cam = host.build_scene(1, width=200, spp=4)
    states = oracle.seed_states(69420, cam.image_width, cam.image_height)
    for _ in range(1 + 2):
        ref = oracle.render(world, cam, states=states, nthreads=8, want_accum=False, want_segments=False)["rgba"]
    for d in ("plain", "full"):
        got = np.load(tmp_path / d / "rgba.npy")
        assert got.dtype == np.float32 and got.shape == ref.shape and (got == ref).all(), d
