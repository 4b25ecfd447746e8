"""bench.py: what a plain run times and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import MANIFEST, ROOT


def _packed(rgb):
    """0x00RRGGBB pixels back from the dumped float32 channels."""
    c = rgb.astype(np.uint32)
    return (c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]


def test_dump_outputs_whole_frames_and_seeded_samples(tmp_path):
    import torch
    import bench
    rng = np.random.default_rng(7)
    small = torch.from_numpy(rng.integers(0, 1 << 24, (93, 157)).astype(np.int32))
    bench.dump_outputs(str(tmp_path / "small"), [small])
    rgb = np.load(tmp_path / "small" / "frame.npy")
    assert rgb.dtype == np.float32 and rgb.shape == (93, 157, 3)
    assert (_packed(rgb) == small.numpy().view(np.uint32)).all()

    # four 1080p frames: over the budget, so each is cut to the same seeded sample of pixels
    big = [torch.from_numpy(rng.integers(0, 1 << 24, (1080, 1920)).astype(np.int32)) for _ in range(4)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted([f"frame{f}.npy" for f in range(4)] + [f"frame{f}_sample_index.npy" for f in range(4)])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10 ** 6
    for f in range(4):
        idx = np.load(tmp_path / "a" / f"frame{f}_sample_index.npy")
        rgb = np.load(tmp_path / "a" / f"frame{f}.npy")
        assert rgb.dtype == np.float32 and idx.dtype == np.float64 and rgb.shape == (idx.size, 3)
        assert (np.diff(idx) > 0).all()
        assert (_packed(rgb) == big[f].numpy().view(np.uint32).ravel()[idx.astype(np.int64)]).all()
        assert (np.load(tmp_path / "b" / f"frame{f}_sample_index.npy") == idx).all()


@pytest.mark.gpu
def test_gpu_plain_bench_run_times_its_steps_and_dumps_the_reference_frame(qr, tmp_path):
    """A plain run times exactly --steps steps, carries none of --full's figures, and the frame its last timed step
    rendered (--dump-outputs) is the reference's frame of the workload."""
    steps = 40
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "3",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert j["steps"] == steps and j["unit"] == "Mrays/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["timing"]["timed_region_ms"] == pytest.approx(steps * j["ms_per_step"])
    assert j["value"] == pytest.approx(j["config"]["rays_per_frame"] * steps / (j["timing"]["timed_region_ms"] * 1e-3) / 1e6)
    assert "roofline" not in j and "cpu_baseline" not in j and "frame_check" not in j["config"]
    rgb = np.load(tmp_path / "frame.npy")
    assert rgb.dtype == np.float32 and rgb.shape == (1080, 1920, 3)
    assert qr.frame_hash(_packed(rgb)) == int(MANIFEST["c2b_demo01_1080p"]["hash"], 16)
