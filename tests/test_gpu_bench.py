"""bench.py on one GPU, as a child process: a plain run takes exactly --steps timed steps and prints the headline line only;
--dump-outputs writes what the timed call computed, and two runs with the same arguments write the same arrays; --full adds
the studies (stage times, roofline, CPU baseline) over the same frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

STEPS = 6
ARGS = ["--gpus", "1", "--scene", "cornell", "--width", "320", "--height", "184", "--steps", str(STEPS), "--warmup", "2", "--no-obj-roundtrip"]
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"traverse_mrays_s", "stage_ms_per_frame", "roofline", "cpu_baseline"}


def _bench(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + list(extra), capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_times_its_steps_and_dumps_the_same_outputs_twice(tmp_path):
    lines = [_bench("--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for line in lines:
        assert HEADLINE <= set(line) and not FULL_ONLY & set(line)
        assert line["steps"] == STEPS and line["timing"]["repeats"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["frame_rays.npy", "frame_rounds.npy", "image.npy"] and sorted(os.listdir(tmp_path / "b")) == files
    a = {f: np.load(tmp_path / "a" / f) for f in files}
    b = {f: np.load(tmp_path / "b" / f) for f in files}
    assert a["image.npy"].shape == (184, 320, 4) and a["image.npy"].dtype == np.float32
    assert a["frame_rays.npy"].shape == (STEPS,) and a["frame_rays.npy"].dtype == np.float64
    assert a["frame_rays.npy"].sum() == round(lines[0]["rays_per_frame"] * STEPS)
    assert float(a["image.npy"][..., :3].mean()) == pytest.approx(lines[0]["image_mean"], rel=1e-6)
    assert np.array_equal(a["frame_rays.npy"], b["frame_rays.npy"]) and np.array_equal(a["frame_rounds.npy"], b["frame_rounds.npy"])
    np.testing.assert_allclose(b["image.npy"], a["image.npy"], rtol=1e-4, atol=1e-5)   # float atomics: deposit order only


def test_full_run_adds_the_studies_over_the_same_frames(tmp_path):
    plain, full = _bench("--dump-outputs", str(tmp_path / "p")), _bench("--full", "--dump-outputs", str(tmp_path / "f"))
    assert FULL_ONLY <= set(full) and full["timing"]["repeats"] == 5 and full["cpu_baseline"]["value"] > 0
    assert full["rays_per_frame"] == plain["rays_per_frame"]
    np.testing.assert_allclose(np.load(tmp_path / "f" / "image.npy"), np.load(tmp_path / "p" / "image.npy"), rtol=1e-4, atol=1e-5)
