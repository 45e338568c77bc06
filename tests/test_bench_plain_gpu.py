"""bench.py without --full: one JSON line with the headline and nothing that takes runs of its own; --dump-outputs writes
the last timed frame, and two runs with the same arguments write the same frame."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
           "--workload", "100k_512_cube", "--dump-outputs", str(out_dir)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs(native_lib, tmp_path):
    a, b = _plain_run(tmp_path / "a"), _plain_run(tmp_path / "b")
    for d in (a, b):
        assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["steps"] == 7 and d["value"] > 0
        assert d["ms_per_step"] == pytest.approx(d["timed_region_s"] * 1e3 / 7)
        assert d["value"] == pytest.approx(1e3 / d["ms_per_step"])
        assert d["timed_path"]["two_launch_sort_frames_timed"] + d["timed_path"]["ordinary_sort_frames_timed"] == 7
        for key in ("roofline", "stage_ms", "verified_vs_two_call", "train", "decode_render", "cpu_baseline", "extra"):
            assert key not in d, key
    files = {}
    for name in ("color", "radii", "num_rendered"):
        fa, fb = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert fa.dtype in (np.float32, np.float64) and fa.dtype == fb.dtype and fa.shape == fb.shape
        assert np.array_equal(fa, fb), name
        files[name] = fa
    assert files["color"].shape == (3, 512, 512) and np.isfinite(files["color"]).all()
    assert files["radii"].shape == (100_000,) and (files["radii"] >= 0).all() and (files["radii"] > 0).any()
    assert files["num_rendered"].shape == (1,) and int(files["num_rendered"][0]) == a["config"]["num_rendered"] > 0
