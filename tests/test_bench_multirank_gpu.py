"""bench.py's multi-rank control flow (barriers, rank-0-only sections, the data-parallel train step with its flat
all-reduce) with two ranks sharing the one visible GPU over gloo (GGD_BENCH_SHARE_GPU=1 test hook): it must finish and
print exactly one JSON line with the aggregate of both ranks.  The real 2/4/8-GPU runs use RCCL and one GPU per rank."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_two_ranks_on_one_gpu(native_lib):
    env = dict(os.environ, GGD_BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29547", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20",
           "--warmup", "3", "--full", "--workload", "100k_512_cube", "--train-iters", "2", "--train-points", "20000",
           "--scenes-per-gpu", "2", "--no-decode", "--no-sweep", "--no-cpu-baseline"]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 20 and d["value"] > 0
    assert d["train_fused_decoder"]["iters_per_s"] > 0
    # 8-GPU readiness (BASELINE config 5): every train section, in both plane formats, all-reduces the reference's payload --
    # decoder + planes + backbone stand-in = 29 763 294 fp32 gradients, each exactly once -- and at least 75 % of those bytes
    # were handed to the collective from inside the backward (gradient hooks), not after it
    for key in ("train", "train_fused_decoder", "train_fused_decoder_fp32"):
        for sec in (d[key], d[key]["eg3d_planes"]):
            assert sec["global_batch"] == 4
            assert sec["parameters_all_reduced"] == 29_763_294, (key, sec["planes"])
            assert sec["allreduce_bytes"] == 4 * 29_763_294, (key, sec["planes"], sec["allreduce_bytes"])
            assert sec["allreduce_bytes_launched_in_backward"] >= 0.75 * sec["allreduce_bytes"], (key, sec["planes"])
            assert sec["allreduce_exposed_ms"] >= 0.0
    assert "PanoHead" in d["train"]["planes"] and "EG3D" in d["train"]["eg3d_planes"]["planes"]
    wf = d["whole_frame"]
    assert 0 < wf["algorithmic_bytes_path"] < wf["contract_formula_bytes"]
