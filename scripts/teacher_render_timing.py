"""The teacher renderer's kernels (teacher.render_teacher: six HIP launches) against the composition available without them
(teacher.render_teacher_torch: the fused field kernel plus ~40 torch ops), on the reference's workload: planes
[3, 3, 256, 256, 32] with the PanoHead axes, one camera at radius 2.7, 64^2 and 128^2 rays, 48 + 48 samples, crop 0.1.
python scripts/teacher_render_timing.py [--rounds R] [--iters I] [--resolutions 64 128]

The two are ALTERNATED: each round times `iters` back-to-back calls of one (device events around the batch, after 3 warm-up
calls), then of the other; R rounds (default 6) of I = 200 calls.  The noise is fixed and generated outside the timed window, the
rays likewise.  Reported per form: the median over the rounds of the per-call time, the range, peak memory of one call above
what is allocated before it (the kernels' workspace is the context's, allocated once and not torch's: reported separately as
workspace_mb), and the largest differences between the two results.  One JSON line per resolution."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gaussian_gan_decoder_amd import density, teacher  # noqa: E402
from density_timing import batch_ms, peak_mb  # noqa: E402


def camera(radius=2.7, azimuth=0.4, elevation=0.15, fov=18.0):
    eye = radius * torch.tensor([math.cos(elevation) * math.sin(azimuth), math.sin(elevation), math.cos(elevation) * math.cos(azimuth)])
    fwd = -eye / eye.norm()
    right = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0]), fwd)
    right = right / right.norm()
    up = torch.linalg.cross(fwd, right)
    m = torch.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, fwd, eye
    f = 1.0 / (2.0 * math.tan(math.radians(fov) / 2.0))
    return m[None], torch.tensor([[[f, 0.0, 0.5], [0.0, f, 0.5], [0.0, 0.0, 1.0]]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--samples", type=int, nargs=2, default=[48, 48])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("teacher_render_timing.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    planes_cl = torch.randn(3, args.depth, args.size, args.size, 32, generator=g).to(dev)
    w = density.osg_weights(torch.randn(64, 32, generator=g) / 32 ** 0.5, 0.5 * torch.randn(64, generator=g),
                            torch.randn(33, 64, generator=g) / 8.0, 0.5 * torch.randn(33, generator=g)).to(dev)
    Nc, Ni = args.samples
    kw = dict(ray_start=2.25, ray_end=3.3, depth_resolution=Nc, depth_resolution_importance=Ni, box_warp=1.0, plane_axes="panohead",
              triplane_depth=args.depth, triplane_crop=0.1)
    cam2world, intrinsics = camera()
    for res in args.resolutions:
        origins, dirs = (t.to(dev) for t in teacher.camera_rays(cam2world, intrinsics, res))
        M = origins.shape[0]
        noise = (torch.rand(M, Nc, generator=g).to(dev), torch.rand(M, Ni, generator=g).to(dev))
        fused = lambda: teacher.render_teacher(planes_cl, w, origins, dirs, noise=noise, **kw)
        composed = lambda: teacher.render_teacher_torch(planes_cl, w, origins, dirs, noise=noise, **kw)
        a, b = fused(), composed()
        diff = {k: float((getattr(a, k) - getattr(b, k)).abs().max()) for k in ("features", "depth", "weights")}
        del a, b
        mem = {"fused": peak_mb(fused), "composed": peak_mb(composed)}
        ms = {"fused": [], "composed": []}
        for _ in range(args.rounds):
            ms["fused"].append(batch_ms(fused, args.iters))
            ms["composed"].append(batch_ms(composed, args.iters))
        res_line = {"rays": M, "samples": [Nc, Ni], "planes": list(planes_cl.shape), "rounds": args.rounds, "iters": args.iters,
                    "max_abs_diff": diff, "workspace_mb": round((teacher.sample_layout(M, Nc, Ni)[2] + 2 * M) * 4 / 2 ** 20, 1)}
        for k in ms:
            res_line[k] = {"median_ms": round(statistics.median(ms[k]), 4), "min_ms": round(min(ms[k]), 4),
                           "max_ms": round(max(ms[k]), 4), "peak_mb": round(mem[k], 1)}
        res_line["speedup"] = round(res_line["composed"]["median_ms"] / res_line["fused"]["median_ms"], 3)
        print(json.dumps(res_line), flush=True)


if __name__ == "__main__":
    main()
