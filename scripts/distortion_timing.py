"""Cost of the depth-distortion map: forward and forward + backward of two variants, alternated in one process.
python scripts/distortion_timing.py [--iters N]

Scene: 500 k Gaussians at 512^2 on a head-like shell (the train step's shape, the scene of scripts/features_timing.py).
  depth_alpha   a render with render_depth_alpha=True                  (what the geometry-supervised frame costs today; runs on a
                                                                       build without the keyword as well)
  distortion    the same render with render_distortion=True            (one more launch each way)
Times are HIP-event milliseconds around the whole call sequence of a variant (launches, allocations and the host's waits for
num_rendered included), median over the iterations; the backward's upstream gradients are N(0, 1) on every map.  Prints one JSON
line."""
import inspect
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gaussian_gan_decoder_amd import rasterizer as R  # noqa: E402
from gaussian_gan_decoder_amd.synthetic import make_scene  # noqa: E402


def main():
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    iters, S, P = arg("--iters", 15), 512, 500_000
    dev = torch.device("cuda:0")
    sc = make_scene(P, S, "shell", seed=3, h=math.pi / 2 + 0.6).to(dev)
    cam, e = sc.cam, torch.empty(0, device=dev)
    gen = torch.Generator().manual_seed(1)
    g = torch.randn(3, S, S, generator=gen).to(dev)
    gD, gA, gX = (torch.randn(1, S, S, generator=gen).to(dev) for _ in range(3))
    op, scl, rot, dc = sc.opacities.contiguous(), sc.scales.contiguous(), sc.rotations.contiguous(), sc.features_dc.contiguous()
    tan = (math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5))

    def forward(**kw):
        return R.rasterize_gaussians_native(sc.bg, sc.xyz, e, op, scl, rot, 1.0, e, cam.world_view_transform,
                                            cam.full_proj_transform, tan[0], tan[1], S, S, dc, 0, cam.camera_center, False, False,
                                            render_depth_alpha=True, **kw)

    def backward(out, **kw):
        n, _, radii, geom, binning, img = out[:6]
        return R.rasterize_gaussians_backward_native(sc.bg, sc.xyz, radii, e, scl, rot, 1.0, e, cam.world_view_transform,
                                                     cam.full_proj_transform, tan[0], tan[1], g, dc, 0, cam.camera_center, geom, n,
                                                     binning, img, False, dL_ddepth=gD, dL_dalpha=gA, **kw)

    def depth_alpha(bwd):
        out = forward()
        if bwd:
            backward(out)

    def distortion(bwd):
        out = forward(render_distortion=True)
        if bwd:
            backward(out, dL_ddistortion=gX)

    variants = dict(depth_alpha=depth_alpha)
    if "render_distortion" in inspect.signature(R.rasterize_gaussians_native).parameters:
        variants["distortion"] = distortion

    def timed(fn, bwd):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn(bwd)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for _ in range(3):
        for fn in variants.values():
            fn(True)
    ms = {k: {"forward": [], "forward_backward": []} for k in variants}
    for _ in range(iters):
        for k, fn in variants.items():
            ms[k]["forward"].append(timed(fn, False))
            ms[k]["forward_backward"].append(timed(fn, True))
    med = {k: {m: round(statistics.median(v), 3) for m, v in t.items()} for k, t in ms.items()}
    spread = {k: {m: round(max(v) - min(v), 3) for m, v in t.items()} for k, t in ms.items()}
    res = dict(scene="500k head-like shell 512^2", iters=iters, ms=med, max_minus_min_ms=spread)
    if "distortion" in med:
        res["distortion_over_depth_alpha"] = {m: round(med["distortion"][m] / med["depth_alpha"][m], 3) for m in med["distortion"]}
        res["distortion_minus_depth_alpha_ms"] = {m: round(med["distortion"][m] - med["depth_alpha"][m], 3) for m in med["distortion"]}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
