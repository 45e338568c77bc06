"""Cost of the anti-aliasing option (ggd_params.antialiasing): the per-Gaussian stages (preprocess forward and backward, from
ggd_stage_times) and the whole forward + backward (device events around the frame, stage timers off), with the option off and
on, alternating in one process.  python scripts/antialiasing_timing.py [--iters N]

Scenes: 1 M Gaussians at 1024^2 (cube) and the train step's shape, 500 k Gaussians at 512^2 on a head-like shell.  Prints one
JSON line per scene: median milliseconds per mode and the on / off ratios."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gaussian_gan_decoder_amd import _capi, rasterizer as R  # noqa: E402
from gaussian_gan_decoder_amd.synthetic import make_dL_dpix, make_scene  # noqa: E402


def scene_args(sc, S, dev):
    cam, e = sc.cam, torch.empty(0, device=dev)
    return (sc.bg, sc.xyz, e, sc.opacities.contiguous(), sc.scales.contiguous(), sc.rotations.contiguous(), 1.0, e,
            cam.world_view_transform, cam.full_proj_transform, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), S, S,
            sc.features_dc.contiguous(), 0, cam.camera_center, False, False)


def measure(name, sc, S, dev, iters):
    args = scene_args(sc, S, dev)
    g = make_dL_dpix(S).to(dev)
    ctx = _capi.context_for(dev)

    def frame(aa):
        n, color, radii, geom, binning, img = R.rasterize_gaussians_native(*args, antialiasing=aa)
        R.rasterize_gaussians_backward_native(args[0], args[1], radii, args[2], args[4], args[5], 1.0, args[7], args[8],
                                              args[9], args[10], args[11], g, args[14], 0, args[16], geom, n, binning, img,
                                              False, False, args[3], antialiasing=aa)

    for _ in range(10):
        frame(False), frame(True)
    torch.cuda.synchronize()
    stages = ("preprocess", "preprocess_bwd")
    t = {m: {k: [] for k in stages + ("fwd_bwd",)} for m in ("off", "on")}
    ctx.set_profiling(True)
    for _ in range(iters):
        for m in ("off", "on"):
            frame(m == "on")
            torch.cuda.synchronize()
            st = ctx.stage_times()
            for k in stages:
                t[m][k].append(st[k])
    ctx.set_profiling(False)
    for _ in range(iters):
        for m in ("off", "on"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            frame(m == "on")
            b.record()
            b.synchronize()
            t[m]["fwd_bwd"].append(a.elapsed_time(b))
    med = {m: {k: round(statistics.median(v), 4) for k, v in t[m].items()} for m in t}
    ratio = {k: round(med["on"][k] / med["off"][k], 3) for k in med["on"]}
    print(json.dumps(dict(scene=name, iters=iters, ms=med, ratio=ratio)), flush=True)


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 30
    dev = torch.device("cuda:0")
    measure("1M cube 1024^2", make_scene(1_000_000, 1024, "cube", seed=0).to(dev), 1024, dev, iters)
    measure("500k head-like shell 512^2", make_scene(500_000, 512, "shell", seed=3, h=math.pi / 2 + 0.6).to(dev), 512, dev,
            iters)


if __name__ == "__main__":
    main()
