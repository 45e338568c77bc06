"""Cost of the depth / alpha extension: blend forward and blend backward stage times (ggd_stage_times) with the extension off
and on, alternating in one process.  python scripts/depth_alpha_timing.py [--iters N]

Scenes: 1 M Gaussians at 1024^2 (cube) and the train step's shape, 500 k Gaussians at 512^2 on a head-like shell.  Prints one
JSON line per scene: median milliseconds of each stage per mode and the on / off ratios."""
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
    gen = torch.Generator().manual_seed(1)
    gD, gA = torch.randn(1, S, S, generator=gen).to(dev), torch.randn(1, S, S, generator=gen).to(dev)
    ctx = _capi.context_for(dev)

    def frame(aux):
        out = R.rasterize_gaussians_native(*args, render_depth_alpha=aux)
        n, color, radii, geom, binning, img = out[:6]
        kw = dict(dL_ddepth=gD, dL_dalpha=gA) if aux else {}
        R.rasterize_gaussians_backward_native(args[0], args[1], radii, args[2], args[4], args[5], 1.0, args[7], args[8],
                                              args[9], args[10], args[11], g, args[14], 0, args[16], geom, n, binning, img,
                                              False, **kw)
        torch.cuda.synchronize()
        return ctx.stage_times()

    for _ in range(5):
        frame(False), frame(True)
    ctx.set_profiling(True)
    t = {m: {"blend": [], "blend_bwd": []} for m in ("off", "on")}
    for _ in range(iters):
        for m in ("off", "on"):
            st = frame(m == "on")
            for k in t[m]:
                t[m][k].append(st[k])
    ctx.set_profiling(False)
    med = {m: {k: round(statistics.median(v), 4) for k, v in t[m].items()} for m in t}
    print(json.dumps(dict(scene=name, ms=med, fwd_ratio=round(med["on"]["blend"] / med["off"]["blend"], 3),
                          bwd_ratio=round(med["on"]["blend_bwd"] / med["off"]["blend_bwd"], 3))), flush=True)


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 30
    dev = torch.device("cuda:0")
    measure("1M cube 1024^2", make_scene(1_000_000, 1024, "cube", seed=0).to(dev), 1024, dev, iters)
    measure("500k head-like shell 512^2", make_scene(500_000, 512, "shell", seed=3, h=math.pi / 2 + 0.6).to(dev), 512, dev,
            iters)


if __name__ == "__main__":
    main()
