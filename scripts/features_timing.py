"""Cost of a 32-channel feature map: forward and forward + backward of three variants, alternated in one process.
python scripts/features_timing.py [--iters N] [--channels C]

Scene: 500 k Gaussians at 512^2 on a head-like shell (the train step's shape, the scene of scripts/depth_alpha_timing.py).
  plain      a render without features                                             (what a frame costs today)
  features   the same render with features=[P, C]                                  (one more launch each way)
  composed   ceil(C / 3) renders with colors_precomp = a channel triple each       (how the same map is produced without the keyword;
                                                                                    runs on a build without it as well)
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
    iters, Cn, S, P = arg("--iters", 20), arg("--channels", 32), 512, 500_000
    dev = torch.device("cuda:0")
    sc = make_scene(P, S, "shell", seed=3, h=math.pi / 2 + 0.6).to(dev)
    cam, e = sc.cam, torch.empty(0, device=dev)
    gen = torch.Generator().manual_seed(1)
    feats = torch.rand(P, Cn, generator=gen).to(dev)
    fbg = torch.rand(Cn, generator=gen).to(dev)
    g = torch.randn(3, S, S, generator=gen).to(dev)
    gF = torch.randn(Cn, S, S, generator=gen).to(dev)
    nt = (Cn + 2) // 3
    pad = torch.zeros(P, 3 * nt - Cn, device=dev)
    triples = [t.contiguous() for t in torch.cat([feats, pad], 1).split(3, dim=1)]
    bgs = [t.contiguous() for t in torch.cat([fbg, torch.zeros(3 * nt - Cn, device=dev)]).split(3)]
    gts = [t.contiguous() for t in torch.cat([gF, torch.zeros(3 * nt - Cn, S, S, device=dev)]).split(3)]
    op, scl, rot, dc = sc.opacities.contiguous(), sc.scales.contiguous(), sc.rotations.contiguous(), sc.features_dc.contiguous()
    tan = (math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5))

    def forward(bg, colors, sh, **kw):
        return R.rasterize_gaussians_native(bg, sc.xyz, colors, op, scl, rot, 1.0, e, cam.world_view_transform,
                                            cam.full_proj_transform, tan[0], tan[1], S, S, sh, 0, cam.camera_center, False, False, **kw)

    def backward(out, bg, colors, sh, grad, **kw):
        n, _, radii, geom, binning, img = out[:6]
        return R.rasterize_gaussians_backward_native(bg, sc.xyz, radii, colors, scl, rot, 1.0, e, cam.world_view_transform,
                                                     cam.full_proj_transform, tan[0], tan[1], grad, sh, 0, cam.camera_center, geom, n,
                                                     binning, img, False, **kw)

    def plain(bwd):
        out = forward(sc.bg, e, dc)
        if bwd:
            backward(out, sc.bg, e, dc, g)

    def features(bwd):
        out = forward(sc.bg, e, dc, features=feats, feature_bg=fbg)
        if bwd:
            backward(out, sc.bg, e, dc, g, features=feats, feature_bg=fbg, dL_dfeatmap=gF)

    def composed(bwd):
        for t, b, gt in zip(triples, bgs, gts):
            out = forward(b, t, e)
            if bwd:
                backward(out, b, t, e, gt)

    variants = dict(plain=plain, composed=composed)
    if "features" in inspect.signature(R.rasterize_gaussians_native).parameters:
        variants["features"] = features

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
    res = dict(scene="500k head-like shell 512^2", channels=Cn, renders_composed=nt, iters=iters, ms=med)
    if "features" in med:
        res["composed_over_features"] = {m: round(med["composed"][m] / med["features"][m], 2) for m in med["features"]}
        res["features_minus_plain_ms"] = {m: round(med["features"][m] - med["plain"][m], 3) for m in med["features"]}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
