"""Cost of the per-Gaussian contribution statistics: a frame with and without the keyword, the launch alone, and the one
alternative that exists without it, alternated in one process.
python scripts/contribution_timing.py [--iters N]

Scene: 500 k Gaussians at 512^2 on a head-like shell (the train step's shape, the scene of scripts/features_timing.py).
  plain          a forward without the keyword                                        (what a frame costs today)
  contribution   the same forward with contribution=raw                               (one more launch)
  via_backward   the forward, then a backward under an all-ones image gradient        (the only way to the SUM without the keyword:
                                                                                       dL_dcolors[:, 0] = sum alpha T; float atomics,
                                                                                       not reproducible; max and count have no
                                                                                       alternative at all)
  launch         ggd_contribution alone on the buffers of a finished forward          (device time of the new kernel)
Times are HIP-event milliseconds around the whole call sequence of a variant (launches, allocations and the host's waits for
num_rendered included), median over the iterations.  Prints one JSON line."""
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gaussian_gan_decoder_amd import _capi  # noqa: E402
from gaussian_gan_decoder_amd import rasterizer as R  # noqa: E402
from gaussian_gan_decoder_amd.contribution import ContributionStats  # noqa: E402
from gaussian_gan_decoder_amd.synthetic import make_scene  # noqa: E402


def main():
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    iters, S, P = arg("--iters", 20), 512, 500_000
    dev = torch.device("cuda:0")
    sc = make_scene(P, S, "shell", seed=3, h=math.pi / 2 + 0.6).to(dev)
    cam, e = sc.cam, torch.empty(0, device=dev)
    ones = torch.ones(3, S, S, device=dev)
    op, scl, rot, dc = sc.opacities.contiguous(), sc.scales.contiguous(), sc.rotations.contiguous(), sc.features_dc.contiguous()
    tan = (math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5))
    stats = ContributionStats(P, dev)

    def forward(**kw):
        return R.rasterize_gaussians_native(sc.bg, sc.xyz, e, op, scl, rot, 1.0, e, cam.world_view_transform, cam.full_proj_transform,
                                            tan[0], tan[1], S, S, dc, 0, cam.camera_center, False, False, **kw)

    def plain():
        forward()

    def contribution():
        forward(contribution=stats.raw)

    def via_backward():
        n, _, radii, geom, binning, img = forward()[:6]
        return R.rasterize_gaussians_backward_native(sc.bg, sc.xyz, radii, e, scl, rot, 1.0, e, cam.world_view_transform,
                                                     cam.full_proj_transform, tan[0], tan[1], ones, dc, 0, cam.camera_center, geom, n,
                                                     binning, img, False)[1]

    out = forward()
    cx, stream = _capi.context_and_stream(dev)
    rs = R.GaussianRasterizationSettings(S, S, tan[0], tan[1], sc.bg, 1.0, cam.world_view_transform, cam.full_proj_transform, 0,
                                         cam.camera_center, False, False)
    keep = []
    prm = R._params(rs, P, 1, dev, keep)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def launch():
        cx.check(cx.lib.ggd_contribution(cx.handle, C.c_void_p(stream), C.byref(prm), ptr(out[3]), ptr(out[4]), ptr(out[5]), out[0],
                                         ptr(stats.raw)))

    variants = dict(plain=plain, contribution=contribution, via_backward=via_backward, launch=launch)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for _ in range(3):
        for fn in variants.values():
            fn()
    # the sum two ways: the fixed-point statistic of one frame against dL_dcolors under the all-ones gradient
    stats.reset()
    contribution()
    torch.cuda.synchronize()
    by_backward = via_backward()[:, 0].double()
    sum_gap = float((stats.weight_sum - by_backward).abs().max())
    used = int((stats.pixel_count > 0).sum())
    pairs = int(stats.pixel_count.sum())
    ms = {k: [] for k in variants}
    for _ in range(iters):
        for k, fn in variants.items():
            ms[k].append(timed(fn))
    med = {k: round(statistics.median(v), 3) for k, v in ms.items()}
    res = dict(scene="500k head-like shell 512^2", iters=iters, num_rendered=int(out[0]), rows_used=used, pairs=pairs, ms=med,
               contribution_minus_plain_ms=round(med["contribution"] - med["plain"], 3),
               via_backward_minus_plain_ms=round(med["via_backward"] - med["plain"], 3),
               max_gap_sum_vs_backward=sum_gap)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
