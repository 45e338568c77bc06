"""Cost of the camera's gradients: the backward with and without camera_grad=True, alternated in one process.
python scripts/camera_grad_timing.py [--iters N]

Scene: 500 k Gaussians at 512^2 on a head-like shell (the train step's shape, the scene of scripts/distortion_timing.py), SH degree
0, one forward whose buffers both variants read.
  plain    rasterize_gaussians_backward_native(...)                      (ggd_backward)
  camera   the same call with camera_grad=True                           (ggd_backward_camera: two more launches)
Times are HIP-event milliseconds.  `call`: around one call (launches, allocations and the host's work included), median over the
iterations.  `batch`: around 20 calls back to back, divided by 20 -- the host runs ahead of the device, so this is the device's
time per call, and camera - plain of it is the two added launches' own time.  Prints one JSON line."""
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
    iters, S, P, batch = arg("--iters", 15), 512, 500_000, 20
    dev = torch.device("cuda:0")
    sc = make_scene(P, S, "shell", seed=3, h=math.pi / 2 + 0.6).to(dev)
    cam, e = sc.cam, torch.empty(0, device=dev)
    g = torch.randn(3, S, S, generator=torch.Generator().manual_seed(1)).to(dev)
    op, scl, rot, dc = sc.opacities.contiguous(), sc.scales.contiguous(), sc.rotations.contiguous(), sc.features_dc.contiguous()
    tan = (math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5))
    view, proj, campos = cam.world_view_transform.contiguous(), cam.full_proj_transform.contiguous(), cam.camera_center.contiguous()
    n, _, radii, geom, binning, img = R.rasterize_gaussians_native(sc.bg, sc.xyz, e, op, scl, rot, 1.0, e, view, proj, tan[0], tan[1],
                                                                   S, S, dc, 0, campos, False, False)

    def backward(**kw):
        return R.rasterize_gaussians_backward_native(sc.bg, sc.xyz, radii, e, scl, rot, 1.0, e, view, proj, tan[0], tan[1], g, dc, 0,
                                                     campos, geom, n, binning, img, False, **kw)

    variants = dict(plain=lambda: backward(), camera=lambda: backward(camera_grad=True))

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    for _ in range(3):
        for fn in variants.values():
            fn()
    ms = {k: {"call": [], "batch": []} for k in variants}
    for _ in range(iters):
        for k, fn in variants.items():
            ms[k]["call"].append(timed(fn, 1))
            ms[k]["batch"].append(timed(fn, batch))
    med = {k: {m: round(statistics.median(v), 4) for m, v in t.items()} for k, t in ms.items()}
    spread = {k: {m: round(max(v) - min(v), 4) for m, v in t.items()} for k, t in ms.items()}
    res = dict(scene="500k head-like shell 512^2, SH degree 0", num_rendered=int(n), iters=iters, ms=med, max_minus_min_ms=spread,
               camera_minus_plain_ms={m: round(med["camera"][m] - med["plain"][m], 4) for m in ("call", "batch")})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
