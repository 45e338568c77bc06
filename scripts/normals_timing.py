"""Cost of the normal-consistency term: forward and forward + backward of three variants, alternated in one process.
python scripts/normals_timing.py [--iters N]

Scene: 500 k Gaussians at 512^2 on a head-like shell (the train step's shape, the scene of scripts/distortion_timing.py), through
render_simple and autograd, as the trainer runs it.
  depth_alpha   (a) a render with render_depth_alpha=True                (the geometry-supervised frame)
  fused         (b) (a) with render_normals=True and fused_normal_loss   (ggd_gaussian_normals, three more feature channels, ggd_normal_loss)
  composed      (c) the same result by composition: the normals in torch ops (gaussian_normals_torch) passed as features=, and
                    normal_loss_torch
The backward of every variant starts from N(0, 1) gradients on colour, depth and alpha; (b) and (c) add the loss to that scalar.
Times are HIP-event milliseconds around the whole call sequence of a variant (launches, allocations and the host's waits for
num_rendered included), median over the iterations.  Prints one JSON line."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gaussian_gan_decoder_amd import normals as N  # noqa: E402
from gaussian_gan_decoder_amd.gaussian_renderer import render_simple  # noqa: E402
from gaussian_gan_decoder_amd.synthetic import make_scene  # noqa: E402


def main():
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    iters, S, P = arg("--iters", 15), 512, 500_000
    if not torch.cuda.is_available():
        raise SystemExit("normals_timing.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    sc = make_scene(P, S, "shell", seed=3, h=math.pi / 2 + 0.6).to(dev)
    cam = sc.cam
    pc = sc.gaussian_model(requires_grad=True)
    gen = torch.Generator().manual_seed(1)
    g = torch.randn(3, S, S, generator=gen).to(dev)
    gD, gA = (torch.randn(1, S, S, generator=gen).to(dev) for _ in range(2))
    tan = math.tan(cam.FoVx * 0.5)
    base = lambda out: (out["render"] * g).sum() + (out["depth"] * gD).sum() + (out["alpha"] * gA).sum()

    def run(scalar, bwd):
        for p in (pc._xyz, pc._scaling, pc._rotation, pc._opacity, pc._features_dc):
            p.grad = None
        with torch.set_grad_enabled(bwd):
            total = scalar()
            if bwd:
                total.backward()
        return total

    def depth_alpha():
        return base(render_simple(cam, pc, bg_color=sc.bg, render_depth_alpha=True))

    def fused():
        out = render_simple(cam, pc, bg_color=sc.bg, render_depth_alpha=True, render_normals=True)
        return base(out) + N.fused_normal_loss(out["normals"], out["depth"], out["alpha"], tan, tan)[0]

    def composed():
        n = N.gaussian_normals_torch(pc.get_rotation, pc.get_scaling, pc.get_xyz, cam.world_view_transform)
        out = render_simple(cam, pc, bg_color=sc.bg, render_depth_alpha=True, features=n)
        return base(out) + N.normal_loss_torch(out["features"], out["depth"], out["alpha"], tan, tan)[0]

    variants = dict(depth_alpha=depth_alpha, fused=fused, composed=composed)

    def timed(fn, bwd):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        run(fn, bwd)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for _ in range(3):
        for fn in variants.values():
            run(fn, True)
    agree = abs(float(run(fused, False)) - float(run(composed, False)))
    ms = {k: {"forward": [], "forward_backward": []} for k in variants}
    for _ in range(iters):
        for k, fn in variants.items():
            ms[k]["forward"].append(timed(fn, False))
            ms[k]["forward_backward"].append(timed(fn, True))
    med = {k: {m: round(statistics.median(v), 3) for m, v in t.items()} for k, t in ms.items()}
    spread = {k: {m: round(max(v) - min(v), 3) for m, v in t.items()} for k, t in ms.items()}
    res = dict(scene="500k head-like shell 512^2", iters=iters, ms=med, max_minus_min_ms=spread,
               fused_minus_composed_scalar=agree,
               fused_minus_depth_alpha_ms={m: round(med["fused"][m] - med["depth_alpha"][m], 3) for m in med["fused"]},
               composed_minus_depth_alpha_ms={m: round(med["composed"][m] - med["depth_alpha"][m], 3) for m in med["composed"]})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
