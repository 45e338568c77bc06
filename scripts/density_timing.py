"""The fused density-field kernel against the composition available without it (the HIP plane gather + torch linear / softplus
/ linear, density.sample_field_torch on the lattice points), on the reference's workload: planes [3, 3, 256, 256, 32] with the
PanoHead axes, the 128^3 lattice (2 097 152 points), sigma only and with rgb.
python scripts/density_timing.py [--rounds R] [--iters I] [--n N]

The two are ALTERNATED: each round times `iters` back-to-back calls of one (device events around the batch, after 3 warm-up
calls), then of the other; R rounds (default 6) of I = 200 calls.  Reported per form: the median over the rounds of the per-call time, the
range, peak memory of one call above what is allocated before it, and the largest difference between the two results.  The
composition gets its lattice points for free (they are generated once, outside the timed window).  One JSON line per form."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gaussian_gan_decoder_amd import density  # noqa: E402


def batch_ms(fn, iters):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--depth", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("density_timing.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    planes_cl = torch.randn(3, args.depth, args.size, args.size, 32, generator=g).to(dev)
    w = density.osg_weights(torch.randn(64, 32, generator=g) / 32 ** 0.5, 0.5 * torch.randn(64, generator=g),
                            torch.randn(33, 64, generator=g) / 8.0, 0.5 * torch.randn(33, generator=g)).to(dev)
    kw = dict(box_warp=1.0, plane_axes="panohead", triplane_depth=args.depth)
    pts = density.lattice_points(args.n, 1.0, "reference", device=dev)
    for want_rgb in (False, True):
        fused = lambda: density.density_grid(planes_cl, w, args.n, want_rgb=want_rgb, **kw)
        composed = lambda: density.sample_field_torch(planes_cl, w, pts, want_rgb=want_rgb, **kw)
        a, b = fused(), composed()
        if want_rgb:
            diff = max(float((a[0].view(-1) - b[0]).abs().max()), float((a[1].view(-1, 32) - b[1]).abs().max()))
        else:
            diff = float((a.view(-1) - b).abs().max())
        del a, b
        mem = {"fused": peak_mb(fused), "composed": peak_mb(composed)}
        ms = {"fused": [], "composed": []}
        for _ in range(args.rounds):
            ms["fused"].append(batch_ms(fused, args.iters))
            ms["composed"].append(batch_ms(composed, args.iters))
        res = {"form": "sigma+rgb" if want_rgb else "sigma", "points": args.n ** 3, "planes": list(planes_cl.shape),
               "rounds": args.rounds, "iters": args.iters, "max_abs_diff": diff}
        for k in ms:
            res[k] = {"median_ms": round(statistics.median(ms[k]), 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4),
                      "peak_mb": round(mem[k], 1)}
        res["speedup"] = round(res["composed"]["median_ms"] / res["fused"]["median_ms"], 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
