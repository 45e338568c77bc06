"""Times the perceptual term: losses.FusedPerceptual (csrc/ggd_perceptual.hip) against the PyTorch stand-in it replaces, and one
DecoderTrainer step with and without fused_perceptual:

    python scripts/perceptual_timing.py [--iters 20] [--warmup 5] [--rounds 3] [--batch 4] [--size 512] [--width-div 1]
                                        [--no-trainer] [--scenes 4] [--points 500000] [--out FILE]

  operator   forward + backward of one call, image and target [batch, 3, size, size], the gradient into the image:
               standin fp32        PerceptualStandIn as the trainer runs it (fp32, channels_last, MIOpen): the parent's path, the bar
               standin autocast    the same under torch.autocast(bfloat16), for information
               fused fp32          FusedPerceptual(precision="fp32"): split-bf16 operands, three MFMAs per product
               fused bf16          FusedPerceptual(precision="bf16"): f16 operands forward, bf16 backward
             The four variants alternate inside every round (others share the host), `rounds` rounds of `iters` timed calls
             each after `warmup` untimed ones; median and p10 / p90 over all timed calls of a variant.  Also printed: the loss of
             each variant, the relative L2 distance of its image gradient from the fp32 stand-in's, and the rate the convolutions'
             FLOP count (from the shapes: 2 * 9 * Cin * Cout * pixels per layer, 2 B images forward, B backward) makes of it.
  trainer    DecoderTrainer.step at config 3's shape with bench.py's stand-ins (perceptual_weight=1, the backbone payload, fused
             decoder, fused activations, PanoHead planes) at both decoder precisions, fused_perceptual off and on.

hipEvent timing (torch.cuda.Event) around every call."""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussian_gan_decoder_amd.losses import FusedPerceptual, PerceptualStandIn   # noqa: E402


def timed_once(fn, iters):
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def quantiles(ms):
    t = torch.tensor(ms, dtype=torch.float64)
    return tuple(float(torch.quantile(t, q)) for q in (0.5, 0.1, 0.9))


def conv_flop(module, batch, size):
    """FLOP of the convolutions of one call: 2 * batch images forward, batch images backward-data (conv1_1's included)."""
    side, total, ci = min(size, 256), 0, 0
    for v in module.CFG:
        if v == "M":
            side //= 2
            continue
        w = module.convs[ci].weight
        total += 2 * 9 * int(w.shape[0]) * int(w.shape[1]) * side * side
        ci += 1
    return 3 * batch * total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--width-div", type=int, default=1)
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--points", type=int, default=500_000)
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--no-operator", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perceptual_timing.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    fmt = lambda r: f"{r[0]:8.3f} [{r[1]:7.3f} {r[2]:7.3f}]"
    lines = [f"# {torch.cuda.get_device_name(0)}; iters {args.iters} x rounds {args.rounds}, warmup {args.warmup}; ms: median [p10 p90]"]
    print(lines[0], flush=True)

    def row(text):
        lines.append(text)
        print(text, flush=True)

    if not args.no_operator:
        B, S = args.batch, args.size
        g = torch.Generator().manual_seed(5)
        yy, xx = torch.meshgrid(torch.linspace(0, 1, S), torch.linspace(0, 1, S), indexing="ij")
        target = torch.stack([torch.stack([0.5 + 0.4 * torch.sin(9 * xx + c + b) * torch.cos(7 * yy - b) for c in range(3)])
                              for b in range(B)]).to(dev)
        image = (target + 0.15 * torch.randn(target.shape, generator=g).to(dev)).clamp(0, 1).contiguous()
        module = PerceptualStandIn(seed=1333, width_div=args.width_div).to(dev).to(memory_format=torch.channels_last)
        fused = {p: FusedPerceptual(module, precision=p) for p in ("fp32", "bf16")}
        results = {}

        def call(name, fn, autocast=False):
            def run():
                x = image.detach().requires_grad_(True)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                    loss = fn(x, target)
                loss.backward()
                results[name] = (loss.detach(), x.grad)
            return run

        variants = [("standin fp32", call("standin fp32", module)), ("standin autocast", call("standin autocast", module, True)),
                    ("fused fp32", call("fused fp32", fused["fp32"])), ("fused bf16", call("fused bf16", fused["bf16"]))]
        ms = {name: [] for name, _ in variants}
        for _ in range(args.rounds):
            for name, fn in variants:
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize()
                ms[name] += timed_once(fn, args.iters)
        flop = conv_flop(module, B, S)
        row(f"operator: batch {B}, {S} x {S}, width_div {args.width_div}, forward + backward; {flop / 1e9:.1f} GFLOP of convolutions per call")
        base_loss, base_grad = results["standin fp32"]
        for name, _ in variants:
            q = quantiles(ms[name])
            loss, grad = results[name]
            rel = float((grad.double() - base_grad.double()).norm() / base_grad.double().norm())
            row(f"  {name:18s} {fmt(q)} ms  {flop / q[0] / 1e9:7.1f} TFLOP/s  loss {float(loss):.6f} (stand-in {float(base_loss):.6f})  "
                f"gradient rel. L2 from the fp32 stand-in {rel:.2e}")

    if not args.no_trainer:
        from gaussian_gan_decoder_amd.train import DecoderTrainer, make_scene_batch
        batches = [make_scene_batch(list(range(args.scenes)), args.points, 512, dev, seed=i) for i in range(2)]
        planes_floats = 3 * 96 * 256 * 256
        row(f"trainer: {args.scenes} scenes x {args.points} points, 512 x 512, fused decoder, stand-ins (perceptual_weight 1, backbone payload)")
        for precision in ("bf16", "fp32"):
            trainers = {}
            for fused_p in (False, True):
                trainers[fused_p] = DecoderTrainer(dev, n_scenes_total=args.scenes, image_size=512, fused_activations=True,
                                                   fused_decoder=True, backbone_params=29_570_000 - planes_floats,
                                                   perceptual_weight=1.0, decoder_precision=precision, plane_axes="panohead",
                                                   triplane_depth=3, fused_perceptual=fused_p)
            ms = {k: [] for k in trainers}
            it = [0]
            for _ in range(args.rounds):
                for k, tr in trainers.items():
                    def step():
                        tr.step(batches[it[0] % 2])
                        it[0] += 1
                    for _ in range(max(2, args.warmup // 2)):
                        step()
                    torch.cuda.synchronize()
                    ms[k] += timed_once(step, max(4, args.iters // 2))
            for k in trainers:
                row(f"  decoder_precision {precision}, fused_perceptual {str(k):5s} {fmt(quantiles(ms[k]))} ms per step")
            del trainers
            torch.cuda.empty_cache()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
