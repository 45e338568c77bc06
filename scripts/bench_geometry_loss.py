"""Times the fused geometry loss (losses.fused_geometry_loss: two HIP launches) against the torch expression it replaces
(losses.geometry_loss_torch on the device), and one DecoderTrainer step with and without the geometry term:

    python scripts/bench_geometry_loss.py [--iters 30] [--warmup 5] [--size 512] [--teacher 64] [--no-trainer]
                                          [--scenes 4] [--points 500000] [--out FILE]

  operator   forward + backward of one call at size x size against teacher x teacher maps: the loss, then total.backward()
             into depth and alpha (leaf tensors)
  trainer    DecoderTrainer.step at config 3's shape (scenes x points, 512 x 512, fused decoder, fused activations; no
             stand-ins) with mask_weight = depth_weight = 0 and with (1, 1)

hipEvent timing (torch.cuda.Event) around every iteration after `warmup` untimed ones; median and p10 / p90 over `iters`."""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussian_gan_decoder_amd import losses as L                               # noqa: E402
from gaussian_gan_decoder_amd.train import DecoderTrainer, make_scene_batch    # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    t = torch.tensor(ms, dtype=torch.float64)
    return tuple(float(torch.quantile(t, q)) for q in (0.5, 0.1, 0.9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--teacher", type=int, default=64)
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--points", type=int, default=500_000)
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geometry_loss.py measures on the GPU: no HIP device visible")
    dev = torch.device("cuda:0")
    fmt = lambda r: f"{r[0]:8.3f} [{r[1]:7.3f} {r[2]:7.3f}]"
    lines = [f"# {torch.cuda.get_device_name(0)}; iters {args.iters}, warmup {args.warmup}; ms: median [p10 p90]"]
    print(lines[0], flush=True)

    def row(text):
        lines.append(text)
        print(text, flush=True)

    S, T = args.size, args.teacher
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing="ij")
    alpha = (torch.clip((torch.exp(-2.0 * (xx ** 2 + yy ** 2)) - 0.2) / 0.5, 0, 1) * torch.rand(S, S, generator=g)).to(dev)
    depth = alpha * (2.3 + 0.9 * torch.rand(S, S, generator=g).to(dev))
    ty, tx = torch.meshgrid(torch.linspace(-1, 1, T), torch.linspace(-1, 1, T), indexing="ij")
    w = (torch.clip((torch.exp(-3.0 * (tx ** 2 + ty ** 2)) - 0.2) / 0.5, 0, 1) * (0.7 + 0.3 * torch.rand(T, T, generator=g))).to(dev)
    t = (2.25 + 1.05 * torch.rand(T, T, generator=g)).to(dev)
    results = {}

    def operator(fn):
        def run():
            D, A = depth.detach().requires_grad_(True), alpha.detach().requires_grad_(True)
            total, terms = fn(D[None], A[None], t, w, 0.149, 0.149, 1.0, 1.0)
            total.backward()
            results[fn.__name__] = (terms.detach(), D.grad, A.grad)
        return run
    row(f"operator, forward + backward, {S} x {S} against {T} x {T}")
    fused = timed(operator(L.fused_geometry_loss), args.iters, args.warmup)
    torch_ = timed(operator(L.geometry_loss_torch), args.iters, args.warmup)
    fused2 = timed(operator(L.fused_geometry_loss), args.iters, args.warmup)
    torch2 = timed(operator(L.geometry_loss_torch), args.iters, args.warmup)
    row(f"  fused_geometry_loss (2 launches)      {fmt(fused)}   second round {fmt(fused2)}")
    row(f"  geometry_loss_torch (torch on device) {fmt(torch_)}   second round {fmt(torch2)}")
    a, b = results["fused_geometry_loss"], results["geometry_loss_torch"]
    row(f"  terms fused {[f'{v:.7f}' for v in a[0].tolist()]} torch {[f'{v:.7f}' for v in b[0].tolist()]}; max |d grad_depth| "
        f"{float((a[1] - b[1]).abs().max()):.2e}, max |d grad_alpha| {float((a[2] - b[2]).abs().max()):.2e} "
        f"(gradient scale {1.0 / (S * S):.2e})")

    if not args.no_trainer:
        row(f"DecoderTrainer.step, {args.scenes} x {args.points} points, 512 x 512, fused decoder (bf16), fused activations")
        batch = make_scene_batch(list(range(args.scenes)), args.points, 512, dev, seed=0, with_geometry=True)
        make = lambda **kw: DecoderTrainer(dev, n_scenes_total=args.scenes, image_size=512, fused_activations=True,
                                           fused_decoder=True, **kw)
        off, on = make(), make(mask_weight=1.0, depth_weight=1.0)
        t_off = timed(lambda: off.step(batch), args.iters, args.warmup)
        t_on = timed(lambda: on.step(batch), args.iters, args.warmup)
        t_off2 = timed(lambda: off.step(batch), args.iters, args.warmup)
        t_on2 = timed(lambda: on.step(batch), args.iters, args.warmup)
        row(f"  mask_weight = depth_weight = 0        {fmt(t_off)}   second round {fmt(t_off2)}")
        row(f"  mask_weight = depth_weight = 1        {fmt(t_on)}   second round {fmt(t_on2)}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
