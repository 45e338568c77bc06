"""Times the fused decoder for every decoder chain and precision tier, beside the PyTorch module of the same type:

    python scripts/bench_decoder_chains.py [--chains 0,1,2] [--tiers bf16,fp32] [--iters 30] [--warmup 5] [--no-torch]
                                           [--fwd-points 1000000] [--train-points 2000000] [--out FILE]

  forward        FusedDecoder.decode_features at 1 M points (the inference launch alone, weights packed beforehand)
  train          pack + forward (pre-activations kept) + backward + weight gradients at 2 M points: FusedDecoderFn forward and
                 backward under a given dattrs -- what a training step spends in the decoder
  torch          the fp32 PyTorch module on the same plane features: forward under no_grad, and forward + backward

hipEvent timing (torch.cuda.Event) around every iteration after `warmup` untimed ones; median and p10 / p90 over `iters`.
On a tree whose fused decoder knows one chain only (no fused_decoder._CHAINS) it times chain 0 alone, through the same calls:
that is how the chain-0 figures of two commits are compared."""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussian_gan_decoder_amd import decoder as D                # noqa: E402
from gaussian_gan_decoder_amd import fused_decoder as FD         # noqa: E402

HAS_CHAINS = hasattr(FD, "_CHAINS")
TYPES = {0: ("sequential_reversed", "SequentialDecoderReverse"), 1: ("sequential", "SequentialDecoder"), 2: ("parallel", "ParallelDecoder")}


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


def inputs(n, dev):
    g = torch.Generator().manual_seed(11)
    feats = (0.6 * torch.randn(n, 32, generator=g)).to(dev)
    pos = (torch.rand(n, 3, generator=g) - 0.5).to(dev)
    dattrs = torch.randn(n, 16, generator=g)
    dattrs[:, 14:] = 0
    return feats, pos, dattrs.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="0,1,2" if HAS_CHAINS else "0")
    ap.add_argument("--tiers", default="bf16,fp32")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fwd-points", type=int, default=1_000_000)
    ap.add_argument("--train-points", type=int, default=2_000_000)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    chains = [int(c) for c in args.chains.split(",")]
    if not HAS_CHAINS and chains != [0]:
        sys.exit("this tree's fused decoder implements chain 0 only")
    dev = torch.device("cuda:0")
    lines = [f"# {torch.cuda.get_device_name(0)}; iters {args.iters}, warmup {args.warmup}; forward at {args.fwd_points} points, "
             f"train (pack + forward + backward + weight gradients) at {args.train_points} points; ms: median [p10 p90]",
             f"{'chain':22s} {'tier':6s} {'forward':>24s} {'train':>27s}"]

    def row(name, tier, f, t):
        fmt = lambda r: f"{r[0]:8.3f} [{r[1]:7.3f} {r[2]:7.3f}]"
        lines.append(f"{name:22s} {tier:6s} {fmt(f)} {fmt(t):>27s}")
        print(lines[-1], flush=True)

    print("\n".join(lines), flush=True)
    ff, fp, _ = inputs(args.fwd_points, dev)
    tf, tp, td = inputs(args.train_points, dev)
    for c in chains:
        name, cls = TYPES[c]
        torch.manual_seed(3)
        mod = getattr(D, cls)().to(dev)
        params = [t for head in FD._head_tensors(mod) for t in head]
        extra = (c,) if HAS_CHAINS else ()
        for tier in args.tiers.split(","):
            hl = tier == "fp32"
            inf = FD.FusedDecoder(mod, precision=tier)
            f = timed(lambda: inf.decode_features(ff, fp), args.iters, args.warmup)
            bufs = [None]

            def train():
                bufs[0] = FD.device_pack(mod, params, bufs[0], hl)
                x = tf.detach().requires_grad_(True)
                a = FD.FusedDecoderFn.apply(x, tp, bufs[0][0], bufs[0][1], hl, *extra, *params)
                a.backward(td)
            t = timed(train, args.iters, args.warmup)
            for p in mod.parameters():
                p.grad = None
            row(f"{c} {name}", tier, f, t)
        if not args.no_torch:
            def tfwd():
                with torch.no_grad():
                    mod(None, fp, features=ff)

            def ttrain():
                x = tf.detach().requires_grad_(True)
                o = mod(None, tp, features=x)
                torch.cat([o.color, o.opacity, o.rotation, o.scale, o.xyz], 1).backward(td[:, :14])
            it = max(3, args.iters // 5)
            row(f"{c} {name}", "torch", timed(tfwd, it, 2), timed(ttrain, it, 2))
            for p in mod.parameters():
                p.grad = None
        del mod, params
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
