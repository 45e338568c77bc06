"""Device time of the fitting loop's optimizer step: SparseGaussianAdam (csrc/ggd_adam.hip, one launch) against torch.optim.Adam
as GaussianModel.training_setup builds it, and against torch.optim.Adam(fused=True), on the same parameters and gradients.
python scripts/adam_timing.py [--rounds R] [--points N] [--steps K]

N rows (default 1 M), 16 SH coefficients per channel: the six GaussianModel groups, 59 floats per row.  Variants, alternated
inside ONE process (every round times each variant once, the order rotating from round to round), hipEvent pairs around K
(default 5) back-to-back steps, R rounds (default 30) after 3 warm-up rounds:
  sparse_100 / sparse_50 / sparse_10    optimizer.step(radii, N) with 100 % / 50 % / 10 % of the rows visible, drawn per row
  torch_adam                            torch.optim.Adam(groups, lr=0.0, eps=1e-15) -- today's training_setup
  torch_adam_fused                      the same with fused=True
Per variant: median, min, the 10th and 90th percentile of the per-step time and spread = p90 - p10.  The sparse step's bytes are
counted from the visible rows (four arrays read, three written, 59 floats each) plus the N radii, and set against 6.3 TB/s.
Acceptance: sparse_100's median is below torch_adam_fused's by more than the two spreads together.
One JSON line."""
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from gaussian_gan_decoder_amd.gaussian_model import PARAM_GROUPS, GaussianModel  # noqa: E402

HBM_TBS = 6.3
M = 16
SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (M - 1, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
FLOATS_PER_ROW = 14 + 3 * (M - 1)


def option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def percentile(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def main():
    rounds, N, steps = max(10, option("--rounds", 30)), option("--points", 1_000_000), max(1, option("--steps", 5))
    if not torch.cuda.is_available():
        raise RuntimeError("adam_timing.py needs an MI355X: no HIP device visible")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    params = {n: torch.nn.Parameter(torch.randn((N,) + s, generator=gen).to(dev)) for n, s in SHAPES.items()}
    for p in params.values():
        p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).to(dev)
    args = dict(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
                position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)

    def model(**over):                                    # every model holds the SAME six parameters; the moments are its own
        pc = GaussianModel(3)
        for name, attr in PARAM_GROUPS:
            setattr(pc, attr, params[name])
        pc.spatial_lr_scale = 1.0
        pc.training_setup(SimpleNamespace(**args, **over))
        return pc

    sparse, stock = model(optimizer_type="sparse_adam").optimizer, model().optimizer
    assert type(stock) is torch.optim.Adam
    fused = torch.optim.Adam([{k: v for k, v in g.items() if k in ("params", "lr", "name")} for g in stock.param_groups],
                             lr=0.0, eps=1e-15, fused=True)
    radii, visible = {}, {}
    for pct in (100, 50, 10):
        r = (torch.randint(1, 60, (N,), generator=gen) * (torch.rand((N,), generator=gen) < pct / 100.0)).to(torch.int32)
        radii[pct], visible[pct] = r.to(dev), int((r > 0).sum())
    variants = {f"sparse_{pct}": (lambda pct=pct: sparse.step(radii[pct], N)) for pct in (100, 50, 10)}
    variants["torch_adam"] = stock.step
    variants["torch_adam_fused"] = fused.step
    names = list(variants)
    ms = {n: [] for n in names}
    for rnd in range(3 + rounds):
        for k in range(len(names)):
            name = names[(k + rnd) % len(names)]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                variants[name]()
            b.record()
            b.synchronize()
            if rnd >= 3:
                ms[name].append(a.elapsed_time(b) / steps)
    out = dict(N=N, sh_coefficients=M, floats_per_row=FLOATS_PER_ROW, rounds=rounds, steps_per_sample=steps)
    stats = {}
    for name in names:
        med, lo, hi = statistics.median(ms[name]), percentile(ms[name], 0.1), percentile(ms[name], 0.9)
        stats[name] = dict(median_ms=round(med, 4), min_ms=round(min(ms[name]), 4), p10_ms=round(lo, 4), p90_ms=round(hi, 4),
                           spread_ms=round(hi - lo, 4))
    for pct in (100, 50, 10):
        s = stats[f"sparse_{pct}"]
        moved = visible[pct] * FLOATS_PER_ROW * 4 * 7 + 4 * N
        s.update(visible_rows=visible[pct], mb=round(moved / 1e6, 1), tb_s=round(moved / s["median_ms"] / 1e9, 2),
                 fraction_of_hbm=round(moved / s["median_ms"] / 1e9 / HBM_TBS, 2))
    dense = N * FLOATS_PER_ROW * 4 * 7
    for name in ("torch_adam", "torch_adam_fused"):
        stats[name]["tb_s_if_one_pass"] = round(dense / stats[name]["median_ms"] / 1e9, 2)
    out.update(stats)
    gap = stats["torch_adam_fused"]["median_ms"] - stats["sparse_100"]["median_ms"]
    combined = stats["torch_adam_fused"]["spread_ms"] + stats["sparse_100"]["spread_ms"]
    out["fused_minus_sparse_100_ms"], out["combined_spread_ms"] = round(gap, 4), round(combined, 4)
    out["sparse_100_beats_fused_beyond_spread"] = bool(gap > combined)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
