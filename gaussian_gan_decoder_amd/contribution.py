"""Per-Gaussian contribution statistics of rendered frames (ggd_contribution, csrc/ggd_contribution.hip):
which Gaussians the frames used and how much -- what pruning and compaction of a trained model rank by.

    stats = ContributionStats(P, device)
    for cam in cameras:
        render_simple(cam, pc, bg, contribution=stats)      # or render(...); accumulates, no torch op per frame
    pc.prune_by_contribution(stats, min_max_weight=0.01)     # GaussianModel: drop what no ray saw with weight >= 0.01

Over every (pixel, Gaussian) pair a frame's colour pass blended, with w = alpha T: `weight_sum` (sum of w: Mini-Splatting's and
gsplat's importance), `pixel_count` (the number of pairs: LightGaussian's hit count) and `weight_max` (the largest w: RadSplat's
score).  The device side is three integer atomics per (8 x 8 pixel quarter, Gaussian) on `raw`, int64 [P, 3]:
(fixed-point sum in units of 2^-24, count, fp32 bits of the maximum), so an accumulation is bit-identical from run to run.  The
decoding below is plain torch and works on a CPU copy of `raw` as well."""
from __future__ import annotations

import torch

from ._capi import CONTRIB_SCALE_LOG2

KINDS = ("sum", "max", "count")


def decode_weight_sum(raw: torch.Tensor) -> torch.Tensor:
    """float64 [P]: raw[:, 0] 2^-24 (exact: a sum of up to 2^29 pairs stays below 2^53)"""
    return raw[:, 0].to(torch.float64) * (2.0 ** -CONTRIB_SCALE_LOG2)


def decode_pixel_count(raw: torch.Tensor) -> torch.Tensor:
    """int64 [P]"""
    return raw[:, 1].clone()


def decode_weight_max(raw: torch.Tensor) -> torch.Tensor:
    """float32 [P]: the low 32 bits of raw[:, 2] reinterpreted"""
    return raw[:, 2].contiguous().view(torch.int32).reshape(-1, 2)[:, 0].contiguous().view(torch.float32)


def check_raw(raw, P: int, device) -> torch.Tensor:
    """The refusals (ValueError) of a statistics tensor handed to a render of P Gaussians on `device`, before any device call."""
    if not isinstance(raw, torch.Tensor):
        raise ValueError(f"contribution must be a ContributionStats or an int64 [{P}, 3] tensor (got {type(raw).__name__})")
    if raw.dtype != torch.int64:
        raise ValueError(f"contribution statistics must be int64 (got {raw.dtype})")
    if tuple(raw.shape) != (P, 3):
        raise ValueError(f"contribution statistics must have dimensions (num_points, 3) = ({P}, 3) (got {tuple(raw.shape)})")
    if raw.device != torch.device(device):
        raise ValueError(f"contribution statistics are on {raw.device}, expected {device}")
    if not raw.is_contiguous():
        raise ValueError("contribution statistics must be contiguous: the kernel accumulates into them in place")
    return raw


class ContributionStats:
    """The accumulated statistics of P Gaussians.  raw: int64 [P, 3] on `device`, zeros at first; frames: renders accumulated."""

    def __init__(self, P: int, device="cpu"):
        self.raw = torch.zeros((int(P), 3), dtype=torch.int64, device=device)
        self.frames = 0

    @property
    def P(self) -> int:
        return int(self.raw.shape[0])

    @property
    def weight_sum(self) -> torch.Tensor:
        return decode_weight_sum(self.raw)

    @property
    def pixel_count(self) -> torch.Tensor:
        return decode_pixel_count(self.raw)

    @property
    def weight_max(self) -> torch.Tensor:
        return decode_weight_max(self.raw)

    def reset(self):
        self.raw.zero_()
        self.frames = 0

    def score(self, kind: str = "sum") -> torch.Tensor:
        """float32 [P]: the statistic to rank by -- "sum", "max" or "count" """
        if kind == "sum":
            return self.weight_sum.to(torch.float32)
        if kind == "max":
            return self.weight_max
        if kind == "count":
            return self.pixel_count.to(torch.float32)
        raise ValueError(f"kind must be one of {KINDS} (got {kind!r})")


def resolve(contribution, P: int, device):
    """The `contribution` keyword of render / render_simple: a ContributionStats (accumulated into), True (a fresh one) or None /
    False (no statistics) -> the object or None.  Refusals (ValueError) before any device call."""
    if contribution is None or contribution is False:
        return None
    if contribution is True:
        return ContributionStats(P, device)
    if not isinstance(contribution, ContributionStats):
        raise ValueError(f"contribution must be a ContributionStats or True (got {type(contribution).__name__})")
    check_raw(contribution.raw, P, device)
    return contribution


__all__ = ["ContributionStats", "KINDS", "check_raw", "decode_pixel_count", "decode_weight_max", "decode_weight_sum", "resolve"]
