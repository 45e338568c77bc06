"""Float64 reference of the contribution statistics (ggd_contribution), written out in numpy over a decoded forward as
_features_ref.blend_f64 is: the forward's decisions are taken where they are stored (n_contrib bounds every pixel's walk; the
fp32 T < 1e-4 stop lies behind it), inside the bound the skip rules are re-evaluated in float64.  A tile's pixels walk its list
together, one numpy step per list position."""
from __future__ import annotations

import numpy as np

FLOOR = 1.0 / 255.0
WINDOW = 1e-6          # a decision this close to its threshold may fall the other way in fp32 (as oracle.fragile_pixels)
SCALE = 2.0 ** 24      # GGD_CONTRIB_SCALE_LOG2
FLIP_GAIN = 0.004      # >= (1/255) / (1 - 1/255) = 0.003937: what one flipped pair at the floor rescales the weights behind it by


def contribution_f64(n_contrib, point_list, ranges, xy, conic_opacity):
    """dict of float64 / int64 arrays [P]: sum, max, count of w = alpha T over the (pixel, Gaussian) pairs of the forward;
    own_fragile: the Gaussian's pairs with |alpha - 1/255| <= 1e-6 or |power| <= 1e-6 (in or out by an ulp of exp);
    slack: the sum of w over its pairs that lie BEHIND a fragile pair of the same pixel."""
    n_contrib = np.asarray(n_contrib)
    H, W = n_contrib.shape
    gx = (W + 15) // 16
    xy = np.asarray(xy, np.float64)
    co = np.asarray(conic_opacity, np.float64)
    P = xy.shape[0]
    out = dict(sum=np.zeros(P), max=np.zeros(P), count=np.zeros(P, np.int64), own_fragile=np.zeros(P, np.int64), slack=np.zeros(P))
    for tile in range(len(ranges)):
        lo, hi = int(ranges[tile][0]), int(ranges[tile][1])
        x0, y0 = (tile % gx) * 16, (tile // gx) * 16
        x1, y1 = min(x0 + 16, W), min(y0 + 16, H)
        if x1 <= x0 or y1 <= y0 or hi <= lo:
            continue
        nc = np.minimum(n_contrib[y0:y1, x0:x1].astype(np.int64), hi - lo)
        ys, xs = np.mgrid[y0:y1, x0:x1].astype(np.float64)
        T = np.ones(nc.shape)
        behind = np.zeros(nc.shape, bool)
        for k in range(int(nc.max(initial=0))):
            i = int(point_list[lo + k])
            live = k < nc
            dx, dy = xy[i, 0] - xs, xy[i, 1] - ys
            power = -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
            with np.errstate(over="ignore"):
                alpha = np.minimum(0.99, co[i, 3] * np.exp(power))
            fragile = live & ((np.abs(alpha - FLOOR) <= WINDOW) | (np.abs(power) <= WINDOW))
            upd = live & ~(power > 0.0) & ~(alpha < FLOOR)
            w = np.where(upd, alpha * T, 0.0)
            out["sum"][i] += w.sum()
            out["max"][i] = max(out["max"][i], float(w.max()))
            out["count"][i] += int(upd.sum())
            out["own_fragile"][i] += int(fragile.sum())
            out["slack"][i] += float(w[behind].sum())
            T = np.where(upd, T * (1.0 - alpha), T)
            behind |= fragile
    return out


def of_forward(o):
    """contribution_f64 of a decoded forward (the oracle's dict, or _util.decode_result's of a native run)"""
    return contribution_f64(o["n_contrib"], o["point_list"], o["ranges"], o["xy"], o["conic_opacity"])


def fragile_cap(P):
    """the most rows with own_fragile > 0 a scene may have (a condition of the comparison, not a measurement)"""
    return max(4, P // 50)


def sum_tolerance(ref, atol=1e-5):
    """per row: atol count (the per-pixel colour bar on a one-hot colour) + 2^-25 count (the fixed-point rounding) + FLIP_GAIN
    slack (pairs behind a pair that may flip) + own_fragile / 255 (its own pairs at the floor, each worth at most 1/255)"""
    return atol * ref["count"] + 2.0 ** -25 * ref["count"] + FLIP_GAIN * ref["slack"] + ref["own_fragile"] / 255.0


def max_tolerance(ref, atol=1e-5):
    """the same with count = 1"""
    return atol + 2.0 ** -25 + FLIP_GAIN * ref["slack"] + ref["own_fragile"] / 255.0


__all__ = ["contribution_f64", "of_forward", "fragile_cap", "sum_tolerance", "max_tolerance", "SCALE"]
