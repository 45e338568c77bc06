"""Exact 3-nearest-neighbour distances on the device: the `distCUDA2` of the reference's simple_knn module.

The reference seeds every Gaussian's scale with log(sqrt(distCUDA2(points))) (gaussian_splatting/scene/gaussian_model.py:
132, 160); its simple_knn sources are not part of that tree, so the definition is restated here: element i is the mean of
the squared distances from point i to its three nearest OTHER points (a different index: coincident points count, with
distance 0).  csrc/ggd_knn.hip computes it exactly -- Morton sort, leaves of `leaf_size()` points with a box each, a
workgroup per leaf of queries -- in a fixed fp32 expression order, so the result is bit-identical
to a brute force that evaluates the same expression, from run to run and under any permutation of the rows.
No CPU fallback, no gradient (upstream's has none either), no host sync.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _capi


def _check(points: torch.Tensor, who: str) -> torch.Tensor:
    if not isinstance(points, torch.Tensor):
        raise TypeError(f"{who}: points must be a torch.Tensor")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{who}: points must be [P, 3]")
    if points.dtype != torch.float32:
        raise TypeError(f"{who}: points must be float32")
    if points.shape[0] < 4:
        raise ValueError(f"{who}: at least 4 points are needed (three neighbours per point)")
    if not points.is_cuda:
        raise RuntimeError(f"{who} needs a HIP device tensor (there is no CPU fallback)")
    return points.detach().contiguous()


def leaf_size() -> int:
    """Points per leaf of the search structure (`examined / P` is a small multiple of it)."""
    return int(_capi.load().ggd_knn_leaf_size())


def max_points() -> int:
    return int(_capi.load().ggd_knn_max_points())


def _run(pts: torch.Tensor, mean, dist2, idx, examined):
    dev = pts.device
    P = int(pts.shape[0])
    cx, stream = _capi.context_and_stream(dev)
    if P > cx.lib.ggd_knn_max_points():
        raise ValueError(f"knn: at most {cx.lib.ggd_knn_max_points()} points")
    nbytes = cx.lib.ggd_knn_tmp_bytes(P)
    tmp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(dev):
        cx.check(cx.lib.ggd_knn3(cx.handle, C.c_void_p(stream), ptr(pts), P, ptr(mean), ptr(dist2), ptr(idx), ptr(examined),
                                 ptr(tmp), nbytes))


def dist_cuda2(points: torch.Tensor) -> torch.Tensor:
    """points: device float32 [P, 3], P >= 4 -> float32 [P]: mean squared distance to the three nearest other points."""
    pts = _check(points, "dist_cuda2")
    mean = torch.empty((pts.shape[0],), dtype=torch.float32, device=pts.device)
    _run(pts, mean, None, None, None)
    return mean


def knn3(points: torch.Tensor, return_examined: bool = False):
    """points: device float32 [P, 3], P >= 4 -> (dist2 [P, 3] float32 ascending, idx [P, 3] int32[, examined]).
    idx are row numbers of `points`, never the row itself; among equally distant candidates any may be reported.
    examined (return_examined=True): device int64 scalar, the number of candidate points whose distance was evaluated,
    summed over all queries (a separately compiled kernel instance counts it; the plain call pays nothing)."""
    pts = _check(points, "knn3")
    P = pts.shape[0]
    dist2 = torch.empty((P, 3), dtype=torch.float32, device=pts.device)
    idx = torch.empty((P, 3), dtype=torch.int32, device=pts.device)
    examined = torch.zeros((), dtype=torch.int64, device=pts.device) if return_examined else None
    _run(pts, None, dist2, idx, examined)
    return (dist2, idx, examined) if return_examined else (dist2, idx)
