"""Brute-force restatement of the 3-nearest-neighbour contract, in numpy, one operation per rounding:

    dx = a.x - b.x (dy, dz alike);  d = (dx*dx + dy*dy) + dz*dz;  three smallest d over all j != i, ascending b0 <= b1 <= b2;
    mean = ((b0 + b1) + b2) / 3

numpy rounds every elementwise operation to the array's dtype and never contracts a multiply-add, so with dtype=np.float32
this IS the expression the kernel evaluates (the bit-exact oracle); with np.float64 it is the check on that oracle."""
import numpy as np

_BUDGET = 1 << 23   # elements of one distance block


def brute_knn3(points, dtype=np.float32, rows=None):
    """points [P, 3] -> the three smallest squared distances to OTHER rows, ascending, [len(rows), 3] in `dtype`
    (rows: the query rows, default all)."""
    p = np.ascontiguousarray(np.asarray(points), dtype=dtype)
    P = p.shape[0]
    assert P >= 4 and p.shape[1] == 3
    rows = np.arange(P) if rows is None else np.asarray(rows, dtype=np.int64)
    out = np.empty((len(rows), 3), dtype=dtype)
    px, py, pz = (np.ascontiguousarray(p[:, k])[None, :] for k in range(3))
    step = max(1, _BUDGET // P)
    for s in range(0, len(rows), step):
        r = rows[s:s + step]
        q = p[r]
        dx = q[:, 0:1] - px
        dy = q[:, 1:2] - py
        dz = q[:, 2:3] - pz
        d = (dx * dx + dy * dy) + dz * dz
        d[np.arange(len(r)), r] = np.inf          # "other" = a different index; coincident points stay in
        out[s:s + step] = np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1)
    return out


def mean_of(d3):
    d3 = np.asarray(d3)
    return ((d3[:, 0] + d3[:, 1]) + d3[:, 2]) / d3.dtype.type(3)


def brute_mean_dist2(points, dtype=np.float32, rows=None):
    return mean_of(brute_knn3(points, dtype, rows))


def dist2_of(points, i, j, dtype=np.float32):
    """the contract's distance between rows i and j (arrays of equal length)"""
    p = np.asarray(points, dtype=dtype)
    dx, dy, dz = (p[i, k] - p[j, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def clouds(P=20000, seed=0):
    """The five test inputs: name -> float32 [~P, 3]."""
    g = np.random.default_rng(seed)
    out = {"uniform": g.random((P, 3), dtype=np.float32) - np.float32(0.5)}
    c = g.normal(0.0, 1e-3, (P, 3)).astype(np.float32)
    c[P // 2:, 0] += np.float32(100.0)
    out["two_far_clusters"] = c
    ax = np.arange(27, dtype=np.float32) / np.float32(27)
    out["lattice"] = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    base = g.random((P // 4, 3), dtype=np.float32)
    out["duplicates_x4"] = g.permutation(np.tile(base, (4, 1))).astype(np.float32)
    d = g.normal(size=(P, 3))
    out["sphere"] = (0.3 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return out
