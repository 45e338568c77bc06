"""float64 restatement of the plane gather / scatter (csrc/ggd_triplane.hip: ggd_planes_gather / ggd_planes_scatter) with a
per-element error budget, and the case table of tests/test_planes_instances_gpu.py.

The restatement is decoder.sample_from_planes(...).mean(0) written out tap by tap (no grid_sample, so it shares no code with
the kernels or with torch's sampler):  coords = (2 / box_warp) * pos;  (u, v[, w]) = coords projected with PLANE_AXES;
i = ((u + 1) * size - 1) / 2 per axis;  4 taps (planes) or 8 taps (grids) at floor(i) + {0, 1}, weights (x) * (y) [* (z)],
zero padding;  the texel is multiplied by the optional modulation [max(D, 1), C];  mean over the three planes.  A tap is
inside when its coordinates are in range, tested in FLOATING POINT: a +-inf or +-1e30 row simply has no tap on that plane.

Budgets.  With S = max(W, H, max(D, 1)):
    fbud[n, c]   = sum over the taps of (n, c)      (|w| + S) * |texel * m| / 3
    gbud[texel]  = sum over the items on the texel  (|w| + S) * |gout * m| / 3
|w|: what an fp32 sum of the terms can lose; S: the fp32 rounding of a texel coordinate of magnitude S (and of 2 / box_warp),
which a unit step between texels turns into the value.  Where an interpolation fraction lies within 16 * S * 2^-24 of 0 or 1
the next texel outside the float64 footprint is credited too (weight 0, budget S * |.| / 3): fp32 may floor to the other
side and touch it with a weight of that size.  An element whose budget is 0 must come out exactly 0.

Acceptance, per element, no array-scale term:   |got - ref64| <= ATOL + KAPPA * 2^-24 * budget.

KAPPA = 4 x the worst ratio of torch's own fp32 CPU evaluation (grid_sample + autograd, an independent correct fp32
implementation; never the code under test) over the whole case table, rounded up.  The 4: the kernels sum through float
atomics in another order (tests/test_masked_loss_gpu.py uses the same factor for the same reason).
tests/test_planes_ref_host.py measures the ratio, prints it and asserts worst <= KAPPA / 4.
Measured: see KAPPA_MEASURED below.
"""
import functools
import itertools
import os
import re
import zlib
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from gaussian_gan_decoder_amd.decoder import PLANE_AXES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "gaussian_gan_decoder_amd", "csrc", "ggd_triplane.hip")).read()


def _const(name):
    return int(re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", _SRC).group(1))


SR_CHUNK, SR_MOD_LDS, SR_MIN_POINTS = _const("SR_CHUNK"), _const("SR_MOD_LDS"), _const("SR_MIN_POINTS")
SORT_TILE = 4096          # items per tile of the 32-bit sort the sorted-run backward uses (case E's 65 / 64 edge)

ATOL = 1e-7
U = 2.0 ** -24
KAPPA_MEASURED = 1.261     # worst |torch fp32 - ref64| / (2^-24 * budget) over the table (test_planes_ref_host.py prints it)
KAPPA = 6


def plane_perm(axes):
    """perm[p][a]: which coordinate plane p reads on its axis a (u, v, w), from PLANE_AXES as sample_from_planes uses it."""
    inv = np.linalg.inv(PLANE_AXES[axes].double().numpy())          # proj[p, :, a] = sum_c coords[:, c] * inv[p, c, a]
    return [[int(np.argmax(np.abs(inv[p][:, a]))) for a in range(3)] for p in range(3)]


def _axis_terms(x64, perm_p, sizes):
    fl, fr = [], []
    for a, size in enumerate(sizes):
        i = ((x64[:, perm_p[a]] + 1.0) * size - 1.0) / 2.0
        f = torch.floor(i)
        fl.append(f)
        fr.append(i - f)                                             # NaN for +-inf rows: every comparison below is false
    return fl, fr


def reference(planes, pos, gout, box_warp, axes, D, mod=None, device="cpu"):
    """planes [3, C * max(D, 1), H, W], pos [N, 3], gout [N, C], mod [max(D, 1), C] or None (D: 0 / None = 2-D planes)
    -> float64 (feat [N, C], grad like planes, fbud [N, C], gbud like planes) on `device`."""
    dev = torch.device(device)
    D = int(D or 0)
    Dd = max(D, 1)
    _, CD, H, W = planes.shape
    C = CD // Dd
    N = pos.shape[0]
    f64 = dict(dtype=torch.float64, device=dev)
    tex = planes.detach().to(**f64).view(3, C, Dd, H, W).permute(0, 2, 3, 4, 1).reshape(3 * Dd * H * W, C)
    m = torch.ones(Dd, C, **f64) if mod is None else mod.detach().to(**f64).view(Dd, C)
    x64 = (2.0 / box_warp) * pos.detach().to(**f64)
    g = gout.detach().to(**f64)
    sizes = (W, H, D) if D > 0 else (W, H)
    S = float(max(W, H, Dd))
    eps = 16.0 * S * U
    feat, fbud = torch.zeros(N, C, **f64), torch.zeros(N, C, **f64)
    grad, gbud = torch.zeros_like(tex), torch.zeros_like(tex)
    perm = plane_perm(axes)

    def scatter(dst, idx, src):
        """dst[idx] += src.  Many items per texel (one cell holding every point) make a device's float64 index_add_ crawl on a
        few addresses: the items are then dealt over K private copies of dst, summed afterwards (untouched texels stay 0)."""
        M = dst.shape[0]
        K = min(256, idx.shape[0] // (4 * M), (1 << 22) // (M * C))
        if K < 2:
            dst.index_add_(0, idx, src)
            return
        tmp = torch.zeros(M * K, C, **f64)
        tmp.index_add_(0, idx * K + torch.arange(idx.shape[0], device=dev) % K, src)
        dst += tmp.view(M, K, C).sum(1)

    def add(p, rows, fl, fr, offs):
        """one tap (offsets per axis; -1 / 2: the credited neighbours, weight 0) of the given rows on plane p"""
        w = torch.ones(rows.shape[0], **f64)
        ok = torch.ones(rows.shape[0], dtype=torch.bool, device=dev)
        cell = []
        for a, o in enumerate(offs):
            f, r = fl[a][rows], fr[a][rows]
            c = f + o
            ok &= (c >= 0) & (c <= sizes[a] - 1)
            if o == 0:
                w = w * (1.0 - r)
            elif o == 1:
                w = w * r
            else:
                ok &= (r < eps) if o == -1 else (r > 1.0 - eps)
                w = w * 0.0
            cell.append(c)
        sel = ok.nonzero().squeeze(1)
        if sel.numel() == 0:
            return
        xi, yi = cell[0][sel].long(), cell[1][sel].long()
        zi = cell[2][sel].long() if D > 0 else torch.zeros_like(xi)
        idx = ((p * Dd + zi) * H + yi) * W + xi
        n = rows[sel]
        ws = w[sel][:, None]
        bs = (ws.abs() + S) / 3.0
        t = tex[idx] * m[zi]
        gm = g[n] * m[zi]
        feat.index_add_(0, n, ws * t / 3.0)
        fbud.index_add_(0, n, bs * t.abs())
        scatter(grad, idx, ws * gm / 3.0)
        scatter(gbud, idx, bs * gm.abs())

    every = torch.arange(N, device=dev)
    for p in range(3):
        fl, fr = _axis_terms(x64, perm[p], sizes)
        for offs in itertools.product((0, 1), repeat=len(sizes)):
            add(p, every, fl, fr, offs)
        near = torch.zeros(N, dtype=torch.bool, device=dev)
        for a in range(len(sizes)):
            near |= ((fr[a] < eps) | (fr[a] > 1.0 - eps)) & (fl[a].abs() < 1e9)
        rows = near.nonzero().squeeze(1)
        if rows.numel():
            for offs in itertools.product((-1, 0, 1, 2), repeat=len(sizes)):
                if any(o in (-1, 2) for o in offs):
                    add(p, rows, fl, fr, offs)

    def back(a):
        return a.view(3, Dd, H, W, C).permute(0, 4, 1, 2, 3).reshape(3, C * Dd, H, W)
    return feat, back(grad), fbud, back(gbud)


def channels_last(a, D):
    """[3, C * max(D, 1), H, W] (planes' shape) -> [3, max(D, 1), H, W, C], the layout of the C ABI's gradient buffer"""
    Dd = max(int(D or 0), 1)
    _, CD, H, W = a.shape
    return a.view(3, CD // Dd, Dd, H, W).permute(0, 2, 3, 4, 1).contiguous()


def item_stats(pos, box_warp, axes, D, H, W, dtype=np.float64):
    """per (plane, point) item: taps inside the grid [3, N], and kept [3, N] by sr_item's rule (-1 <= floor(i) <= size - 1 on
    every used axis).  dtype = np.float32 repeats the kernel's own arithmetic (scale = 2 / box_warp in fp32)."""
    D = int(D or 0)
    sizes = (W, H, D) if D > 0 else (W, H)
    perm = plane_perm(axes)
    ft = dtype
    x = (ft(2.0) / ft(box_warp)) * pos.detach().cpu().numpy().astype(ft)
    N = x.shape[0]
    taps, kept = np.zeros((3, N), np.int64), np.zeros((3, N), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(3):
            cnt, ok = np.ones(N, np.int64), np.ones(N, bool)
            for a, size in enumerate(sizes):
                f = np.floor(((x[:, perm[p][a]] + ft(1.0)) * ft(size) - ft(1.0)) * ft(0.5))
                cnt = cnt * (((f >= 0) & (f <= size - 1)).astype(np.int64) + ((f + 1 >= 0) & (f + 1 <= size - 1)).astype(np.int64))
                ok &= (f >= -1) & (f <= size - 1)
            taps[p], kept[p] = cnt, ok
    return taps, kept


def worst_ratio(got, ref, bud):
    """max over the elements of (|got - ref| - ATOL) / (2^-24 * budget); inf if an element of zero budget is not exactly 0"""
    err = (got.to(torch.float64) - ref).abs()
    zero = bud == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    if bool(zero.all()):
        return 0.0
    return float(((err[~zero] - ATOL).clamp_min(0.0) / (U * bud[~zero])).max())


def assert_within(got, ref, bud, what, extra=None):
    """|got - ref| <= ATOL + KAPPA * 2^-24 * bud (+ extra) for every element; a zero budget means exactly 0"""
    assert got.numel() == ref.numel() == bud.numel(), f"{what}: {tuple(got.shape)} against {tuple(ref.shape)}"
    got = got.reshape(ref.shape)            # ([3, H, W, C] and [3, 1, H, W, C] are the same buffer)
    extra = None if extra is None else extra.reshape(ref.shape)
    err = (got.to(torch.float64) - ref).abs()
    assert bool(torch.isfinite(err).all()), f"{what}: non-finite values"
    bound = ATOL + KAPPA * U * bud
    zero = bud == 0
    if extra is not None:
        bound = bound + extra
        zero = zero & (extra == 0)
    bad0 = zero & (err != 0)
    assert not bool(bad0.any()), f"{what}: {int(bad0.sum())} elements of zero budget are not exactly 0 (max {float(err[bad0].max()):.3e})"
    over = err > bound
    if bool(over.any()):
        k = int(torch.argmax((err - bound).flatten()))
        raise AssertionError(f"{what}: {int(over.sum())} of {err.numel()} elements over budget; worst at flat index {k}: "
                             f"|got - ref| = {float(err.flatten()[k]):.3e}, bound {float(bound.flatten()[k]):.3e}, "
                             f"ref {float(ref.flatten()[k]):.6e}")


# ---- the case table ------------------------------------------------------------------------------------------------------
# layout: mixed = edge rows, 10 % texel centres, 2 % uniform in 1.3 x the box, the rest uniform in the box;
#         shuffled = mixed, shuffled (group B takes the first N rows of one pool);  kept = exactly `kept` items survive;
#         tiles = mixed with `far` points at 5.0;  onecell / onepoint = every non-edge row in one cell / at one position
Case = namedtuple("Case", "name group C D H W axes N box_warp mod layout gen_N kept far taps_check")


def _case(name, group, C, D, H, W, axes, N, box_warp, mod, layout="mixed", gen_N=None, kept=None, far=0, taps_check=True):
    return Case(name, group, C, D, H, W, axes, N, box_warp, mod, layout, gen_N or N, kept, far, taps_check)


def edge_rows(box_warp, sizes):
    """the rows every case carries: box corners, face centres, edge midpoints, half a texel and one texel beyond every face
    (for every grid size in use), first and last texel centres, +-1e30 and +-inf in one coordinate"""
    h, inner = 0.5 * box_warp, 0.137 * box_warp
    rows = [[sx * h, sy * h, sz * h] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    for a in range(3):
        for s in (-1, 1):
            r = [0.0, 0.0, 0.0]; r[a] = s * h; rows.append(r)
    for a in range(3):                                    # two coordinates on faces: the 2-tap items of a tri-grid
        for s, t in itertools.product((-1, 1), repeat=2):
            r = [0.0, 0.0, 0.0]; r[a] = s * h; r[(a + 1) % 3] = t * h; rows.append(r)
    for size in sizes:
        for a in range(3):
            for s in (-1, 1):
                for beyond in (0.5 / size, 1.0 / size):
                    r = [inner] * 3; r[a] = s * (0.5 + beyond) * box_warp; rows.append(r)
            for t in (0, size - 1):
                r = [inner] * 3; r[a] = ((t + 0.5) / size - 0.5) * box_warp; rows.append(r)
    for a in range(3):
        for v in (1e30, -1e30, float("inf"), -float("inf")):
            r = [inner] * 3; r[a] = v; rows.append(r)
    return torch.tensor(rows, dtype=torch.float64)


def _sizes(c):
    return sorted({c.W, c.H} | ({c.D} if c.D > 1 else set()))


def _mixed(c, n, g):
    """n rows: 10 % on texel centres, 2 % uniform in 1.3 x the box, the rest uniform inside it (float64)"""
    sizes = torch.tensor(_sizes(c), dtype=torch.float64)
    pos = (torch.rand(n, 3, generator=g, dtype=torch.float64) - 0.5) * 0.98 * c.box_warp
    n_c, n_o = n // 10, n // 50
    sz = sizes[torch.randint(0, len(sizes), (n_c, 3), generator=g)]
    pos[:n_c] = ((torch.floor(torch.rand(n_c, 3, generator=g, dtype=torch.float64) * sz) + 0.5) / sz - 0.5) * c.box_warp
    pos[n_c:n_c + n_o] = (torch.rand(n_o, 3, generator=g, dtype=torch.float64) - 0.5) * 1.3 * c.box_warp
    return pos


def _positions(c, g):
    n = c.gen_N
    edge = edge_rows(c.box_warp, _sizes(c))
    E = edge.shape[0]
    if c.layout == "shuffled":
        pool = torch.cat([edge, _mixed(c, max(n, 4 * E) - E, g)])
        return pool[torch.randperm(pool.shape[0], generator=g)][:n]
    if c.layout in ("mixed", "tiles"):
        pos = torch.cat([edge, _mixed(c, n - E, g)])
        if c.far:
            pos[E + torch.randperm(n - E, generator=g)[:c.far]] = 5.0
        return pos
    if c.layout in ("onecell", "onepoint"):
        # every coordinate between the centres of texels 2 and 3 of an 8-texel axis: one cell on every plane
        lo = torch.tensor([(2.0 + 0.5) / 8 - 0.5] * 3, dtype=torch.float64) * c.box_warp
        frac = torch.rand(n - E, 3, generator=g, dtype=torch.float64) if c.layout == "onecell" else \
            torch.full((n - E, 3), 0.3, dtype=torch.float64)
        return torch.cat([edge, lo + 0.98 * frac * c.box_warp / 8])
    if c.layout == "uniform":
        return torch.cat([edge, (torch.rand(n - E, 3, generator=g, dtype=torch.float64) - 0.5) * 0.98 * c.box_warp])
    assert c.layout == "kept" and c.D == 0
    core = (torch.rand(n - E, 3, generator=g, dtype=torch.float64) - 0.5) * 0.9 * c.box_warp   # all three items kept
    pos = torch.cat([core, edge]).float()
    _, kept = item_stats(pos, c.box_warp, c.axes, c.D, c.H, c.W)
    # edge rows that drop items give way to interior rows where the target leaves no room for them
    for i in range(n - E, n):
        if int(kept.sum()) >= c.kept:
            break
        if not kept[:, i].all():
            pos[i] = pos[i - (n - E)]
            kept[:, i] = True
    drop = int(kept.sum()) - c.kept
    assert drop >= 0
    far = 5.0 * c.box_warp
    q = min(drop // 3, n - E)              # the core rows keep three items each: whole rows first
    pos[:q, 1:] = far
    drop -= 3 * q
    for i in range(q, n):                  # y far: drops plane 0's item; z far: drops the items of planes 1 and 2
        if drop == 0:
            break
        k0, k12 = int(kept[0, i]), int(kept[1, i]) + int(kept[2, i])
        if k0 + k12 == 0:
            continue
        if drop >= k0 + k12:
            pos[i, 1] = far; pos[i, 2] = far; drop -= k0 + k12
        elif drop == k0:
            pos[i, 1] = far; drop = 0
        elif drop == k12:
            pos[i, 2] = far; drop = 0
    assert drop == 0
    return pos


@functools.lru_cache(maxsize=16)
def build(c):
    """the inputs of a case (CPU float32): planes [3, C * max(D, 1), H, W], pos [N, 3], gout [N, C], mod or None.
    Cases that differ in N only (gen_N equal) share their leading rows."""
    seed = zlib.crc32(repr(c._replace(name="", group="", N=0)).encode())
    g = torch.Generator().manual_seed(seed)
    Dd = max(c.D, 1)
    planes = torch.randn(3, c.C * Dd, c.H, c.W, generator=g)
    mod = (1.0 + 0.25 * torch.randn(Dd, c.C, generator=g)) if c.mod else None
    gout = torch.randn(c.gen_N, c.C, generator=g)
    pos = _positions(c, g).float()
    assert pos.shape == (c.gen_N, 3)
    return SimpleNamespace(planes=planes, pos=pos[:c.N].contiguous(), gout=gout[:c.N].contiguous(), mod=mod)


def points_per_wave(C, gather):
    """points per wave of the kernel that runs: gather4_kernel (four channels per lane) for the gather with C in {16, 32, 64},
    plane_kernel (lane = channel) else"""
    return 256 // C if gather and C in (16, 32, 64) else 64 // C


B_SENTINEL_ROWS = 64      # rows of the pool behind row N that group B hands to the kernels (they must not be touched)


def _table():
    t = []
    geoms = [(0, "eg3d"), (3, "eg3d"), (2, "panohead")]
    # A: every instance of the plain forms
    for ci, C in enumerate((1, 2, 4, 8, 16, 32, 64)):
        for gi, (D, axes) in enumerate(geoms):
            for mod in (False, True):
                bw = 0.7 if (ci + gi + int(mod)) % 2 == 0 else 4.0
                t.append(_case(f"A-C{C}-D{D}-{axes}-{'mod' if mod else 'plain'}", "A", C, D, 12, 20, axes, 2051, bw, mod))
    # B: wave and workgroup edges (direct calls); one pool per (C, D), the first N rows.  The "every number of taps" self-check
    # holds from N = 255 on (C = 1); the edges below it (N = 1 .. 33) have too few rows to carry every kind of item.
    for C in (1, 32, 64):
        for D in (0, 2):
            for gather in (True, False):
                P = points_per_wave(C, gather)
                for N in sorted({n for n in (1, P - 1, P, P + 1, 4 * P - 1, 4 * P, 4 * P + 1) if n >= 1}):
                    t.append(_case(f"B-{'gather' if gather else 'scatter'}-C{C}-D{D}-N{N}", "B" + ("g" if gather else "s"), C, D, 12, 20,
                                   "panohead" if D else "eg3d", N, 0.7 if D else 4.0, C != 32, "shuffled", 4 * 64 + 1 + B_SENTINEL_ROWS,
                                   taps_check=N >= 255))
    # C: sorted form and plain form on both sides of the switch
    for C, Dbig in ((64, 17), (32, 33), (16, 65)):
        for tag, D, H, W, axes, mod in (("2d-plain", 0, 8, 8, "eg3d", False), ("2d-lds", 0, 8, 8, "eg3d", True),
                                        ("eg3d-plain", 3, 8, 8, "eg3d", False), ("eg3d-lds", 3, 8, 8, "eg3d", True),
                                        ("panohead-plain", 3, 8, 8, "panohead", False), ("panohead-lds", 3, 8, 8, "panohead", True),
                                        ("global", Dbig, 6, 6, "eg3d" if C == 32 else "panohead", True)):
            for N in (SR_MIN_POINTS, SR_MIN_POINTS - 1):
                t.append(_case(f"C-C{C}-{tag}-N{N}", "C", C, D, H, W, axes, N, 4.0 if tag.startswith("2d") else 0.7, mod,
                               gen_N=SR_MIN_POINTS))
    # D: kept-item counts on and next to the chunk / stream edges (box_warp 1 and 8 x 8: every edge row is exact in fp32).
    # A kept count below 3 N - 1 is reached by moving rows far outside, the edge rows that drop items first: only the
    # 3 N - 1 case still carries every kind of item, so only it takes the "every number of taps" self-check.
    for C in (16, 64):
        for k in (0, 1, SR_CHUNK - 1, SR_CHUNK, SR_CHUNK + 1, 4 * SR_CHUNK - 1, 4 * SR_CHUNK, 4 * SR_CHUNK + 1, 3 * SR_MIN_POINTS - 1):
            t.append(_case(f"D-C{C}-kept{k}", "D", C, 0, 8, 8, "eg3d", SR_MIN_POINTS, 1.0, False, "kept", kept=k,
                           taps_check=k == 3 * SR_MIN_POINTS - 1))
    # E: 65 launched sort tiles, 64 live
    t.append(_case("E-lookback-65-64", "E", 32, 0, 64, 64, "eg3d", 88_000, 1.0, False, "tiles", far=700))
    # F: run lengths
    n_edge = edge_rows(1.0, [8]).shape[0]
    t.append(_case("F-one-cell", "F", 32, 0, 8, 8, "eg3d", SR_MIN_POINTS + n_edge, 1.0, True, "onecell"))
    t.append(_case("F-one-position", "F", 64, 0, 8, 8, "eg3d", SR_MIN_POINTS + n_edge, 1.0, False, "onepoint"))
    t.append(_case("F-short-runs", "F", 16, 0, 256, 256, "eg3d", SR_MIN_POINTS, 0.7, False, "uniform"))
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def group(*names):
    return [c for c in CASES if c.group in names]


# G (accumulate) reuses cases of A (plain form) and C (sorted form)
ACCUMULATE_CASES = [BY_NAME[n] for n in ("A-C8-D0-eg3d-mod", "A-C32-D2-panohead-plain", f"C-C32-2d-lds-N{SR_MIN_POINTS}",
                                         f"C-C64-eg3d-lds-N{SR_MIN_POINTS}", f"C-C16-panohead-plain-N{SR_MIN_POINTS}",
                                         f"C-C16-global-N{SR_MIN_POINTS}")]


@functools.lru_cache(maxsize=8)
def reference_of(c, device="cpu"):
    b = build(c)
    return reference(b.planes, b.pos, b.gout, c.box_warp, c.axes, c.D, b.mod, device)
