"""Case tables that reach every feature-map kernel instance (csrc/ggd_features.hip: EXP_MODE x channel group, each with the
colour pass's pre-cull on and off) and every shape of stage_round's compaction by construction.  CPU only:
tests/test_features_cases_host.py proves the tables sound against the oracle, tests/test_features_instances_gpu.py runs them.

A case is a dict: id, table ("F" or "Q"), scene (a key of _instance_cases.SCENES; table F) or layout (a key of LAYOUTS; table Q),
C, bg (bool: feature_bg given or None) and options {exp_mode, cull, ...}.  `inputs(case)` builds the activated inputs,
`reference(case)` the CPU oracle forward with its fragile-pixel mask, `features(P, C)` the signed feature rows and background;
all cached: do not modify.  The launchers' dispatch rules are restated at the bottom, and `staged_counts` restates what
stage_round stages per (quarter, round)."""
from __future__ import annotations

import functools

import numpy as np
import torch

import _instance_cases as IC
from _util import run_oracle, scene_inputs

ROUND = 64      # list entries per round (GGD_FEATURES_ROUND; the GPU tests check it against the library's)
FLUSH = 32      # staged records per chunk of the backward's flush


# ---- the launchers' rules (csrc/ggd_features.hip::ggd_launch_features_forward / _backward)
def channel_group(C):
    """CG: C rounded up to 4 / 8 / 16 / 32"""
    assert 1 <= C <= 32
    return 4 if C <= 4 else (8 if C <= 8 else (16 if C <= 16 else 32))


def forward_instance(case):
    em = case["options"]["exp_mode"]
    return f"features_forward_kernel<{1 if em == 3 else em}, {channel_group(case['C'])}>"


def backward_instance(case):
    return f"features_backward_kernel<{case['options']['exp_mode']}, {channel_group(case['C'])}>"


@functools.lru_cache(maxsize=None)
def features(P, C, given=True):
    """(features [P, C], feature_bg [C] or None), both uniform in [-1, 1): the normals that ride this pass are signed.  Seeded per
    (P, C); cached: do not modify"""
    gen = torch.Generator().manual_seed(31000 + 41 * P + C)
    f = 2.0 * torch.rand(P, C, generator=gen) - 1.0
    bg = 2.0 * torch.rand(C, generator=gen) - 1.0
    return f.contiguous(), (bg if given else None)


# ---- table F: general scenes (those the C = 32 tests of tests/test_features_gpu.py already use), every exp mode at C on and
# behind a group edge (4, 8, 16: no padding channel; 9, 17: the most) and at 31.  Within an exp mode the two C of the groups 16
# and 32 share a scene and differ in the cull; the groups 4 and 8 take the other cull in the next mode.
F_CHANNELS = (4, 8, 9, 16, 17, 31)


def _table_f():
    out = []
    for em in (0, 1, 2, 3):
        for i, Cn in enumerate(F_CHANNELS):
            scene = ("A1", "A2")[(i // 2 + em) % 2]
            cull, bg = (i + em) % 2, (i // 2 + i) % 2 == 0
            out.append(dict(id=f"{scene}-exp{em}-C{Cn}-cull{cull}-{'bg' if bg else 'nobg'}", table="F", scene=scene, layout=None,
                            C=Cn, bg=bg, options=dict(IC.DEFAULTS, exp_mode=em, cull=cull)))
    return out


# ---- table Q: hand-built scenes of ONE 16 x 16 tile (four quarters, sub = (qy0 / 8) * 2 + qx0 / 8).  Camera of
# scene_inputs(P=k, size=16, seed=7); isotropic splats with identity quaternions whose centres are computed from a pixel position
# and a view-space depth through the inverse view matrix; the depth rises by 1e-3 per index, so the tile's list is the index
# order.  A layout is a list of (quarter, count, kind) blocks in depth order:
#   faint    opacity 0.04 (ragged: 0.03), scale 0.65 px (sigma 0.85 px with the 0.3 low-pass, >= 1/255 within 1.84 px), centre
#            uniformly within +-1 px of the quarter's centre q0 + 3.5: the footprint ends >= 0.65 px inside the quarter's own pixel
#            rectangle and >= 1.65 px from any other quarter's, so the box test of the pre-cull alone decides what a quarter stages
#   opaque   opacity 0.95, scale 0.2 px (sigma 0.58 px), centred ON the pixel (q0 + 3, q0 + 3): that pixel's transmittance goes
#            0.05, 2.5e-3, 1.25e-4 and the fourth of the stack stops it (6e-6 < 1e-4; no step within 2e-5 of the stop), its
#            neighbours keep T >= 0.2
#   dead     opacity 0.002 < 1 / 255: in the list, blended by no pixel (its dL_dfeatures row must stay exactly 0); always last, so
#            no n_contrib reaches it and the rounds of the blocks before it are unmoved
DEAD = (1, 1, "dead")
LAYOUTS = {
    # quarter 3's forward sees rounds of 0, 64, 0, 1 survivors, its backward 1, 63, 1, 0; quarter 0's 64, 0, 64 both ways;
    # quarters 1 and 2 blend nothing
    "empty-rounds": [(0, 64, "faint"), (3, 64, "faint"), (0, 64, "faint"), (3, 1, "faint"), DEAD],
    # quarter 1: forward 33, 32, 1, backward 32, 33, 1; quarter 2: 31, 32 and 32, 31 -- the survivor counts around FLUSH
    "flush-edges": [(1, 33, "faint"), (2, 31, "faint"), (1, 32, "faint"), (2, 32, "faint"), (1, 1, "faint"), DEAD],
    # one quarter whose lanes end at very different positions: the stacked pixel stops in the first round, pixels near the centre go
    # on past position 129, the corners see nothing
    "ragged": [(2, 5, "opaque"), (2, 140, "faint-ragged"), DEAD],
}
# what each quarter stages per round with the pre-cull on, in the kernel's order (the host test derives it from the oracle's records,
# the GPU tests from the library's own)
Q_STAGED = {
    "empty-rounds": dict(forward=[[64, 0, 64], [], [], [0, 64, 0, 1]], backward=[[64, 0, 64], [], [], [1, 63, 1, 0]]),
    "flush-edges": dict(forward=[[], [33, 32, 1], [31, 32], []], backward=[[], [32, 33, 1], [32, 31], []]),
    "ragged": dict(forward=[[], [], [64, 64, 17], []], backward=[[], [], [64, 64, 17], []]),
}
KINDS = {"faint": (0.04, 0.65), "faint-ragged": (0.03, 0.65), "opaque": (0.95, 0.2), "dead": (0.002, 0.65)}
Q_SIZE = 16
Q_SEED = {"empty-rounds": 1, "flush-edges": 2, "ragged": 3}   # of the centres' jitter (chosen on the oracle alone: the host caps)
Q_CHANNELS = (1, 4, 5, 8, 9, 16, 17, 32)
Q_MODE_CHANNELS = (4, 5, 9, 17)    # one C per channel group for the exp modes 0 .. 2


def quarter_origin(sub):
    """(qx0, qy0) of quarter `sub` of the tile at the origin"""
    return (sub & 1) * 8, (sub >> 1) * 8


def quarter_maxn(n_contrib, sub):
    """the deepest last contributor over the pixels of quarter `sub` of the tile at the origin: the entries its rounds walk"""
    qx0, qy0 = quarter_origin(sub)
    return int(n_contrib[qy0:qy0 + 8, qx0:qx0 + 8].max(initial=0))


def layout_quarters(name):
    """the quarter of every splat of a layout, in index (= list) order"""
    return np.concatenate([np.full(n, q) for q, n, _ in LAYOUTS[name]])


def layout_kinds(name):
    return np.concatenate([np.full(n, k) for _, n, k in LAYOUTS[name]])


@functools.lru_cache(maxsize=None)
def layout_inputs(name, depth_step=1e-3, seed=None):
    """the activated inputs of a table Q layout (cached: do not modify).  depth_step: the rise of the view-space depth per index
    (the footprints stay constant in pixels: the scale follows z); seed: of the centres' jitter, Q_SEED[name] by default"""
    blocks = LAYOUTS[name]
    k = sum(n for _, n, _ in blocks)
    d = scene_inputs(P=k, size=Q_SIZE, seed=7)
    W = H = Q_SIZE
    V = d["viewmatrix"].double().numpy()                     # row vectors: p_view = [p, 1] @ V
    Pm = np.linalg.inv(V) @ d["projmatrix"].double().numpy()   # p_hom = p_view @ Pm
    z0 = float((np.array([0.0, 0.0, 0.0, 1.0]) @ V)[2])       # depth of the look-at point
    focal = W / (2.0 * d["tanfovx"])
    rng = np.random.RandomState(7100 + (Q_SEED[name] if seed is None else seed))
    xyz, op, sc = np.zeros((k, 3)), np.zeros((k, 1)), np.zeros((k, 3))
    i = 0
    for q, n, kind in blocks:
        qx0, qy0 = quarter_origin(q)
        opacity, scale_px = KINDS[kind]
        for _ in range(n):
            if kind == "opaque":
                px, py = qx0 + 3.0, qy0 + 3.0
            else:
                px, py = qx0 + 3.5 + rng.uniform(-1.0, 1.0), qy0 + 3.5 + rng.uniform(-1.0, 1.0)
            z = z0 + depth_step * i
            nx, ny = (2.0 * px + 1.0) / W - 1.0, (2.0 * py + 1.0) / H - 1.0     # pixel = ((ndc + 1) S - 1) / 2
            # (xv, yv) with p_hom.xy / p_hom.w = (nx, ny) for p_view = (xv, yv, z, 1)
            A = np.array([[Pm[0, 0] - nx * Pm[0, 3], Pm[1, 0] - nx * Pm[1, 3]], [Pm[0, 1] - ny * Pm[0, 3], Pm[1, 1] - ny * Pm[1, 3]]])
            b = np.array([nx * (z * Pm[2, 3] + Pm[3, 3]) - z * Pm[2, 0] - Pm[3, 0], ny * (z * Pm[2, 3] + Pm[3, 3]) - z * Pm[2, 1] - Pm[3, 1]])
            xv, yv = np.linalg.solve(A, b)
            xyz[i] = (np.array([xv, yv, z, 1.0]) @ np.linalg.inv(V))[:3]
            op[i], sc[i] = opacity, scale_px * z / focal
            i += 1
    quat = torch.zeros(k, 4); quat[:, 0] = 1.0
    t = lambda a: torch.from_numpy(a.astype(np.float32)).contiguous()
    return dict(d, means3D=t(xyz), opacities=t(op), scales=t(sc), rotations=quat.contiguous())


def _table_q():
    out = []
    for name in LAYOUTS:
        for em, channels in ((3, Q_CHANNELS), (0, Q_MODE_CHANNELS), (1, Q_MODE_CHANNELS), (2, Q_MODE_CHANNELS)):
            for i, Cn in enumerate(channels):
                for cull in (0, 1):
                    bg = (i + cull) % 2 == 0
                    out.append(dict(id=f"{name}-exp{em}-C{Cn}-cull{cull}-{'bg' if bg else 'nobg'}", table="Q", scene=None,
                                    layout=name, C=Cn, bg=bg, options=dict(IC.DEFAULTS, exp_mode=em, cull=cull)))
    return out


TABLE_F = _table_f()
TABLE_Q = _table_q()


def inputs(case):
    """the activated inputs of a case (cached: do not modify)"""
    return layout_inputs(case["layout"]) if case["table"] == "Q" else IC.inputs(dict(scene=case["scene"]))


def reference(case):
    """dict(o, frag): the oracle forward of a case and its fragile-pixel mask (cached: do not modify)"""
    if case["table"] == "Q":
        return _layout_reference(case["layout"])
    r = IC.reference(dict(scene=case["scene"], feature="aux"))
    return dict(o=r["o"], frag=r["frag"])


@functools.lru_cache(maxsize=None)
def _layout_reference(name):
    from oracle import ggd_oracle as O
    o = run_oracle(layout_inputs(name))
    return dict(o=o, frag=O.fragile_pixels(o))


def case_features(case):
    return features(inputs(case)["P"], case["C"], case["bg"])


def upstream(case, frag_px):
    """N(0, 1) upstream gradients (colour [3, H, W], feature map [C, H, W]) of a case, zero on the pixels of the bool mask"""
    d = inputs(case)
    g, _, _ = IC.upstream_gradients(d["H"], d["W"], frag_px)
    gF = torch.randn(case["C"], d["H"], d["W"], generator=torch.Generator().manual_seed(IC.GRAD_SEED + 100 + case["C"]))
    gF[:, torch.from_numpy(frag_px)] = 0.0
    return g, gF


def fragile_counts(case):
    """(fragile pixels, fragile Gaussians) of a case from the oracle alone: its fragile-pixel mask, and the feature backward's
    reference (tests/_features_ref.py::backward_ref: colour and every channel triple) on the oracle's OWN final_T / n_contrib / lists"""
    return _fragile_counts(case["scene"], case["layout"], case["C"], case["bg"])


@functools.lru_cache(maxsize=None)
def _fragile_counts(scene, layout, Cn, bg):
    import _features_ref as FR
    case = dict(table="Q" if layout else "F", scene=scene, layout=layout, C=Cn, bg=bg)
    d, r = inputs(case), reference(case)
    o = r["o"]
    f, b = case_features(case)
    g, gF = upstream(case, r["frag"])
    own = dict(o, radii=torch.from_numpy(o["radii"]))
    _, _, frag = FR.backward_ref(d, o, own, g.numpy(), f.numpy(), None if b is None else b.numpy(), gF.numpy())
    return int(r["frag"].sum()), int((frag > 0).sum())


def caps(case):
    """half of the caps the helpers assert, as _instance_cases.caps: (1, 2) for table Q"""
    d = inputs(case)
    return (2 + d["W"] * d["H"] // 5000) // 2, max(4, d["P"] // 1000) // 2


# ---- what the oracle forward says about a layout
def footprint_radius(conic_opacity):
    """radius [P] of the alpha >= 1/255 footprint of isotropic records: sqrt(2 ln(255 o) / A), 0 where o < 1/255"""
    co = np.asarray(conic_opacity, np.float64)
    with np.errstate(all="ignore"):
        r = np.sqrt(2.0 * np.log(255.0 * co[:, 3]) / co[:, 0])
    return np.where(255.0 * co[:, 3] >= 1.0, r, 0.0)


def oracle_records(o):
    """the oracle forward's records in the form staged_counts reads a native forward's: xy and, as the pre-cull's half extents,
    the footprint radius (-inf under the alpha floor, as the preprocess kernel stores it)"""
    r = footprint_radius(o["conic_opacity"])
    ex = np.where(255.0 * o["conic_opacity"][:, 3].astype(np.float64) >= 1.0, r, -np.inf).astype(np.float32)
    return dict(xy=o["xy"].astype(np.float32), cull_extent=np.stack([ex, ex], 1))


def rect_distance(x, y, r, sub):
    """distance [P] from the footprints (centre x, y, radius r) to the pixel rectangle [q0, q0 + 7]^2 of quarter `sub` (<= 0: reaches it)"""
    qx0, qy0 = quarter_origin(sub)
    dx = np.maximum(np.maximum(qx0 - x, x - (qx0 + 7.0)), 0.0)
    dy = np.maximum(np.maximum(qy0 - y, y - (qy0 + 7.0)), 0.0)
    return np.hypot(dx, dy) - r


# ---- stage_round, restated: the number of records each round of each quarter stages
def _box_hits(x, y, ex, ey, wx0, wx1, wy0, wy1):
    """record_box_hits (csrc/ggd_blend_math.h) in float32"""
    with np.errstate(all="ignore"):
        return ~((x + ex < wx0) | (x - ex > wx1) | (y + ey < wy0) | (y - ey > wy1))


def round_bounds(maxn, direction):
    """[(first, end)] list positions of a quarter's rounds, in the order the kernel takes them: the forward's start at 0, 64, 128,
    ...; the backward's end at maxn and reach back ROUND entries each (the last one starts at 0)"""
    if direction == "forward":
        return [(b, min(b + ROUND, maxn)) for b in range(0, maxn, ROUND)]
    assert direction == "backward"
    out, cend = [], maxn
    while cend > 0:
        cstart = cend - ROUND if cend > ROUND else 0
        out.append((cstart, cend))
        cend = cstart
    return out


def staged_counts(records, point_list, ranges, n_contrib, cull, direction):
    """{(tile, sub): [survivors of each round, in the kernel's order]} for every quarter of every tile.  records: dict with xy
    [P, 2] and cull_extent [P, 2] float32 (a decoded forward's, or oracle_records).  With the cull on a record is staged where its
    box [x +- ex] x [y +- ey] meets the quarter's pixel rectangle [qx0, qx0 + 7] x [qy0, qy0 + 7] -- the first stage of the
    pre-cull; the exact second stage (record_reaches_block) is not restated: the table Q scenes are built so that the box test
    alone decides (a centre inside its rectangle passes the second stage, every other quarter's box test fails).  With the cull
    off every entry of a round is staged."""
    H, W = n_contrib.shape
    gx, gy = (W + 15) // 16, (H + 15) // 16
    f32 = np.float32
    xy, ext = np.asarray(records["xy"], f32), np.asarray(records["cull_extent"], f32)
    out = {}
    for tile in range(gx * gy):
        lo, hi = (int(v) for v in ranges[tile])
        hi = max(hi, lo)
        tx, ty = tile % gx, tile // gx
        for sub in range(4):
            qx0, qy0 = tx * 16 + (sub & 1) * 8, ty * 16 + (sub >> 1) * 8
            block = n_contrib[qy0:min(qy0 + 8, H), qx0:min(qx0 + 8, W)]
            maxn = int(min(int(block.max(initial=0)), hi - lo))
            counts = []
            for first, end in round_bounds(maxn, direction):
                ids = np.asarray(point_list[lo + first:lo + end], np.int64)
                if cull:
                    keep = _box_hits(xy[ids, 0], xy[ids, 1], ext[ids, 0], ext[ids, 1], f32(qx0), f32(qx0) + f32(7), f32(qy0),
                                     f32(qy0) + f32(7))
                    counts.append(int(keep.sum()))
                else:
                    counts.append(len(ids))
            out[(tile, sub)] = counts
    return out


def empty_round_between(counts):
    """a round without survivors lies between two rounds with some"""
    nz = [i for i, c in enumerate(counts) if c > 0]
    return bool(nz) and any(c == 0 for c in counts[nz[0]:nz[-1]])
