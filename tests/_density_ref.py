"""float64 restatement of the density field (csrc/ggd_density.hip: ggd_density_points / ggd_density_grid) with a per-element
error budget, and the case table of tests/test_density_host.py and tests/test_density_gpu.py.

The restatement, written out tap by tap:  f = the plane-mean features of tests/_planes_ref.py (reference(): no grid_sample, zero
padding with the inside test in floating point, so a +-inf, +-1e30 or NaN coordinate simply has no tap on the planes it
reaches);  z = W1 f + b1;  h = softplus(z);  o = W2 h + b2;  sigma = o[0];  rgb = act(o[1:33]).

Budgets (in units of 2^-24, like _planes_ref's; fbud is its feature budget):
    zbud[j] = sum_c |W1[j, c]| fbud[c]  +  |b1[j]| + sum_c |W1[j, c] f[c]|        the feature error through |W1|, plus what an
                                                                                   fp32 sum of the terms can lose
    hbud[j] = zbud[j] + 4 softplus(z[j])                                           softplus is 1-Lipschitz; a few ulp of its value
    obud[i] = sum_j |W2[i, j]| hbud[j]  +  |b2[i]| + sum_j |W2[i, j] h[j]|         the same propagation through the second layer
    sigma: obud[0];   rgb: slope * obud[1 + i] + 4 |rgb|                           slope = the activation's: 1.002 s (1 - s) for the
        sigmoid, sqrt(2) or 0.2 sqrt(2) for the lrelu (sqrt(2) wherever the fp32 pre-activation may lie on the other side of
        0), 1 for none; 4 |rgb|: the activation's own roundings (exp, divide, the two constants)

Acceptance, per element, no array-scale term:   |got - ref64| <= ATOL + KAPPA * 2^-24 * budget.

KAPPA = 2 x the worst ratio (|err| - ATOL) / (2^-24 * budget) of two independent fp32 implementations -- the values the
reference's own code produced (tests/golden/density_fixture.npz) and torch's fp32 CPU evaluation (grid_sample, F.linear,
F.softplus) of every case of the table; never the code under test -- rounded up.  The 2: the kernel sums in another order (the
MFMA's k-order against addmm's).  tests/test_density_host.py measures the ratio, prints it and asserts worst <= KAPPA / 2.
Measured: see KAPPA_MEASURED below.
"""
import functools
import math
import os
import re
import zlib
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from gaussian_gan_decoder_amd.decoder import PLANE_AXES
import _planes_ref as P

ROOT = P.ROOT
_SRC = open(os.path.join(ROOT, "gaussian_gan_decoder_amd", "csrc", "ggd_density.hip")).read()


def _const(name):
    return int(re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", _SRC).group(1))


T = _const("DN_POINTS")       # points per workgroup
ATOL = P.ATOL
U = P.U
KAPPA_MEASURED = 0.225          # worst ratio of the fixture's values and of torch's fp32 CPU evaluation (test_density_host.py prints it)
KAPPA = 1
H, W = 12, 10                 # plane size of every case: non-square, so that an H / W swap shows
ULPS = 4.0                    # "a few ulp": the softplus' and the activation's own roundings, in units of 2^-24 |value|
SQRT2 = math.sqrt(2.0)

worst_ratio = P.worst_ratio


def softplus64(z):
    return torch.where(z > 30.0, z, torch.log1p(torch.exp(z.clamp(max=30.0))))


def reference(planes, pos, box_warp, axes, D, w1, b1, w2, b2, act):
    """planes [3, 32 * max(D, 1), H, W], pos [N, 3], effective weights, act in ("sigmoid", "lrelu", "none")
    -> SimpleNamespace of float64 tensors: sigma [N], sbud [N], rgb [N, 32], rbud [N, 32], z [N, 64], fbud [N, 32]"""
    N = pos.shape[0]
    f, _, fbud, _ = P.reference(planes, pos, torch.zeros(N, 32), box_warp, axes, D)
    w1, b1, w2, b2 = (t.detach().double() for t in (w1, b1, w2, b2))
    z = f @ w1.t() + b1
    zbud = fbud @ w1.abs().t() + b1.abs() + f.abs() @ w1.abs().t()
    h = softplus64(z)
    hbud = zbud + ULPS * h
    o = h @ w2.t() + b2
    obud = hbud @ w2.abs().t() + b2.abs() + h @ w2.abs().t()
    pre, pbud = o[:, 1:], obud[:, 1:]
    if act == "sigmoid":
        s = torch.sigmoid(pre)
        rgb = s * 1.002 - 0.001
        slope = 1.002 * s * (1.0 - s)
    elif act == "lrelu":
        rgb = torch.where(pre > 0, pre, 0.2 * pre) * SQRT2
        slope = torch.where(pre > -(ATOL + 64.0 * U * pbud), SQRT2, 0.2 * SQRT2)
    else:
        rgb, slope = pre, torch.ones_like(pre)
    return SimpleNamespace(sigma=o[:, 0], sbud=obud[:, 0], rgb=rgb, rbud=slope * pbud + ULPS * rgb.abs(), z=z, fbud=fbud)


def assert_within(got, ref, bud, what):
    """|got - ref| <= ATOL + KAPPA * 2^-24 * bud for every element"""
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: {tuple(got.shape)} against {tuple(ref.shape)}"
    err = (got.detach().cpu().to(torch.float64) - ref).abs()
    assert bool(torch.isfinite(err).all()), f"{what}: non-finite values"
    bound = ATOL + KAPPA * U * bud
    over = err > bound
    if bool(over.any()):
        k = int(torch.argmax((err - bound).flatten()))
        raise AssertionError(f"{what}: {int(over.sum())} of {err.numel()} elements over budget; worst at flat index {k}: "
                             f"|got - ref| = {float(err.flatten()[k]):.3e}, bound {float(bound.flatten()[k]):.3e}, "
                             f"ref {float(ref.flatten()[k]):.6e}")


# ---- the case table ------------------------------------------------------------------------------------------------------
# Every case has one pool of POOL rows, shuffled: the edge rows of _planes_ref (box corners, faces, half a texel and a texel
# beyond every face, first / last texel centres, +-1e30, +-inf), a NaN in each coordinate and in all three, and _planes_ref's
# mixed rows (10 % texel centres, 2 % in 1.3 x the box, the rest inside).  The size cases take its first N rows.
Case = namedtuple("Case", "name D axes act lr_mul box_warp w1_scale")
POOL = 3 * T + 5
SENTINEL_ROWS = 64            # rows behind row N of an over-allocated output that must stay untouched
SIZES = sorted({1, 7, 8, 9, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5})
FORMS = [(0, "eg3d"), (1, "eg3d"), (1, "panohead"), (3, "eg3d"), (3, "panohead")]
ACTS = ("sigmoid", "lrelu", "none")


def _table():
    t = []
    for fi, (D, axes) in enumerate(FORMS):
        for ai, act in enumerate(ACTS):
            lr = 1.0 if (fi + ai) % 2 == 0 else 2.0
            t.append(Case(f"D{D}-{axes}-{act}-lr{lr:g}", D, axes, act, lr, 0.7 if (fi + ai) % 3 == 0 else 1.0, 1.0))
    # pre-activations of the softplus beyond +-25 (its threshold is 20) and +-90 (e^-90 is subnormal in fp32)
    t.append(Case("softplus-range-D3-panohead-none", 3, "panohead", "none", 1.0, 1.0, 150.0))
    t.append(Case("softplus-range-D0-eg3d-sigmoid", 0, "eg3d", "sigmoid", 2.0, 1.0, 150.0))
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
FORM_CASES = [c for c in CASES if c.w1_scale == 1.0]
RANGE_CASES = [c for c in CASES if c.w1_scale != 1.0]
SIZE_CASES = [BY_NAME["D3-panohead-none-lr1"], BY_NAME["D0-eg3d-sigmoid-lr1"]]


def layer(weight, bias, lr_mul):
    """what osg_weights reads of a FullyConnectedLayer (networks_stylegan2.py:109-112)"""
    return SimpleNamespace(weight=weight, bias=bias, weight_gain=lr_mul / np.sqrt(weight.shape[1]), bias_gain=lr_mul)


@functools.lru_cache(maxsize=None)
def build(c):
    """the inputs of a case (CPU float32): planes [3, 32 * max(D, 1), H, W], pos [POOL, 3], decoder (duck-typed OSGDecoder)"""
    g = torch.Generator().manual_seed(zlib.crc32(repr(c).encode()))
    Dd = max(c.D, 1)
    planes = torch.randn(3, 32 * Dd, H, W, generator=g)
    net = [layer(c.w1_scale * torch.randn(64, 32, generator=g) / c.lr_mul, 0.5 * torch.randn(64, generator=g), c.lr_mul), None,
           layer(torch.randn(33, 64, generator=g) / c.lr_mul, 0.5 * torch.randn(33, generator=g), c.lr_mul)]
    pc = P._case("", "", 32, c.D, H, W, c.axes, POOL, c.box_warp, False)
    edge = P.edge_rows(c.box_warp, P._sizes(pc))
    nan = torch.full((4, 3), 0.137 * c.box_warp, dtype=torch.float64)
    for a in range(3):
        nan[a, a] = float("nan")
    nan[3, :] = float("nan")
    pool = torch.cat([edge, nan, P._mixed(pc, POOL - edge.shape[0] - 4, g)])
    pos = pool[torch.randperm(POOL, generator=g)].float().contiguous()
    return SimpleNamespace(planes=planes, pos=pos, decoder=SimpleNamespace(net=net, activation=c.act))


@functools.lru_cache(maxsize=None)
def reference_of(c):
    from gaussian_gan_decoder_amd.density import osg_weights
    b = build(c)
    w = osg_weights(b.decoder)
    return reference(b.planes, b.pos, c.box_warp, c.axes, c.D, w.w1, w.b1, w.w2, w.b2, c.act)


# ---- the values the reference's own code produced (tests/golden/make_density_golden.py) ------------------------------------------
FIX = np.load(os.path.join(ROOT, "tests", "golden", "density_fixture.npz"))
FIX_CASES = [str(n) for n in FIX["cases"]]
FIX_LATTICES = [(int(n), float(c)) for n, c in FIX["lattices"]]


def fixture_case(name):
    """(planes [3, 32 * max(D, 1), H, W], coords, duck-typed decoder, D, axes, box_warp, activation) of a fixture case"""
    D, lr_mul, box_warp = (float(v) for v in FIX[name + ".meta"])
    D = int(D)
    gains = FIX[name + ".gains"]
    net = [SimpleNamespace(weight=torch.from_numpy(FIX["w1_raw"].astype(np.float32)), bias=torch.from_numpy(FIX[name + ".b1_raw"]),
                           weight_gain=gains[0], bias_gain=gains[1]), None,
           SimpleNamespace(weight=torch.from_numpy(FIX["w2_raw"].astype(np.float32)), bias=torch.from_numpy(FIX[name + ".b2_raw"]),
                           weight_gain=gains[2], bias_gain=gains[3])]
    teacher, act = str(FIX[name + ".teacher"]), str(FIX[name + ".activation"])
    # EG3D's OSGDecoder has no activation attribute: osg_weights must default to the sigmoid
    dec = SimpleNamespace(net=net) if teacher == "eg3d" else SimpleNamespace(net=net, activation=act)
    axes = "eg3d" if teacher == "eg3d" else "panohead"
    assert np.array_equal(FIX[name + ".plane_axes"], PLANE_AXES[axes].numpy())
    assert abs(gains[0] - lr_mul / math.sqrt(32)) < 1e-12 and gains[1] == lr_mul
    planes = torch.from_numpy(FIX[f"planes_d{D}"].astype(np.float32))
    return SimpleNamespace(planes=planes, coords=torch.from_numpy(FIX[name + ".coords"]), decoder=dec, D=D, axes=axes,
                           box_warp=box_warp, act=act, sigma=torch.from_numpy(FIX[name + ".sigma"]),
                           rgb=torch.from_numpy(FIX[name + ".rgb"]))
