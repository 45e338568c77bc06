"""float64 restatement (numpy) of the per-ray part of the teacher renderer (gaussian_gan_decoder_amd/teacher.py,
csrc/ggd_teacher.hip), stage by stage, the fixture loader and the tolerances of tests/test_teacher_render_host.py and
tests/test_teacher_render_gpu.py.

Stages (each takes fp32 arrays and continues in float64):
    coarse_depths    fp32, exact: fl(t[k] + fl(u * delta)) and fl(o + fl(depth * d)) with numpy's float32 -- bit-equality stage
    march            midpoints, softplus(sigma_mid - 1), alpha = 1 - exp(-sigma_mid * width), w = alpha * exclusive cumprod
    importance       the pools, + 0.01, both ends dropped, + 1e-5, normalised, cumulative sum, searchsorted(right) and the
                     linear interpolation: (coarse depths, coarse sigma, u_fine) -> fine depths
    composite        the union ordered by depth (ties by index), march, the three sums, NaN -> inf, the clamp to the depth range
                     of the call: (depths, sigma, rgb of both sets) -> features, weights, depth
    end_to_end       the stages chained around the float64 field of tests/_density_ref.py; the coordinates (and with them the crop)
                     are formed in fp32 from the fp32-rounded depth, as every implementation forms them

Tolerances.  For each stage, the worst deviation over the fixture (tests/golden/teacher_render_fixture.npz, values the reference's
own code produced) of the REFERENCE'S OWN fp32 result from this restatement fed the same fp32 inputs is recorded below as
*_MEASURED (absolute, per output; test_teacher_render_host.py measures it again, prints it and asserts that the constant is what
it measures).  The accepted tolerance is twice that: two fp32 evaluations with different summation orders can each stand that
far from the float64 value, on opposite sides.  Never the code under test.
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

import _density_ref as D

ROOT = D.ROOT
FIX = dict(np.load(os.path.join(ROOT, "tests", "golden", "teacher_render_fixture.npz")))
FIX.update(np.load(os.path.join(ROOT, "tests", "golden", "teacher_render_fixture_rgb.npz")))   # the large cases' per-sample rgb
CASES = [str(n) for n in FIX["cases"]]
NEAR_CROP = 1e-5                 # a fine sample this close to the crop limit may flip with an ulp of depth: its ray is left out

# worst |reference fp32 - float64 restatement| over the fixture (absolute)
IMPORTANCE_MEASURED = 3.89e-7       # fine depths
COMPOSITE_MEASURED = SimpleNamespace(features=8.25e-7, weights=1.88e-7, depth=6.36e-7)
END_TO_END_MEASURED = SimpleNamespace(features=1.339e-6, weights=2.842e-7, depth=6.438e-7)
TOL_IMPORTANCE = 2.0 * IMPORTANCE_MEASURED
TOL_COMPOSITE = SimpleNamespace(**{k: 2.0 * v for k, v in vars(COMPOSITE_MEASURED).items()})
TOL_END_TO_END = SimpleNamespace(**{k: 2.0 * v for k, v in vars(END_TO_END_MEASURED).items()})


def case(name):
    """the inputs, the reference's intermediate values and its outputs of one fixture case (numpy float32 / torch for the planes)"""
    Dd, lr_mul, box_warp, crop, white_back, Nc, Ni, res = (float(v) for v in FIX[name + ".meta"])
    Dd, Nc, Ni = int(Dd), int(Nc), int(Ni)
    gains = FIX[name + ".gains"]
    net = [SimpleNamespace(weight=torch.from_numpy(FIX["w1_raw"].astype(np.float32)), bias=torch.from_numpy(FIX[name + ".b1_raw"]),
                           weight_gain=gains[0], bias_gain=gains[1]), None,
           SimpleNamespace(weight=torch.from_numpy(FIX["w2_raw"].astype(np.float32)), bias=torch.from_numpy(FIX[name + ".b2_raw"]),
                           weight_gain=gains[2], bias_gain=gains[3])]
    teacher, act = str(FIX[name + ".teacher"]), str(FIX[name + ".activation"])
    dec = SimpleNamespace(net=net) if teacher == "eg3d" else SimpleNamespace(net=net, activation=act)
    f = {k: FIX[f"{name}.{k}"] for k in ("origins", "dirs", "u_coarse", "u_fine", "depths_coarse", "depths_fine", "sigma", "rgb",
                                         "features", "depth", "weights")}
    return SimpleNamespace(name=name, planes=torch.from_numpy(FIX[f"planes_d{Dd}"].astype(np.float32)), decoder=dec, D=Dd,
                           axes="eg3d" if teacher == "eg3d" else "panohead", act=act, box_warp=box_warp,
                           scaled=teacher == "eg3d", crop=None if crop < 0 else crop, white_back=bool(white_back), Nc=Nc, Ni=Ni, resolution=int(res),
                           M=f["origins"].shape[0], **f)


def as_stored(c, features):
    """the features as the case's reference returned them: EG3D's marcher scales them to (-1, 1) itself, in fp32"""
    return features * 2 - 1 if c.scaled else features


def render_kwargs(c):
    return dict(ray_start=2.25, ray_end=3.3, depth_resolution=c.Nc, depth_resolution_importance=c.Ni, box_warp=c.box_warp,
                plane_axes=c.axes, triplane_depth=c.D or None, triplane_crop=c.crop, white_back=c.white_back)


def crop_limit(c):
    return None if c.crop is None else np.float32(c.box_warp / 2 - c.crop)


# ---- the stages ----------------------------------------------------------------------------------------------------------------
def coordinates(origins, dirs, depths):
    """fl(o + fl(depth * d)) in fp32: origins, dirs [M, 3], depths [M, S] -> [M, S, 3]"""
    o, d, t = origins.astype(np.float32), dirs.astype(np.float32), depths.astype(np.float32)
    return o[:, None, :] + t[:, :, None] * d[:, None, :]


def coarse_depths(table, delta, u):
    """fl(t[k] + fl(u * delta)) in fp32: table [Nc] (torch.linspace's values), delta the double, u [M, Nc]"""
    return table.astype(np.float32)[None, :] + u.astype(np.float32) * np.float32(delta)


def cropped(sigma, coords, lim):
    if lim is None:
        return sigma
    inside = (np.abs(coords[..., 0]) <= lim) & (np.abs(coords[..., 2]) <= lim)
    return np.where(inside, sigma, sigma.dtype.type(-1e3))


def softplus(x):
    return np.where(x > 30.0, x, np.log1p(np.exp(np.minimum(x, 30.0))))


def march(depths, sigma):
    """depths, sigma [M, S] (ordered) -> w [M, S - 1], depth midpoints [M, S - 1], all float64"""
    t, s = depths.astype(np.float64), sigma.astype(np.float64)
    width = t[:, 1:] - t[:, :-1]
    alpha = 1.0 - np.exp(-softplus(0.5 * (s[:, :-1] + s[:, 1:]) - 1.0) * width)
    through = np.cumprod(np.concatenate([np.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10], 1), 1)[:, :-1]
    return alpha * through, 0.5 * (t[:, :-1] + t[:, 1:])


def importance(depths, sigma, u, eps=1e-5):
    """coarse depths [M, Nc], coarse sigma after the crop [M, Nc], u [M, Ni] -> fine depths [M, Ni] (float64)"""
    w, bins = march(depths, sigma)
    M = w.shape[0]
    ninf = np.full((M, 1), -np.inf)
    padded = np.concatenate([ninf, w, ninf], 1)
    pooled = np.maximum(padded[:, :-1], padded[:, 1:])                # max_pool1d(2, 1, padding 1): Nc values
    w = 0.5 * (pooled[:, :-1] + pooled[:, 1:]) + 0.01                 # avg_pool1d(2, 1): Nc - 1 values
    w = w[:, 1:-1] + eps
    n = w.shape[1]
    cdf = np.concatenate([np.zeros((M, 1)), np.cumsum(w / w.sum(1, keepdims=True), 1)], 1)
    u = u.astype(np.float64)
    out = np.empty_like(u)
    for r in range(M):
        inds = np.searchsorted(cdf[r], u[r], side="right")
        below, above = np.maximum(inds - 1, 0), np.minimum(inds, n)
        denom = cdf[r, above] - cdf[r, below]
        denom = np.where(denom < eps, 1.0, denom)
        out[r] = bins[r, below] + (u[r] - cdf[r, below]) / denom * (bins[r, above] - bins[r, below])
    return out


def composite(depths, sigma, rgb, white_back, scaled=False):
    """depths, sigma [M, S], rgb [M, S, 32] of the union (coarse first, then fine; any order) -> SimpleNamespace(features [M, 32],
    weights [M], depth [M], lo, hi) in float64; lo / hi: the clamp bounds (exact: the minimum and maximum of the fp32 depths).
    scaled: EG3D's marcher ends with features * 2 - 1 (eg3d ray_marcher.py:55), which PanoHead moved into synthesis and
    TeacherRender.images applies for both."""
    order = np.argsort(depths, 1, kind="stable")
    t, s = np.take_along_axis(depths, order, 1), np.take_along_axis(sigma, order, 1)
    c = np.take_along_axis(rgb.astype(np.float64), order[:, :, None], 1)
    w, t_mid = march(t, s)
    total = w.sum(1)
    features = (w[:, :, None] * (0.5 * (c[:, :-1] + c[:, 1:]))).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        depth = (w * t_mid).sum(1) / total
    depth = np.where(np.isnan(depth), np.inf, depth)
    lo, hi = float(depths.min()), float(depths.max())
    if white_back:
        features = features + 1.0 - total[:, None]
    if scaled:
        features = features * 2.0 - 1.0
    return SimpleNamespace(features=features, weights=total, depth=np.clip(depth, lo, hi), lo=lo, hi=hi)


def field(c, coords):
    """the float64 field of tests/_density_ref.py at fp32 coordinates [M, S, 3] -> sigma [M, S], rgb [M, S, 32] (before the crop)"""
    from gaussian_gan_decoder_amd.density import osg_weights
    w = osg_weights(c.decoder)
    ref = D.reference(c.planes, torch.from_numpy(np.ascontiguousarray(coords.reshape(-1, 3))), c.box_warp, c.axes, c.D, w.w1, w.b1,
                      w.w2, w.b2, c.act)
    return ref.sigma.numpy().reshape(coords.shape[:2]), ref.rgb.numpy().reshape(coords.shape[:2] + (32,))


def end_to_end(c, table, delta):
    """the whole chain in float64 from the case's rays and noise"""
    lim = crop_limit(c)
    t_c = coarse_depths(table, delta, c.u_coarse)
    x_c = coordinates(c.origins, c.dirs, t_c)
    s_c, rgb_c = field(c, x_c)
    s_c = cropped(s_c, x_c, lim)
    if c.Ni == 0:
        return composite(t_c, s_c, rgb_c, c.white_back, c.scaled), None
    t_f = importance(t_c, s_c, c.u_fine)
    x_f = coordinates(c.origins, c.dirs, t_f.astype(np.float32))
    s_f, rgb_f = field(c, x_f)
    s_f = cropped(s_f, x_f, lim)
    return composite(np.concatenate([t_c.astype(np.float64), t_f], 1), np.concatenate([s_c, s_f], 1),
                     np.concatenate([rgb_c, rgb_f], 1), c.white_back, c.scaled), t_f


def near_crop_rays(c, coords_fine):
    """rays with a fine sample within NEAR_CROP of the crop limit in |x| or |z| (bool, one per row of coords_fine [M, Ni, 3])"""
    lim = crop_limit(c)
    if lim is None or coords_fine.shape[1] == 0:
        return np.zeros(coords_fine.shape[0], bool)
    gap = np.abs(np.abs(np.asarray(coords_fine, np.float64)[..., [0, 2]]) - float(lim))
    return (gap < NEAR_CROP).any(axis=(1, 2))


def worst(got, ref, rows=None):
    """max |got - ref| (over the kept rows); inf where one side is non-finite and the other differs"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    if got.size == 0:
        return 0.0
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    err = np.where(same, 0.0, np.abs(got - ref))
    return float(np.where(np.isfinite(err), err, np.inf).max())
