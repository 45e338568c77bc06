"""Reference for the depth-distortion map (ggd_forward_distortion / ggd_backward_distortion), numpy, no GPU.

Per pixel the reference walks a frame's decoded lists (the NATIVE run's on the GPU, the oracle's own here on the CPU), bounded by
that frame's n_contrib, over the fp32 oracle's per-Gaussian records (xy, conic_opacity, depths), re-evaluates the skip rules
(power > 0, alpha < 1/255) in float64 as _features_ref.blend_f64 does, and forms with w = alpha T

    D = sum_i sum_j w_i w_j |z_i - z_j|                                       (the literal double sum, with abs())

The gradients are the closed forms, in LIST order (at equal depths the derivative of |z_i - z_j| is taken as if the later record
lay behind, which is what a sorted walk means and the limit the kernels evaluate):

    dD/dz_k = 2 w_k (A_{k-1} - (A - A_k))              dD/dw_k = 2 u_k,  u_k = sum_j w_j |z_k - z_j|
    dL/dalpha_k = T_k c_k - sum_{j>k} w_j c_j / (1 - alpha_k),  c_k = 2 g u_k          (a one-channel blend of the values c_k)

taken on to the per-record sums of the backward's accumulator (mean2D in the units of dL_dmeans2D, conic, opacity, z) exactly as
oracle/ggd_oracle.c::ggo_render_backward_ref64 takes the colour's, and from there through the oracle's float64 per-Gaussian
backward with its running error analysis (ggo_preprocess_backward_err) to dL_dmeans3D, dL_dcov3D, dL_dscales, dL_drots.

Budgets: beside every sum the same sum with every term in absolute value -- for D the terms of the recurrence the kernels
evaluate, D = 2 sum_k w_k (z_k A_{k-1} - B_{k-1}): 2 sum_k w_k (|z_k| A_{k-1} + sum_{j<k} w_j |z_j|).  The bar is
|gpu - ref64| <= ATOL + K * 2^-24 * budget.

In the gradients the sums in front of a record enter as the backward has them: it walks back to front, so A_{k-1} is the
pixel's total less what lies behind less the record's own, A - (A - A_k) - w_k, three terms of magnitude A + (A - A_k) + w_k
(B_{k-1} likewise, in |z|) -- that magnitude, not A_{k-1} itself, is what an fp32 evaluation of the difference can be held to.
(A pixel with ONE contributor shows it: A_0 = 0 exactly when summed from the front, w_1 - w_1 of two differently rounded w_1 when
formed from the total; the budget of the first form is 0 there.)

K comes from this module's own float32 twin, never from a kernel: `evaluate(..., dtype=np.float32)` runs the same expressions
(prefix recurrences, exp, transmittance product, per-record sums) in numpy float32 on the float64 run's contributor set, and
`fp32_share` is the largest |twin - ref64| / (2^-24 budget) over every element of D and of the four accumulator sums.  Over the
scenes of tests/test_distortion_gpu.py (SCENES below; tests/test_distortion_host.py recomputes it) the largest share is
MEASURED_SHARE; K is four times that, rounded up, for a different but legitimate summation order on the device."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from _util import adversarial_inputs, scene_inputs

EPS32 = 2.0 ** -24
ATOL = 1e-5
MEASURED_SHARE = 141.0   # largest share of the budget the float32 twin uses over SCENES: the z sums of "adversarial", whose needles and
#                         image-filling splats make `power` a cancelling sum (D 83.1 there; "shell" 7.0 in z, 2.6 in D; the hand-built
#                         scenes below 1); test_distortion_host.py recomputes and prints each
K = 564.0              # = 4 * MEASURED_SHARE, rounded up

SCENES = {
    # 40 x 24: 3 x 2 tiles, the right column 8 pixels wide, the bottom row 8 high (partial tiles AND quarters); the dense shell puts
    # more than two 64-entry gather rounds into a tile's list
    "shell": lambda: scene_inputs(P=300, size=40, width=40, height=24, kind="shell", lsm=-3.2, seed=21),
    "adversarial": adversarial_inputs,
    "hand": lambda: hand_scene(),
    "opaque-front": lambda: opaque_front_scene(),
    "two-layers": lambda: two_layer_scene(),
}


def _placed(P, size, seed, place):
    """scene_inputs' camera (looking at the origin) with Gaussians the caller places: place(right, up, fwd, pixel) ->
    (means3D, scales, opacities) as lists per Gaussian, in world units; identity rotations.  pixel: the world size of a pixel at
    the origin's depth."""
    import math
    import torch
    d = scene_inputs(P=P, size=size, seed=seed)
    view = d["viewmatrix"]                      # row-vector convention: p_view = [p, 1] @ view
    right, up, fwd = view[:3, 0], view[:3, 1], view[:3, 2]
    dist = float(torch.inverse(view)[3, :3].norm())
    pixel = 2.0 * d["tanfovx"] * dist / size
    means, scales, ops = place(right, up, fwd, pixel)
    assert len(means) == P
    q = torch.zeros(P, 4); q[:, 0] = 1.0
    return dict(d, means3D=torch.stack(means).float().contiguous(), opacities=torch.tensor(ops).float().reshape(P, 1).contiguous(),
                scales=torch.tensor(scales).float().reshape(P, 1).repeat(1, 3).contiguous(), rotations=q.contiguous())


def hand_scene():
    """32 x 32.  Gaussians 0 and 1: exact duplicates in position (equal depth bits), different opacity, in front of Gaussian 2 on
    the same ray: the centre pixels see all three and the tie contributes 0.  Gaussian 3: alone, 10 pixels to the right: pixels
    with ONE contributor.  The corners see nothing."""
    def place(right, up, fwd, px):
        o = 0.0 * fwd
        return [o, o, 0.25 * fwd, 10.0 * px * right], [2.0 * px, 2.0 * px, 2.0 * px, 1.2 * px], [0.5, 0.3, 0.7, 0.6]
    return _placed(4, 32, 31, place)


def opaque_front_scene(n_front=6, n_back=30):
    """16 x 16.  n_front image-filling layers of alpha ~ 0.85 (scale 3: G >= 0.995 over the image) in front of n_back small
    Gaussians: 0.15^4 = 5.1e-4 and the fifth layer would leave (0.150 .. 0.154)^5 <= 8.7e-5 < 1e-4, so every pixel's n_contrib is
    4 while its list goes on for n_front + n_back - 4 entries -- and no pixel is near the stop."""
    import torch
    gen = torch.Generator().manual_seed(33)
    def place(right, up, fwd, px):
        means = [-(0.3 - 0.05 * i) * fwd for i in range(n_front)]
        back = torch.rand(n_back, 3, generator=gen)
        means += [(0.1 + 0.2 * float(b[2])) * fwd + 12.0 * px * ((float(b[0]) - 0.5) * right + (float(b[1]) - 0.5) * up) for b in back]
        return means, [3.0] * n_front + [2.0 * px] * n_back, [0.85] * n_front + [0.5] * n_back
    return _placed(n_front + n_back, 16, 32, place)


def two_layer_scene(a1=0.6, a2=0.5):
    """16 x 16.  Two image-filling splats (scale 100: G = 1 - 4e-6 at the image's edge) of opacity a1 in front and a2 behind:
    every pixel has alpha_1 = a1 G_1, alpha_2 = a2 G_2 and D = 2 alpha_1 alpha_2 (1 - alpha_1) (z_2 - z_1)."""
    def place(right, up, fwd, px):
        return [-0.15 * fwd, 0.15 * fwd], [100.0, 100.0], [a1, a2]
    return _placed(2, 16, 34, place)


@functools.lru_cache(maxsize=None)
def scene(name):
    """cached: do not modify"""
    return SCENES[name]()


def _excl(v):
    """exclusive running sum, sequential in v's dtype"""
    c = np.cumsum(v, dtype=v.dtype)
    return np.concatenate([np.zeros(1, v.dtype), c[:-1]]), c


def evaluate(o, lists=None, g=None, dtype=np.float64):
    """o: an fp32 oracle forward (its xy, conic_opacity, depths are the records); lists: a dict with point_list, ranges and
    n_contrib (default: o's own); g: dL/dD [H, W] or None (forward only).  Returns a dict: D, D_literal (float64 only), D_budget
    and count (the pixel's contributors) [H, W]; with g the accumulator sums mean2D [P, 2], conic [P, 3], opacity [P], z [P] and
    S_<name>, their budgets; fragile [P], the (pixel, Gaussian) pairs within 1e-6 of the alpha floor.  The skip rules are always evaluated in float64; `dtype` is the arithmetic of the values."""
    lists = o if lists is None else lists
    W, H, P = o["W"], o["H"], o["P"]
    gx = (W + 15) // 16
    dt = np.dtype(dtype).type
    xy64, co64 = o["xy"].astype(np.float64), o["conic_opacity"].astype(np.float64)
    xy, co, zs = xy64.astype(dt), co64.astype(dt), o["depths"].astype(np.float32).astype(dt)
    plist, ranges, ncon = lists["point_list"], lists["ranges"], lists["n_contrib"]
    out = dict(D=np.zeros((H, W), dt), D_literal=np.zeros((H, W)), D_budget=np.zeros((H, W)),
               count=np.zeros((H, W), np.int64), fragile=np.zeros(P, np.uint32))
    names = dict(mean2D=(P, 2), conic=(P, 3), opacity=(P,), z=(P,))
    if g is not None:
        g = np.asarray(g, np.float32).reshape(H, W)
        for k, sh in names.items():
            out[k], out["S_" + k] = np.zeros(sh, dt), np.zeros(sh)
    half, cap = dt(0.5), dt(np.float32(0.99))
    sx, sy = dt(0.5 * W), dt(0.5 * H)
    for py in range(H):
        for px in range(W):
            lo = int(ranges[(py // 16) * gx + px // 16][0])
            ids = plist[lo:lo + int(ncon[py, px])].astype(np.int64)
            if ids.size == 0:
                continue
            # decisions, float64
            dx, dy = xy64[ids, 0] - px, xy64[ids, 1] - py
            c = co64[ids]
            pw = -0.5 * (c[:, 0] * dx * dx + c[:, 2] * dy * dy) - c[:, 1] * dx * dy
            al = np.minimum(float(np.float32(0.99)), c[:, 3] * np.exp(np.minimum(pw, 0.0)))
            np.add.at(out["fragile"], ids[(pw <= 0.0) & (np.abs(al * 255.0 - 1.0) <= 1e-6)], 1)
            keep = (pw <= 0.0) & (al >= 1.0 / 255.0)
            ids = ids[keep]
            out["count"][py, px] = ids.size
            if ids.size == 0:
                continue
            # values, in dt
            dx, dy = xy[ids, 0] - dt(px), xy[ids, 1] - dt(py)
            cA, cB, cC, op = co[ids, 0], co[ids, 1], co[ids, 2], co[ids, 3]
            z = zs[ids]
            pw = -half * (cA * dx * dx + cC * dy * dy) - cB * dx * dy
            G = np.exp(pw)
            alpha = np.minimum(cap, op * G)
            om = dt(1.0) - alpha
            T = np.concatenate([np.ones(1, dt), np.cumprod(om, dtype=dt)[:-1]])
            w = alpha * T
            Apre, Ainc = _excl(w)
            Bpre, Binc = _excl(w * z)
            Bpre_abs, Binc_abs = _excl(w * np.abs(z))
            out["D"][py, px] = dt(2.0) * np.cumsum(w * (z * Apre - Bpre), dtype=dt)[-1]
            w64, z64 = w.astype(np.float64), z.astype(np.float64)
            out["D_budget"][py, px] = 2.0 * float((w64 * (np.abs(z64) * Apre + Bpre_abs)).sum())
            if dt is np.float64:
                out["D_literal"][py, px] = float(w64 @ np.abs(z64[:, None] - z64[None, :]) @ w64)
            if g is None or g[py, px] == 0.0:
                continue
            gp = dt(g[py, px])
            SA, SB, SB_abs = Ainc[-1] - Ainc, Binc[-1] - Binc, Binc_abs[-1] - Binc_abs
            # magnitudes of the sums in front as the back-to-front walk forms them: total - behind - own
            Amag = (Ainc[-1] + SA + w).astype(np.float64)
            Bmag = (Binc_abs[-1] + SB_abs + w * np.abs(z)).astype(np.float64)
            dDdz = dt(2.0) * w * (Apre - SA)
            u = (z * Apre - Bpre) + (SB - z * SA)
            cval = dt(2.0) * gp * u
            cmag = 2.0 * abs(float(gp)) * (np.abs(z64) * (Amag + SA) + Bmag + SB_abs)
            wc, wcm = w * cval, w64 * cmag
            behind = np.cumsum(wc[::-1], dtype=dt)[::-1] - wc            # sum_{j>k} w_j c_j
            behind_m = np.cumsum(wcm[::-1])[::-1] - wcm
            dLda = T * cval - behind / om
            mag = T * cmag + behind_m / om
            dLdG, mG = op * dLda, np.abs(op) * mag
            gdx, gdy = G * dx, G * dy
            add = lambda name, col, v, m: (np.add.at(out[name], (ids, col) if col is not None else ids, v),
                                           np.add.at(out["S_" + name], (ids, col) if col is not None else ids,
                                                     np.abs(np.asarray(m, np.float64))))
            add("mean2D", 0, dLdG * (-gdx * cA - gdy * cB) * sx, mG * (np.abs(gdx * cA) + np.abs(gdy * cB)) * sx)
            add("mean2D", 1, dLdG * (-gdy * cC - gdx * cB) * sy, mG * (np.abs(gdy * cC) + np.abs(gdx * cB)) * sy)
            add("conic", 0, -half * gdx * dx * dLdG, half * gdx * dx * mG)
            add("conic", 1, -half * gdx * dy * dLdG, half * gdx * dy * mG)
            add("conic", 2, -half * gdy * dy * dLdG, half * gdy * dy * mG)
            add("opacity", None, G * dLda, G * mag)
            add("z", None, gp * dDdz, 2.0 * abs(float(gp)) * w64 * (Amag + SA))
    return out


def fp32_share(o, g, lists=None):
    """{quantity: largest |float32 twin - float64| / (2^-24 budget)} of one frame, over the elements with a budget"""
    r64 = evaluate(o, lists, g, np.float64)
    r32 = evaluate(o, lists, g, np.float32)
    share = {}
    for name, bud in (("D", "D_budget"), ("mean2D", "S_mean2D"), ("conic", "S_conic"), ("opacity", "S_opacity"), ("z", "S_z")):
        b = r64[bud]
        err = np.abs(r32[name].astype(np.float64) - r64[name])
        assert (err[b == 0.0] == 0.0).all(), name
        share[name] = float((err[b > 0.0] / (EPS32 * b[b > 0.0])).max(initial=0.0))
    return share


def closed_form_two_layers(a1, a2, z1, z2):
    """two constant-alpha layers at depths z1 < z2: D = 2 a1 a2 (1 - a1) (z2 - z1)"""
    return 2.0 * a1 * a2 * (1.0 - a1) * (z2 - z1)


def backward_ref(d, o, n, g_dist):
    """fp64 reference and budget of the distortion map's share of ggd_backward_distortion for one forward (o = fp32 oracle forward
    of d, n = the decoded native forward), in the form of _util.backward_reference: (ref, budget, fragile), the budget in units of
    2^-24 for the bar ATOL + K eps32 budget, and the evaluate() dict as a fourth.  For an anti-aliased run d and o carry the
    effective opacities (tests/test_antialiasing_gpu.py::_gpu_opacity_inputs) and _antialias_ref.compose_backward goes on from
    here.  dL_dcolors / dL_dsh are zeros (the map does not depend on the colours)."""
    from oracle import ggd_oracle as O
    L = O.lib()
    r = evaluate(o, n, g_dist, np.float64)
    P, M, W, H = o["P"], o["M"], o["W"], o["H"]
    prm = o["prm"]
    er = lambda a, e=None: None if a is None else np.ascontiguousarray(
        np.stack([np.asarray(a, np.float64), np.zeros_like(a, np.float64) if e is None else e], axis=-1))
    prm64 = O._Params(P, M, o["sh_degree"], W, H, 0, float(prm.tanfovx), float(prm.tanfovy), float(prm.scale_modifier))
    have_cp, have_c3 = o["colors_precomp"] is not None, o["cov3D_precomp"] is not None
    scales, rots = er(o["scales"]), er(o["rotations"])
    if have_c3:
        cov = er(o["cov3D_precomp"])
    else:
        cov = np.zeros((P, 6, 2), np.float64)
        L.ggo_cov3d_all_err(P, O._p(scales), C.c_double(float(prm.scale_modifier)), O._p(rots), O._p(cov))
    ze = lambda *sh: np.zeros(sh + (2,), np.float64)
    d_means3D, d_cov3D, d_scales, d_rots = ze(P, 3), ze(P, 6), ze(P, 3), ze(P, 4)
    d_sh = ze(P, max(M, 1), 3) if M > 0 else None
    zc = np.zeros((P, 3))
    L.ggo_preprocess_backward_err(C.byref(prm64), O._p(er(o["viewmatrix"])), O._p(er(o["projmatrix"])), O._p(er(o["campos"])),
                                  O._p(er(o["means3D"])), O._p(er(o["shs"])), int(have_cp), O._p(scales), O._p(rots), O._p(cov),
                                  int(have_c3), O._p(o["radii"]), O._p(o["clamped"]), O._p(er(r["mean2D"], r["S_mean2D"])),
                                  O._p(er(r["conic"], r["S_conic"])), O._p(er(zc, zc)), O._p(d_means3D), O._p(d_cov3D),
                                  O._p(d_sh), O._p(d_scales), O._p(d_rots))
    vis = o["radii"] > 0
    outs = dict(dL_dmeans3D=d_means3D, dL_dcov3D=d_cov3D, dL_dsh=d_sh, dL_dscales=d_scales, dL_drots=d_rots)
    ref = {k: (None if v is None else np.ascontiguousarray(v[..., 0])) for k, v in outs.items()}
    bud = {k: (None if v is None else np.ascontiguousarray(v[..., 1])) for k, v in outs.items()}
    m2, b2 = np.zeros((P, 3)), np.zeros((P, 3))
    m2[:, :2], b2[:, :2] = r["mean2D"] * vis[:, None], r["S_mean2D"] * vis[:, None]
    ref.update(dL_dmeans2D=m2, dL_dconic=r["conic"], dL_dopacity=r["opacity"] * vis, dL_dcolors=zc)
    bud.update(dL_dmeans2D=b2, dL_dconic=r["S_conic"], dL_dopacity=r["S_opacity"] * vis, dL_dcolors=zc.copy())
    # the z term reaches the means as the depth map's does (_depth_alpha_ref): dL/dz times row 2 of the view matrix
    v = np.asarray(o["viewmatrix"], np.float64).reshape(-1)
    col = np.array([v[2], v[6], v[10]])[None, :]
    dz, Sz = (r["z"] * vis)[:, None], (r["S_z"] * vis)[:, None]
    ref["dL_dmeans3D"] = ref["dL_dmeans3D"] + dz * col
    bud["dL_dmeans3D"] = bud["dL_dmeans3D"] + (Sz + 2.0 * np.abs(dz)) * np.abs(col) + 2.0 * np.abs(ref["dL_dmeans3D"])
    return ref, bud, r["fragile"], r


__all__ = ["ATOL", "EPS32", "K", "MEASURED_SHARE", "SCENES", "scene", "evaluate", "fp32_share", "closed_form_two_layers",
           "backward_ref", "hand_scene", "opaque_front_scene", "two_layer_scene"]
