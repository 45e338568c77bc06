"""Reference for the camera's gradients (ggd_backward_camera): numpy, float64, and its float32 twin.

Inputs: the per-Gaussian sums of the blend backward (what the library keeps in its accumulator records) -- dL_dconic [P, 3],
dL_dmeans2D [P, 2+], the colour gradients [P, 3] and the depth slot [P] (None = 0), as `oracle.ggd_oracle.backward_ref64` returns
them in float64 -- and the scene (an oracle forward dict: inputs, radii, clamped, cov3D).  Outputs: the 35 values (dL_dviewmatrix
[16], dL_dprojmatrix [16], dL_dcampos [3], flat entry k = derivative in flat entry k of the input, m[4c + r] = row r, column c) and,
beside each, the same sum with every term in absolute value -- the budget.

Every value is linear in the nine sums.  `terms` evaluates one Gaussian's 35 contributions for given sums; the reference takes it
on each of the nine slots alone (the others zero), which gives the terms |L_ij a_ij| of the budget and, with the accumulators' own
allowance KAPPA 2^-24 budget_ij in place of a_ij, what that allowance carries into the sums (`carried`).

The bar of the GPU tests:  |gpu - ref64| <= 1e-5 + carried + K 2^-24 budget.  K follows the project's rule: four times, rounded up,
the largest share of the budget that this module's own float32 twin (the same expressions in numpy float32, summed in index order)
uses over the test scenes.  It is never taken from a kernel; tests/test_camera_grad_host.py recomputes and prints the share.
"""
from __future__ import annotations

import math

import numpy as np

from _util import ATOL, EPS32, KAPPA, adversarial_inputs, scene_inputs

MEASURED_SHARE = 14.0         # float32 twin, largest |twin - ref64| / (2^-24 budget) over SCENES (recomputed by the host test)
K = int(math.ceil(4 * MEASURED_SHARE))

SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435)

# flat entries no kernel reads: the bottom row of the view matrix, row 2 of the projection matrix
UNREAD = [4 * c + 3 for c in range(4)] + [16 + 4 * c + 2 for c in range(4)]


def _sh_dir_grad(deg, sh, x, y, z):
    """d colour [P, 3] / d (x, y, z): three [P, 3] arrays; sh [P, M, 3]."""
    k = lambda i: sh[:, i, :]
    X, Y, Z = x[:, None], y[:, None], z[:, None]
    dt = sh.dtype.type
    dx = -dt(SH_C1) * k(3); dy = -dt(SH_C1) * k(1); dz = dt(SH_C1) * k(2)
    if deg > 1:
        c = [dt(v) for v in SH_C2]
        dx = dx + (c[0] * Y * k(4) + c[2] * dt(2) * -X * k(6) + c[3] * Z * k(7) + c[4] * dt(2) * X * k(8))
        dy = dy + (c[0] * X * k(4) + c[1] * Z * k(5) + c[2] * dt(2) * -Y * k(6) + c[4] * dt(2) * -Y * k(8))
        dz = dz + (c[1] * Y * k(5) + c[2] * dt(4) * Z * k(6) + c[3] * X * k(7))
    if deg > 2:
        c = [dt(v) for v in SH_C3]
        xx, yy, zz, xy, yz, xz = X * X, Y * Y, Z * Z, X * Y, Y * Z, X * Z
        dx = dx + (c[0] * k(9) * dt(6) * xy + c[1] * k(10) * yz + c[2] * k(11) * dt(-2) * xy + c[3] * k(12) * dt(-6) * xz +
                   c[4] * k(13) * (dt(4) * zz - dt(3) * xx - yy) + c[5] * k(14) * dt(2) * xz + c[6] * k(15) * dt(3) * (xx - yy))
        dy = dy + (c[0] * k(9) * dt(3) * (xx - yy) + c[1] * k(10) * xz + c[2] * k(11) * (dt(4) * zz - xx - dt(3) * yy) +
                   c[3] * k(12) * dt(-6) * yz + c[4] * k(13) * dt(-2) * xy + c[5] * k(14) * dt(-2) * yz +
                   c[6] * k(15) * dt(-6) * xy)
        dz = dz + (c[1] * k(10) * xy + c[2] * k(11) * dt(8) * yz + c[3] * k(12) * dt(3) * (dt(2) * zz - xx - yy) +
                   c[4] * k(13) * dt(8) * xz + c[5] * k(14) * (xx - yy))
    return dx, dy, dz


def terms(o, conic, mean2d, color, gz, gop=None, dtype=np.float64, aa_opacity=None):
    """[P, 35]: every Gaussian's contribution to the 35 values (zeros for radii <= 0), evaluated in `dtype`; and the number of
    visible Gaussians whose view-space x or y the forward clamped.
    aa_opacity (antialiasing): the opacities o [P] as given to the forward, whose blend saw o h; gop is then dL/d(o h), the blend's
    opacity sum, and the h chain of the per-Gaussian backward joins dL/d(a, b, c)."""
    dt = np.dtype(dtype).type
    f = lambda a: np.asarray(a, np.float64).astype(dtype)
    P = o["P"]
    V, PV, cam = f(o["viewmatrix"]).reshape(16), f(o["projmatrix"]).reshape(16), f(o["campos"]).reshape(3)
    p = np.concatenate([f(o["means3D"]).reshape(P, 3), np.ones((P, 1), dtype)], 1)
    c6 = f(o["cov3D"]).reshape(P, 6)
    vis = np.asarray(o["radii"]) > 0
    gA, gB, gC = (f(conic)[:, i] for i in range(3))
    g0, g1 = f(mean2d)[:, 0], f(mean2d)[:, 1]
    gcol = f(color).reshape(P, 3)
    gz = np.zeros(P, dtype) if gz is None else f(gz)
    tanx, tany = dt(o["prm"].tanfovx), dt(o["prm"].tanfovy)
    fx, fy = dt(o["W"]) / (dt(2) * tanx), dt(o["H"]) / (dt(2) * tany)
    out = np.zeros((P, 35), dtype)
    with np.errstate(all="ignore"):
        t = [V[r] * p[:, 0] + V[4 + r] * p[:, 1] + V[8 + r] * p[:, 2] + V[12 + r] for r in range(3)]
        limx, limy = dt(1.3) * tanx, dt(1.3) * tany
        tz = t[2]
        txtz, tytz = t[0] / tz, t[1] / tz
        clx, cly = (txtz < -limx) | (txtz > limx), (tytz < -limy) | (tytz > limy)
        tx, ty = np.clip(txtz, -limx, limx) * tz, np.clip(tytz, -limy, limy) * tz
        J00, J02 = fx / tz, -(fx * tx) / (tz * tz)
        J11, J12 = fy / tz, -(fy * ty) / (tz * tz)
        T = [[J00 * V[4 * j] + J02 * V[4 * j + 2] for j in range(3)], [J11 * V[4 * j + 1] + J12 * V[4 * j + 2] for j in range(3)]]
        S = [[c6[:, 0], c6[:, 1], c6[:, 2]], [c6[:, 1], c6[:, 3], c6[:, 4]], [c6[:, 2], c6[:, 4], c6[:, 5]]]
        U = [[T[i][0] * S[0][j] + T[i][1] * S[1][j] + T[i][2] * S[2][j] for j in range(3)] for i in range(2)]
        abc0 = U[0][0] * T[0][0] + U[0][1] * T[0][1] + U[0][2] * T[0][2]
        abc1 = U[0][0] * T[1][0] + U[0][1] * T[1][1] + U[0][2] * T[1][2]
        abc2 = U[1][0] * T[1][0] + U[1][1] * T[1][1] + U[1][2] * T[1][2]
        a, b, c = abc0 + dt(0.3), abc1, abc2 + dt(0.3)
        denom = a * c - b * b
        d2i = dt(1) / (denom * denom + dt(0.0000001))
        da = d2i * (-c * c * gA + dt(2) * b * c * gB + (denom - a * c) * gC)
        dc = d2i * (-a * a * gC + dt(2) * a * b * gB + (denom - a * c) * gA)
        db = d2i * dt(2) * (b * c * gA - (denom + dt(2) * b * b) * gB + a * b * gC)
        if aa_opacity is not None:
            w = dt(0.3)
            r = (abc0 * abc2 - abc1 * abc1) / denom
            h = np.sqrt(np.maximum(dt(2.5e-5), r))
            k = np.where(r > dt(2.5e-5), f(gop) * f(aa_opacity).reshape(P) / (dt(2) * h * denom * denom), dt(0))
            da = da + k * w * (abc2 * abc2 + w * abc2 + abc1 * abc1)
            dc = dc + k * w * (abc0 * abc0 + w * abc0 + abc1 * abc1)
            db = db + dt(-2) * k * w * abc1 * (abc0 + abc2 + w)
        dT = [[dt(2) * U[0][j] * da + U[1][j] * db for j in range(3)], [dt(2) * U[1][j] * dc + U[0][j] * db for j in range(3)]]
        dJ00 = V[0] * dT[0][0] + V[4] * dT[0][1] + V[8] * dT[0][2]
        dJ02 = V[2] * dT[0][0] + V[6] * dT[0][1] + V[10] * dT[0][2]
        dJ11 = V[1] * dT[1][0] + V[5] * dT[1][1] + V[9] * dT[1][2]
        dJ12 = V[2] * dT[1][0] + V[6] * dT[1][1] + V[10] * dT[1][2]
        iz = dt(1) / tz
        iz2, iz3 = iz * iz, iz * iz * iz
        dtx = np.where(clx, dt(0), -fx * iz2 * dJ02)
        dty = np.where(cly, dt(0), -fy * iz2 * dJ12)
        dtz = -fx * iz2 * dJ00 - fy * iz2 * dJ11 + (dt(2) * fx * tx) * iz3 * dJ02 + (dt(2) * fy * ty) * iz3 * dJ12 + gz
        for cc in range(4):
            w0 = J00 * dT[0][cc] if cc < 3 else dt(0)
            w1 = J11 * dT[1][cc] if cc < 3 else dt(0)
            w2 = J02 * dT[0][cc] + J12 * dT[1][cc] if cc < 3 else dt(0)
            out[:, 4 * cc + 0] = dtx * p[:, cc] + w0
            out[:, 4 * cc + 1] = dty * p[:, cc] + w1
            out[:, 4 * cc + 2] = dtz * p[:, cc] + w2
        h0 = PV[0] * p[:, 0] + PV[4] * p[:, 1] + PV[8] * p[:, 2] + PV[12]
        h1 = PV[1] * p[:, 0] + PV[5] * p[:, 1] + PV[9] * p[:, 2] + PV[13]
        h3 = PV[3] * p[:, 0] + PV[7] * p[:, 1] + PV[11] * p[:, 2] + PV[15]
        m_w = dt(1) / (h3 + dt(0.0000001))
        mul1, mul2 = h0 * m_w * m_w, h1 * m_w * m_w
        dh = {0: m_w * g0, 1: m_w * g1, 3: -(mul1 * g0 + mul2 * g1)}
        for cc in range(4):
            for r, v in dh.items():
                out[:, 16 + 4 * cc + r] = v * p[:, cc]
        if o["shs"] is not None and o["sh_degree"] > 0:
            sh = f(o["shs"]).reshape(P, -1, 3)
            g = np.where(np.asarray(o["clamped"]).reshape(P, 3) != 0, dt(0), gcol)
            v = p[:, :3] - cam[None, :]
            ln = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
            x, y, z = v[:, 0] / ln, v[:, 1] / ln, v[:, 2] / ln
            dx, dy, dz = _sh_dir_grad(o["sh_degree"], sh, x, y, z)
            dd = [(dx * g).sum(1), (dy * g).sum(1), (dz * g).sum(1)]
            s2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
            i32 = dt(1) / np.sqrt(s2 * s2 * s2)
            out[:, 32] = -((s2 - v[:, 0] * v[:, 0]) * dd[0] - v[:, 1] * v[:, 0] * dd[1] - v[:, 2] * v[:, 0] * dd[2]) * i32
            out[:, 33] = -(-v[:, 0] * v[:, 1] * dd[0] + (s2 - v[:, 1] * v[:, 1]) * dd[1] - v[:, 2] * v[:, 1] * dd[2]) * i32
            out[:, 34] = -(-v[:, 0] * v[:, 2] * dd[0] - v[:, 1] * v[:, 2] * dd[1] + (s2 - v[:, 2] * v[:, 2]) * dd[2]) * i32
    out[~vis] = 0
    return out, int(((clx | cly) & vis).sum())


NSLOT = 10   # conic A, B, C | mean2D x, y | colour r, g, b | depth slot | opacity (read by the antialiasing h chain only)


def _slots(src, gz, P):
    z = lambda a, n: np.zeros((P, n)) if a is None else np.asarray(a, np.float64).reshape(P, -1)[:, :n]
    return np.concatenate([z(src["dL_dconic"], 3), z(src["dL_dmeans2D"], 2), z(src["dL_dcolors"], 3), z(gz, 1),
                           z(src.get("dL_dopacity"), 1)], 1)


def _split(a):
    return a[:, 0:3], a[:, 3:5], a[:, 5:8], a[:, 8], a[:, 9]


def reference(o, ref, budget, gz=None, gz_budget=None, aa_opacity=None):
    """(values [35], budget [35], carried [35], clamped count) in float64.  ref / budget: backward_ref64's dicts (dL_dconic,
    dL_dmeans2D, dL_dcolors, and dL_dopacity for antialiasing); gz / gz_budget: the depth slot and its budget (None = 0)."""
    P = o["P"]
    a, s = _slots(ref, gz, P), _slots(budget, gz_budget, P)
    vis = (np.asarray(o["radii"]) > 0)[:, None]
    a, s = a * vis, s * vis
    val, bud, car = np.zeros(35), np.zeros(35), np.zeros(35)
    ncl = 0
    for j in range(NSLOT if aa_opacity is not None else NSLOT - 1):
        for src, dst in ((a, None), (s, car)):
            one = np.zeros_like(src); one[:, j] = src[:, j]
            t, ncl = terms(o, *_split(one), dtype=np.float64, aa_opacity=aa_opacity)
            if dst is None:
                val += t.sum(0); bud += np.abs(t).sum(0)
            else:
                dst += KAPPA * EPS32 * np.abs(t).sum(0)
    return val, bud, car, ncl


def twin32(o, ref, gz=None, aa_opacity=None):
    """The float32 twin: the same expressions in numpy float32 on the float32-rounded sums, added in index order."""
    a = _slots(ref, gz, o["P"]).astype(np.float32)
    t, _ = terms(o, *_split(a), dtype=np.float32, aa_opacity=aa_opacity)
    acc = np.zeros(35, np.float32)
    for i in np.nonzero(np.asarray(o["radii"]) > 0)[0]:
        acc = acc + t[i]
    return acc.astype(np.float64)


def share(o, ref, budget, gz=None, gz_budget=None, aa_opacity=None):
    """Largest |twin - ref64| / (2^-24 budget) over the 35 values, beyond what the float32 rounding of the sums themselves
    accounts for (that rounding is inside `carried`: half an ulp of a sum is below KAPPA 2^-24 of its budget only where the
    budget is large, so it is subtracted explicitly)."""
    val, bud, car, _ = reference(o, ref, budget, gz, gz_budget, aa_opacity)
    tw = twin32(o, ref, gz, aa_opacity)
    a = _slots(ref, gz, o["P"])
    rounding = np.zeros(35)
    for j in range(NSLOT):
        one = np.zeros_like(a); one[:, j] = np.abs(a[:, j] - a[:, j].astype(np.float32).astype(np.float64))
        t, _ = terms(o, *_split(one), dtype=np.float64, aa_opacity=aa_opacity)
        rounding += np.abs(t).sum(0)
    err = np.maximum(np.abs(tw - val) - rounding, 0.0)
    return float((err / np.maximum(EPS32 * bud, 1e-300))[bud > 0].max(initial=0.0))


def adversarial_copy():
    """_util.adversarial_inputs() -- duplicates, points behind the camera, zero and full opacity, splats far larger than the image
    (whose view-space x, y the forward clamps) and smaller than a pixel, off-screen centres, a zero quaternion, an oblique camera
    -- with three members softened, because a sum over Gaussians cannot leave a Gaussian out and the budget here does not follow
    the conditioning inside one Gaussian's arithmetic:
      the five 1/255 opacities are 2/255    on the floor itself every pixel of those Gaussians is a fragile pair;
      the needles are (0.3, 0.02, 0.02)     at (2, 1e-4, 1e-4) one needle's own float32 arithmetic loses 4.6e5 x 2^-24 of the budget;
      the near-plane pair is at z = 0.199 (culled) and z = 0.5    at z = 0.2 + 5e-8 the divide by h3 loses 490 x 2^-24."""
    import torch
    d = adversarial_inputs()
    op, sc, xyz = d["opacities"].clone(), d["scales"].clone(), d["means3D"].clone()
    op[120:125] = 2.0 / 255.0
    sc[170:175, 0] = 0.3; sc[170:175, 1:] = 0.02
    view = d["viewmatrix"]
    cam_pos, fwd = torch.inverse(view)[3, :3], view[:3, 2]
    xyz[90] = cam_pos + 0.199 * fwd
    xyz[91] = cam_pos + 0.5 * fwd
    d.update(opacities=op.contiguous(), scales=sc.contiguous(), means3D=xyz.contiguous())
    return d


# name -> scene; every one is checked (host test) to flag no Gaussian on the alpha floor
SCENES = {
    "shell": lambda: scene_inputs(P=300, size=40, kind="shell", lsm=-4.0, seed=3, width=40, height=24),
    "adversarial": adversarial_copy,
    "p1": lambda: scene_inputs(P=1, size=32, lsm=-3.0, seed=1),
    "p65": lambda: scene_inputs(P=65, size=32, lsm=-3.5, seed=2),
    "p257": lambda: scene_inputs(P=257, size=32, lsm=-4.0, seed=4),
    "p70001": lambda: scene_inputs(P=70001, size=32, lsm=-7.5, seed=6),
    "sh3": lambda: scene_inputs(P=300, size=40, kind="shell", lsm=-4.0, seed=3, width=40, height=24, sh_degree=3),
    "sh1_m16": lambda: scene_inputs(P=300, size=40, kind="shell", lsm=-4.0, seed=3, width=40, height=24, sh_degree=1, sh_M=16),
    "colors": lambda: scene_inputs(P=300, size=40, kind="shell", lsm=-4.0, seed=3, width=40, height=24, use_colors=True),
    "cov": lambda: scene_inputs(P=300, size=40, kind="shell", lsm=-4.0, seed=3, width=40, height=24, use_cov=True),
}
INSTANCE_SCENE = "sh1_m16"   # the scene of the antialiasing, depth / alpha, feature + distortion and fused-activation cases


def depth_slot(o, g_depth, g_alpha, lists=None):
    """(gz [P], its budget [P]) of the depth / alpha maps' backward: the pseudo-colour construction of tests/_depth_alpha_ref.py,
    whose colour-channel-0 gradient is dL/dz.  lists: the decoded native forward (default: the oracle's own lists)."""
    from _depth_alpha_ref import pseudo_rgb
    from oracle import ggd_oracle as O
    rgb = pseudo_rgb(o)
    o_aux = dict(o, rgb=rgb, bg=np.zeros(3, np.float32), colors_precomp=rgb)
    g_aux = np.stack([np.asarray(g_depth, np.float32), np.asarray(g_alpha, np.float32), np.zeros_like(np.asarray(g_depth, np.float32))])
    kw = {} if lists is None else dict(final_T=lists["final_T"], n_contrib=lists["n_contrib"], point_list=lists["point_list"],
                                       ranges=lists["ranges"])
    r, b, _ = O.backward_ref64(o_aux, g_aux, **kw)
    vis = np.asarray(o["radii"]) > 0
    return r["dL_dcolors"][:, 0] * vis, b["dL_dcolors"][:, 0] * vis


def tolerance(bud, car):
    return ATOL + car + K * EPS32 * bud
