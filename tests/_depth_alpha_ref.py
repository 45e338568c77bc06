"""Reference construction for the depth / alpha extension (ggd_forward_aux / ggd_backward_aux), from the unchanged oracle.

Depth and alpha are blends of per-Gaussian constants over a zero background: with the pseudo-colour rgb := [z, 1, 0] and
bg := 0 the oracle's blend writes the depth map into channel 0 and the alpha map into channel 1, and the gradient of that
pseudo-colour image w.r.t. everything but the colours is the extension's.  The depth gradient reaches the means through z
itself as well: dL/dz (= dL/dcolour channel 0 of the pseudo-colour) times dz/dmean = (view[2], view[6], view[10])."""
from __future__ import annotations

import ctypes as C

import numpy as np

from _util import EPS32, backward_reference


def pseudo_rgb(o):
    z = np.asarray(o["depths"], np.float32)
    return np.ascontiguousarray(np.stack([z, np.ones_like(z), np.zeros_like(z)], 1).astype(np.float32))


def forward_ref(o):
    """(depth[H, W], alpha[H, W]) of the fp32 oracle forward `o`, blended by the oracle over its own lists."""
    from oracle import ggd_oracle as O
    L = O.lib()
    W, H = o["W"], o["H"]
    color = np.zeros((3, H, W), np.float32)
    fT = np.zeros((H, W), np.float32)
    nc = np.zeros((H, W), np.uint32)
    bg0 = np.zeros(3, np.float32)
    rgb = pseudo_rgb(o)
    L.ggo_render_f32(C.byref(o["prm"]), O._p(bg0), O._p(o["ranges"]), O._p(o["point_list"]), O._p(o["xy"]),
                     O._p(o["conic_opacity"]), O._p(rgb), O._p(color), O._p(fT), O._p(nc))
    return color[0], color[1]


def backward_ref(d, o, n, g_rgb, g_depth, g_alpha):
    """fp64 reference + fp32 budget of ggd_backward_aux for one forward (o = fp32 oracle forward of d, n = run_native(d)):
    the colour reference plus the pseudo-colour reference (every array but dL_dcolors / dL_dsh), plus the depth term of
    dL_dmeans3D.  Returns (ref, budget, fragile) in the form of _util.backward_reference."""
    ref, bud, frag = backward_reference(d, o, n, np.asarray(g_rgb, np.float32))
    rgb = pseudo_rgb(o)
    o_aux = dict(o, rgb=rgb, bg=np.zeros(3, np.float32), colors_precomp=rgb)
    g_aux = np.stack([np.asarray(g_depth, np.float32), np.asarray(g_alpha, np.float32),
                      np.zeros_like(np.asarray(g_depth, np.float32))])
    from oracle import ggd_oracle as O
    ref_a, bud_a, frag_a = O.backward_ref64(o_aux, g_aux, final_T=n["final_T"], n_contrib=n["n_contrib"],
                                            point_list=n["point_list"], ranges=n["ranges"])
    out_ref, out_bud = {}, {}
    for k, r in ref.items():
        if k in ("dL_dcolors", "dL_dsh") or r is None or ref_a.get(k) is None:
            out_ref[k], out_bud[k] = r, bud[k]
            continue
        out_ref[k] = r + ref_a[k]
        out_bud[k] = bud[k] + bud_a[k]
    vis = (o["radii"] > 0)[:, None]
    v = np.asarray(o["viewmatrix"], np.float64).reshape(-1)
    dz = ref_a["dL_dcolors"][:, 0:1]
    col = np.array([v[2], v[6], v[10]])[None, :]
    out_ref["dL_dmeans3D"] = out_ref["dL_dmeans3D"] + vis * dz * col
    # the fp32 product dz * view and its sum into the mean gradient: the conditioning of dz, scaled, plus two roundings
    out_bud["dL_dmeans3D"] = (out_bud["dL_dmeans3D"] + vis * (bud_a["dL_dcolors"][:, 0:1] + 2.0 * np.abs(dz)) * np.abs(col)
                              + 2.0 * np.abs(out_ref["dL_dmeans3D"]))
    return out_ref, out_bud, np.maximum(frag, frag_a)


__all__ = ["pseudo_rgb", "forward_ref", "backward_ref", "EPS32"]
