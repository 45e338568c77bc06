"""Reference construction for the feature maps (ggd_forward_features / ggd_backward_features), from the unchanged oracle.

A feature map is a blend of per-Gaussian constants: the C channels are cut into ceil(C / 3) pseudo-colour triples (the last one
zero-padded, each with its background triple from feature_bg), the oracle's fp32 blend of a triple over its own lists gives three
planes of the forward, and backward_ref64 of a triple over the NATIVE run's final_T / n_contrib / lists gives that triple's share
of every geometric gradient (with its error budget) and, as its dL_dcolors, three columns of dL_dfeatures."""
from __future__ import annotations

import ctypes as C

import numpy as np

from _util import backward_reference


def triples(features, feature_bg=None):
    """[(rgb float32 [P, 3], bg float32 [3], channels)] for features [P, C]: channels = the triple's real channel indices"""
    f = np.asarray(features, np.float32)
    P, Cn = f.shape
    bgv = np.zeros(Cn, np.float32) if feature_bg is None else np.asarray(feature_bg, np.float32).reshape(Cn)
    out = []
    for c0 in range(0, Cn, 3):
        ch = list(range(c0, min(c0 + 3, Cn)))
        rgb = np.zeros((P, 3), np.float32)
        bg = np.zeros(3, np.float32)
        rgb[:, :len(ch)] = f[:, ch]
        bg[:len(ch)] = bgv[ch]
        out.append((np.ascontiguousarray(rgb), bg, ch))
    return out


def forward_ref(o, features, feature_bg=None):
    """F [C, H, W] float32: the fp32 oracle forward `o`'s blend of every triple over its own lists"""
    from oracle import ggd_oracle as O
    L = O.lib()
    W, H = o["W"], o["H"]
    Cn = np.asarray(features).shape[1]
    F = np.zeros((Cn, H, W), np.float32)
    for rgb, bg, ch in triples(features, feature_bg):
        color = np.zeros((3, H, W), np.float32)
        fT = np.zeros((H, W), np.float32)
        nc = np.zeros((H, W), np.uint32)
        L.ggo_render_f32(C.byref(o["prm"]), O._p(bg), O._p(o["ranges"]), O._p(o["point_list"]), O._p(o["xy"]),
                         O._p(o["conic_opacity"]), O._p(rgb), O._p(color), O._p(fT), O._p(nc))
        F[ch] = color[:len(ch)]
    return F


def triple_gradients(g_feat, ch):
    """the [3, H, W] upstream gradient of a triple (zero planes for its padding channels)"""
    g = np.asarray(g_feat, np.float32)
    out = np.zeros((3,) + g.shape[1:], np.float32)
    out[:len(ch)] = g[ch]
    return out


def backward_ref(d, o, n, g_rgb, features, feature_bg, g_feat, g_depth=None, g_alpha=None):
    """fp64 reference + fp32 budget of ggd_backward_features for one forward (o = fp32 oracle forward of d, n = the decoded native
    forward): the colour reference (with the depth / alpha one when g_depth / g_alpha are given) plus every triple's, summed over
    all arrays but dL_dcolors / dL_dsh; ref["dL_dfeatures"] [P, C] = the triples' dL_dcolors.  Returns (ref, budget, fragile) in the
    form of _util.backward_reference."""
    from oracle import ggd_oracle as O
    if g_depth is not None or g_alpha is not None:
        from _depth_alpha_ref import backward_ref as aux_ref
        z = np.zeros((o["H"], o["W"]), np.float32)
        ref, bud, frag = aux_ref(d, o, n, g_rgb, z if g_depth is None else g_depth, z if g_alpha is None else g_alpha)
    else:
        ref, bud, frag = backward_reference(d, o, n, np.asarray(g_rgb, np.float32))
    ref, bud = dict(ref), dict(bud)
    P, Cn = np.asarray(features).shape
    ref_f, bud_f = np.zeros((P, Cn)), np.zeros((P, Cn))
    for rgb, bg, ch in triples(features, feature_bg):
        o_t = dict(o, rgb=rgb, bg=bg, colors_precomp=rgb)
        r, b, fr = O.backward_ref64(o_t, triple_gradients(g_feat, ch), final_T=n["final_T"], n_contrib=n["n_contrib"],
                                    point_list=n["point_list"], ranges=n["ranges"])
        for k in ref:
            if k in ("dL_dcolors", "dL_dsh") or ref[k] is None or r.get(k) is None:
                continue
            ref[k] = ref[k] + r[k]
            bud[k] = bud[k] + b[k]
        ref_f[:, ch] = r["dL_dcolors"][:, :len(ch)]
        bud_f[:, ch] = b["dL_dcolors"][:, :len(ch)]
        frag = np.maximum(frag, fr)
    ref["dL_dfeatures"], bud["dL_dfeatures"] = ref_f, bud_f
    return ref, bud, frag


def blend_f64(o, features, feature_bg=None):
    """A direct float64 C-channel blend written out in numpy over the oracle forward's lists and per-Gaussian records, taking the
    fp32 oracle's decisions (n_contrib bounds every pixel's walk; inside it the skip rules are re-evaluated in float64): F [C, H, W]."""
    f = np.asarray(features, np.float64)
    P, Cn = f.shape
    bg = np.zeros(Cn) if feature_bg is None else np.asarray(feature_bg, np.float64).reshape(Cn)
    W, H = o["W"], o["H"]
    gx = (W + 15) // 16
    xy, co = o["xy"].astype(np.float64), o["conic_opacity"].astype(np.float64)
    F = np.zeros((Cn, H, W))
    for y in range(H):
        for x in range(W):
            lo, _ = o["ranges"][(y // 16) * gx + x // 16]
            T = 1.0
            acc = np.zeros(Cn)
            for k in range(int(o["n_contrib"][y, x])):
                i = int(o["point_list"][int(lo) + k])
                dx, dy = xy[i, 0] - x, xy[i, 1] - y
                power = -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
                if power > 0.0:
                    continue
                alpha = min(0.99, co[i, 3] * np.exp(power))
                if alpha < 1.0 / 255.0:
                    continue
                acc += f[i] * alpha * T
                T *= 1.0 - alpha
            F[:, y, x] = acc + T * bg
    return F


__all__ = ["triples", "forward_ref", "backward_ref", "blend_f64", "triple_gradients"]
