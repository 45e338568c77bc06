"""Reference for the absolute screen-space gradients (absgrad; ggd_backward_abs): SURVEY.md 9.5 restated in float64 numpy.

Per pixel q and contributing record of Gaussian i, with dL/dG = opacity * dL/dalpha and d = mean - pixel:

    g_x(q, i) = dL/dG * G * (-A d.x - B d.y)        g_y(q, i) = dL/dG * G * (-C d.y - B d.x)
    signed[i] = (0.5 W sum_q g_x, 0.5 H sum_q g_y)       (means2D.grad, what the oracle's backward_ref64 returns)
    abs[i]    = (0.5 W sum_q |g_x|, 0.5 H sum_q |g_y|)   (means2D.absgrad)

`blend_sums` walks every 16 x 16 tile over the state a forward saved (final_T, n_contrib, point_list, ranges, xy,
conic_opacity, rgb).  WHICH (pixel, Gaussian) pairs contribute is decided in float32 exactly as the forward decides it (the
power of the oracle's gauss_power, expf, the 1/255 floor, positions below n_contrib); every value is then float64, as in
oracle/ggd_oracle.c::ggo_render_backward_ref64.  The blend is linear in the colour channels, so the depth / alpha terms of a
render_depth_alpha backward are two more channels (z, 1) over background 0 (tests/_depth_alpha_ref.py's pseudo-colour): the
absolute value is taken of the per-pixel SUM over all channels, which no sum of two oracle calls can give.

tests/test_absgrad_host.py vouches for this file: on the oracle's own forward state its signed sums are backward_ref64's.

Error budget of abs[i]: the unchanged oracle's budget["dL_dmeans2D"].  That budget is sum_q (roundings weight) * |factors| with
every product of a term, the two products inside (-A d.x - B d.y) included, taken in absolute value: it bounds the rounding
error of each per-pixel TERM, whatever its sign, so it holds for a sum of |terms| as it does for the sum of terms (|.| is
1-Lipschitz: the error of |t| is at most the error of t).  Rounding count of the form the kernel evaluates: per pixel
wx = (G dx) dL/dalpha (2 roundings), nB wy (1), the fma with 2 hA wx (1), then the sum, then op * 0.5 W (1) and the final
product (1): six.  The signed path applies the same six operations, four of them before the sum and the conic map after it:
six as well.  The weight of a term in the oracle's budget is 4 + relT + relG >= 6 on top of those of G, alpha and T, so the
budget is used as it is; KAPPA and ATOL stay tests/_util.py's.  Nothing here is taken from the kernel under test."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def _fma32(a, b, c):
    """float32 fma of float32 arrays: the product of two floats is exact in double; one rounding of the double sum, one to
    float (a double rounding can differ from a true fma only on a tie of the last bit)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def state_of(fwd, rgb=None, bg=None):
    """the blend state of a forward dict (the oracle's, or tests/_util.py::decode_result's of a native forward); rgb [P, C] and
    bg [C] replace the forward's colours and background when given (more channels than three are fine)"""
    return dict(W=int(fwd["W"]), H=int(fwd["H"]), final_T=np.asarray(fwd["final_T"], F32), n_contrib=np.asarray(fwd["n_contrib"]),
                point_list=np.asarray(fwd["point_list"]), ranges=np.asarray(fwd["ranges"]).reshape(-1, 2),
                xy=np.asarray(fwd["xy"], F32), conic_opacity=np.asarray(fwd["conic_opacity"], F32),
                rgb=np.asarray(fwd["rgb"] if rgb is None else rgb, F32), bg=np.asarray(fwd["bg"] if bg is None else bg, F32))


def blend_sums(st, dL_dpix):
    """(signed [P, 2], abs [P, 2]) in float64 for the state `st` (state_of) and the upstream gradient dL_dpix [C, H, W]"""
    W, H = st["W"], st["H"]
    gx_tiles = (W + 15) // 16
    xy, co, rgb = st["xy"], st["conic_opacity"], st["rgb"].astype(np.float64)
    bg = st["bg"].astype(np.float64)
    g = np.asarray(dL_dpix, F32).astype(np.float64).reshape(rgb.shape[1], H, W)
    P = xy.shape[0]
    signed, absd = np.zeros((P, 2)), np.zeros((P, 2))
    cap, floor = F32(0.99), F32(1.0) / F32(255.0)
    for tile in range(gx_tiles * ((H + 15) // 16)):
        tx, ty = tile % gx_tiles, tile // gx_tiles
        ys, xs = np.meshgrid(np.arange(ty * 16, min(ty * 16 + 16, H)), np.arange(tx * 16, min(tx * 16 + 16, W)), indexing="ij")
        px, py = xs.reshape(-1), ys.reshape(-1)
        last = st["n_contrib"][py, px].astype(np.int64)
        n = int(last.max(initial=0))
        if n == 0:
            continue
        lo = int(st["ranges"][tile, 0])
        ids = st["point_list"][lo:lo + n].astype(np.int64)
        A32, B32, C32, o32 = (co[ids, k][None, :] for k in range(4))
        # ---- decisions: float32, the forward's
        dxf = xy[ids, 0][None, :] - px.astype(F32)[:, None]
        dyf = xy[ids, 1][None, :] - py.astype(F32)[:, None]
        t1 = ((F32(-0.5) * C32) * dyf) * dyf
        t2 = (-B32) * dyf
        power32 = _fma32(_fma32(np.broadcast_to(F32(-0.5) * A32, dxf.shape), dxf, t2), dxf, t1)
        with np.errstate(over="ignore"):   # (a positive power is never blended)
            alpha32 = np.minimum(cap, o32 * np.exp(power32, dtype=F32))
        live = (np.arange(n)[None, :] < last[:, None]) & ~(power32 > 0) & ~(alpha32 < floor)
        # ---- values: float64 from the same float32 inputs
        A, B, C, o = (v.astype(np.float64) for v in (A32, B32, C32, o32))
        dx = xy[ids, 0].astype(np.float64)[None, :] - px[:, None]
        dy = xy[ids, 1].astype(np.float64)[None, :] - py[:, None]
        power = ((-0.5 * A) * dx + (-B) * dy) * dx + ((-0.5 * C) * dy) * dy
        G = np.where(live, np.exp(np.minimum(power, 0.0)), 0.0)
        alpha = np.where(live, np.minimum(np.float64(cap), o * G), 0.0)
        om = 1.0 - alpha
        Tf = st["final_T"][py, px].astype(np.float64)[:, None]
        # transmittance in front of record j: final_T over the product of (1 - alpha) of j and everything behind it
        T = Tf / np.cumprod(om[:, ::-1], axis=1)[:, ::-1]
        wgt = alpha * T
        dL_dalpha = np.zeros_like(T)
        for ch in range(rgb.shape[1]):
            c = rgb[ids, ch][None, :]
            cw = c * wgt
            behind = np.cumsum(cw[:, ::-1], axis=1)[:, ::-1] - cw       # sum over the records behind j of c alpha T
            dL_dalpha += (c - behind / (T * om)) * g[ch, py, px][:, None]
        bgdot = (bg[None, :] * g[:, py, px].T).sum(1)[:, None]
        dL_dalpha = dL_dalpha * T - (Tf / om) * bgdot
        dL_dG = o * dL_dalpha
        gdx, gdy = G * dx, G * dy
        tx_ = dL_dG * (-gdx * A - gdy * B) * (0.5 * W)
        ty_ = dL_dG * (-gdy * C - gdx * B) * (0.5 * H)
        signed[ids, 0] += tx_.sum(0); signed[ids, 1] += ty_.sum(0)
        absd[ids, 0] += np.abs(tx_).sum(0); absd[ids, 1] += np.abs(ty_).sum(0)
    return signed, absd


def aux_channels(o, g_rgb, g_depth, g_alpha):
    """(rgb [P, 5], bg [5], dL_dpix [5, H, W]): the colour plus the depth / alpha pseudo-colour (z, 1) over background 0"""
    z = np.asarray(o["depths"], F32)
    rgb = np.concatenate([np.asarray(o["rgb"], F32), z[:, None], np.ones_like(z)[:, None]], 1)
    bg = np.concatenate([np.asarray(o["bg"], F32), np.zeros(2, F32)])
    H, W = o["H"], o["W"]
    g = np.concatenate([np.asarray(g_rgb, F32).reshape(3, H, W), np.asarray(g_depth, F32).reshape(1, H, W),
                        np.asarray(g_alpha, F32).reshape(1, H, W)])
    return rgb, bg, g


def reference(d, o, n, g_rgb, g_depth=None, g_alpha=None):
    """(ref, budget, fragile, signed) of an absgrad backward for the native forward `n` of `d` (o: the fp32 oracle forward of d): the
    eight usual arrays from the unchanged oracle (tests/_util.py::backward_reference, with the depth / alpha gradients
    tests/_depth_alpha_ref.py::backward_ref), plus ref["dL_dmeans2D_abs"] [P, 3] from blend_sums over n's saved state, under
    budget["dL_dmeans2D"]; `signed` [P, 3] is blend_sums' signed sum (ref["dL_dmeans2D"] up to float64 rounding)."""
    from _depth_alpha_ref import backward_ref
    from _util import backward_reference
    aux = g_depth is not None or g_alpha is not None
    nn = dict(n, W=o["W"], H=o["H"], bg=o["bg"])
    if aux:
        zero = np.zeros((o["H"], o["W"]), F32)
        g_depth = zero if g_depth is None else np.asarray(g_depth, F32).reshape(o["H"], o["W"])
        g_alpha = zero if g_alpha is None else np.asarray(g_alpha, F32).reshape(o["H"], o["W"])
        ref, bud, frag = backward_ref(d, o, n, np.asarray(g_rgb, F32), g_depth, g_alpha)
        rgb, bg, g = aux_channels(dict(o, rgb=n["rgb"]), g_rgb, g_depth, g_alpha)
        signed, absd = blend_sums(state_of(nn, rgb=rgb, bg=bg), g)
    else:
        ref, bud, frag = backward_reference(d, o, n, np.asarray(g_rgb, F32))
        signed, absd = blend_sums(state_of(nn), np.asarray(g_rgb, F32))
    vis = (np.asarray(o["radii"]) > 0)[:, None]
    ref, bud = dict(ref), dict(bud)
    ref["dL_dmeans2D_abs"] = np.concatenate([absd * vis, np.zeros((absd.shape[0], 1))], 1)
    bud["dL_dmeans2D_abs"] = bud["dL_dmeans2D"]
    return ref, bud, frag, np.concatenate([signed * vis, np.zeros((absd.shape[0], 1))], 1)
