"""fp64 reference of the opt-in anti-aliasing (opacity-compensated 2D filter, ggd_params.antialiasing), test-only.

With (x, z, y) the EWA 2D covariance of a Gaussian BEFORE the 0.3 px^2 dilation and w = 0.3:
    det0 = x y - z^2,  det1 = (x + w)(y + w) - z^2,  r = det0 / det1,  h = sqrt(max(2.5e-5, r)),  o_eff = o h.
The covariance restates oracle/torch_raster.preprocess without the + 0.3, for scales / rotations or cov3D_precomp and any
scale_modifier, in float64 torch.  Like the kernels (and upstream), a view-space x / y clamped to the 1.3 tan(fov) frustum is
treated as a constant, so the gradients below follow the same convention as the rest of the backward.

Everything takes the activated attributes (opacity after the sigmoid, normalised quaternion, exp'd scales)."""
from __future__ import annotations

import numpy as np
import torch

W_DIL = 0.3
R_MIN = 2.5e-5
EPS32 = 2.0 ** -24


def _f64(t):
    return None if t is None else torch.as_tensor(t).detach().to(torch.float64).clone()


def cov6_from_scale_rot(scales, rotations, mod):
    """Sigma = R S S R^T (quaternion (w, x, y, z) as given), stored (S00, S01, S02, S11, S12, S22)."""
    r, x, y, z = rotations.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    L = R * (mod * scales)[:, None, :]
    S = L @ L.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)


def cov2d(d, means3D, cov6):
    """(x, z, y): the undilated EWA 2D covariance [P] each, differentiable w.r.t. means3D and cov6 (float64 tensors).
    Points at or behind the near plane get a placeholder depth (their values are meaningless but finite)."""
    f32 = lambda v: float(np.float32(v))          # the kernels see the fp32 camera constants
    tanfx, tanfy = f32(d["tanfovx"]), f32(d["tanfovy"])
    V = _f64(d["viewmatrix"]).reshape(4, 4)
    P = means3D.shape[0]
    t = torch.cat([means3D, torch.ones(P, 1, dtype=torch.float64)], 1) @ V
    tz = torch.where(t[:, 2] > 0.2, t[:, 2], torch.ones_like(t[:, 2]))
    fx, fy = d["W"] / (2.0 * tanfx), d["H"] / (2.0 * tanfy)

    def clamped(u, lim):   # a coordinate clamped to the frustum is a constant (no gradient), as in the kernels
        q = u / tz
        out = (q < -lim) | (q > lim)
        return torch.where(out, (torch.clamp(q, -lim, lim) * tz).detach(), u)
    tx, ty = clamped(t[:, 0], 1.3 * tanfx), clamped(t[:, 1], 1.3 * tanfy)
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz)], 1),
                     torch.stack([zero, fy / tz, -(fy * ty) / (tz * tz)], 1)], 1)
    T = J @ V[:3, :3].t()
    c = cov6
    Sg = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).view(-1, 3, 3)
    C2 = T @ Sg @ T.transpose(1, 2)
    return C2[:, 0, 0], C2[:, 0, 1], C2[:, 1, 1]


def h_of(x, z, y, w=W_DIL):
    """h = sqrt(max(2.5e-5, det0 / det1)); the max is fmaxf's (a NaN ratio gives the floor)."""
    det0 = x * y - z * z
    det1 = (x + w) * (y + w) - z * z
    r = det0 / det1
    return torch.sqrt(torch.fmax(r, torch.full_like(r, R_MIN)))


def _inputs(d, grad):
    mk = (lambda t: None if t is None else _f64(t).requires_grad_(True)) if grad else _f64
    means3D = mk(d["means3D"])
    if d.get("cov3D_precomp") is not None:
        scales = rotations = None
        cov6 = mk(_f64(d["cov3D_precomp"]).reshape(-1, 6))
    else:
        scales, rotations = mk(d["scales"]), mk(d["rotations"])
        cov6 = cov6_from_scale_rot(scales, rotations, float(np.float32(d["scale_modifier"])))
        if grad:
            cov6.retain_grad()
    return means3D, scales, rotations, cov6


def h_and_conditioning(d):
    """(h, cond) as float64 numpy [P]: cond = 1 + (|x y| + z^2) / |det0| bounds the relative rounding of det0 = x y - z^2 in
    units of the fp32 epsilon (the cancellation the kernels' fp32 h inherits); 1 where the clamp holds h constant."""
    with torch.no_grad():
        means3D, _, _, cov6 = _inputs(d, False)
        x, z, y = cov2d(d, means3D, cov6)
        h = h_of(x, z, y)
        det0 = x * y - z * z
        cond = 1.0 + (torch.abs(x * y) + z * z) / torch.abs(det0)
        cond = torch.where(h > np.sqrt(R_MIN), cond, torch.ones_like(cond))
    return h.numpy(), np.nan_to_num(cond.numpy(), nan=1.0, posinf=1e30)


def o_eff(d):
    """o h, float64 numpy [P] (d["opacities"] are the activated opacities)."""
    h, _ = h_and_conditioning(d)
    return _f64(d["opacities"]).reshape(-1).numpy() * h


def vjp(d, g_oeff):
    """The anti-aliasing share of the backward for dL/do_eff = g_oeff [P] (zero for culled Gaussians): returns float64 numpy
    dL_dopacity = g h (the whole opacity gradient) and the h chain of dL_dmeans3D, dL_dcov3D, dL_dscales, dL_drots (to be
    added to the plain backward evaluated at o_eff)."""
    means3D, scales, rotations, cov6 = _inputs(d, True)
    x, z, y = cov2d(d, means3D, cov6)
    h = h_of(x, z, y)
    g = torch.as_tensor(np.asarray(g_oeff, np.float64)).reshape(-1)
    o = _f64(d["opacities"]).reshape(-1)
    (g * o * h).sum().backward()
    npy = lambda t: t.grad.numpy().copy()
    out = dict(dL_dopacity=(g * h).detach().numpy().reshape(-1, 1), dL_dmeans3D=npy(means3D), dL_dcov3D=npy(cov6))
    if scales is not None:
        out.update(dL_dscales=npy(scales), dL_drots=npy(rotations))
    return out


def chain_conditioning(d):
    """(magnitude, rounding share) of the h chain d(o h)/dp, from one evaluation of (x, z, y) and h:

    magnitude[array] = sum_u |d(o h)/du du/dp| over u in (x, z, y), float64 numpy per gradient array, >= |d(o h)/dp|: the three
    terms the kernels add up (dL/da, dL/db, dL/dc taken on through T) before any of them cancels.

    share = sum_j |d^2(o h) / dSigma_k dSigma_j| dSigma_j, float64 numpy [P, 6] in units of eps32: where Sigma = R S S R^T is
    evaluated in fp32 (scales / rotations given) its entries carry the rounding the oracle's error analysis gives them
    (ggo_cov3d_all_err) -- for a nearly isotropic Gaussian the off-diagonal entries are what is left of cancelling terms -- and
    d(o h)/dSigma is taken at that rounded Sigma.  Zeros for a precomputed covariance."""
    import ctypes as C
    from oracle import ggd_oracle as O
    means3D, scales, rotations, cov6 = _inputs(d, True)
    params = dict(dL_dmeans3D=means3D, dL_dcov3D=cov6)
    if scales is not None:
        params.update(dL_dscales=scales, dL_drots=rotations)
    P = means3D.shape[0]
    o = _f64(d["opacities"]).reshape(-1)
    xzy = cov2d(d, means3D, cov6)
    oh = (o * h_of(*xzy)).sum()
    d_du = torch.autograd.grad(oh, xzy, retain_graph=True)                      # d(o h)/dx, /dz, /dy  [P] each
    mag = {k: np.zeros(tuple(t.shape)) for k, t in params.items()}
    for u in range(3):
        grads = torch.autograd.grad(xzy[u], list(params.values()), grad_outputs=d_du[u], retain_graph=True)
        for k, gr in zip(params, grads):
            mag[k] += np.abs(gr.numpy())
    share = np.zeros((P, 6))
    if scales is not None:
        er = lambda t: np.ascontiguousarray(np.stack([_f64(t).numpy(), np.zeros(tuple(t.shape))], axis=-1))
        cov_err = np.zeros((P, 6, 2), np.float64)
        mod = float(np.float32(d["scale_modifier"]))
        O.lib().ggo_cov3d_all_err(P, O._p(er(d["scales"])), C.c_double(mod), O._p(er(d["rotations"])), O._p(cov_err))
        dS = torch.as_tensor(cov_err[..., 1])
        (G,) = torch.autograd.grad(oh, cov6, create_graph=True)                  # [P, 6]
        for k in range(6):
            (Hk,) = torch.autograd.grad(G[:, k].sum(), cov6, retain_graph=True)
            share[:, k] = (Hk.abs() * dS).sum(1).numpy()
        share = np.nan_to_num(share, nan=0.0, posinf=0.0)
    return mag, share


def compose_backward(d, ref, budget, rel=64.0, kappa=0.25):
    """The plain fp64 reference `ref` / `budget` (oracle backward_ref64 at o_eff) turned into the anti-aliasing one: its
    dL_dopacity (= dL/do_eff) is replaced by g h and the h chain g d(o h)/dp is added to the geometric gradients.  The fp32
    chain differs from that product in three ways, each allowed for on top of the plain budget, in the units check_gradients
    applies kappa * eps32 to:
      * its own arithmetic: rel * eps32 * cond per term (cond from h_and_conditioning: the fp32 h carries the cancellation of
        det0), over the magnitude sum_u |g d(o h)/du du/dp| of the three terms it adds (chain_conditioning) -- not over their
        sum, which cancels for the off-diagonal covariance entries;
      * g itself is the blend's fp32 sum with the error budget[dL_dopacity] of its own, which the chain multiplies by
        |d(o h)/dp| <= that magnitude: thousands for a sub-pixel splat on a small image (d h / d x ~ h / (2 x), T^2 ~ (f / z)^2),
        where an error of g far inside its own bound is the whole error of dL/dcov3D;
      * dL/dcov3D is taken at the fp32 Sigma (the rounding share of chain_conditioning).  The off-diagonal 2D covariance z of a nearly isotropic
        splat is a few 1e-5 px^2 made of Sigma's off-diagonal entries, themselves cancellation residues: d(o h)/dSigma_01 is
        linear in z and inherits hundreds of eps32."""
    g = ref["dL_dopacity"].reshape(-1)
    aa = vjp(d, g)
    h, cond = h_and_conditioning(d)
    mag, share = chain_conditioning(d)
    out_ref, out_bud = dict(ref), dict(budget)
    scale = rel / kappa
    out_ref["dL_dopacity"] = aa["dL_dopacity"].reshape(ref["dL_dopacity"].shape)
    out_bud["dL_dopacity"] = (budget["dL_dopacity"].reshape(-1) * h
                              + scale * cond * np.abs(aa["dL_dopacity"].reshape(-1))).reshape(ref["dL_dopacity"].shape)
    for k in ("dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drots"):
        if k not in aa or ref.get(k) is None:
            continue
        t = aa[k].reshape(ref[k].shape)
        col = lambda v: np.asarray(v, np.float64).reshape((-1,) + (1,) * (t.ndim - 1))
        out_ref[k] = ref[k] + t
        # (a culled Gaussian has g = 0 and no budget of it: its gradients stay exact zeros)
        out_bud[k] = budget[k] + (scale * col(cond) * col(np.abs(g)) + col(budget["dL_dopacity"])) * mag[k].reshape(t.shape)
        if k == "dL_dcov3D":
            out_bud[k] = out_bud[k] + col(np.abs(g)) * share.reshape(t.shape)
    return out_ref, out_bud
