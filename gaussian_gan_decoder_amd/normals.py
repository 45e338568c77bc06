"""Normal consistency: per-Gaussian view-space normals and the loss that holds their blend to the normals of
the surface the depth map describes -- the regulariser 2DGS, gsplat, GOF and PGSR pair with the distortion loss.

`gaussian_normals`: a splat's shortest axis in view space, turned towards the camera (ggd_gaussian_normals, one HIP launch each
way).  Blended as three feature channels (`render` / `render_simple(..., render_normals=True)`) they give the map N_r = sum alpha_i
T_i n_i.  `fused_normal_loss`: mean over the image of alpha - N_r . N_s, with N_s the unit normal of the back-projected expected
depth's central differences (ggd_normal_loss, two HIP launches, exact gradients in all three maps).  `depth_to_normal`: N_s alone.
`gaussian_normals_torch` / `normal_loss_torch`: the same two as torch expressions -- what CPU tensors get, and the composition the
kernels are timed against (scripts/normals_timing.py).
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F


def _normals_args(rotations, scales, means3D, viewmatrix, what):
    P = int(means3D.shape[0]) if means3D.dim() == 2 else -1
    if tuple(means3D.shape) != (P, 3) or tuple(scales.shape) != (P, 3) or tuple(rotations.shape) != (P, 4):
        raise ValueError(f"{what}: rotations [P,4], scales [P,3] and means3D [P,3] expected, got {tuple(rotations.shape)}, "
                         f"{tuple(scales.shape)}, {tuple(means3D.shape)}")
    if viewmatrix.numel() != 16:
        raise ValueError(f"{what}: viewmatrix must have 16 elements, got {tuple(viewmatrix.shape)}")
    tensors = (rotations, scales, means3D, viewmatrix)
    if any(t.dtype != rotations.dtype for t in tensors):
        raise TypeError(f"{what}: tensors of one dtype expected, got {[t.dtype for t in tensors]}")
    if any(t.device != rotations.device for t in tensors):
        raise RuntimeError(f"{what}: rotations, scales, means3D and viewmatrix must live on one device")
    return P


def gaussian_normals_torch(rotations, scales, means3D, viewmatrix, raw=False):
    """gaussian_normals as a torch expression in the tensors' own dtype and on their own device (about a dozen elementwise passes
    over P rows each way).  Differentiable in `rotations` only."""
    _normals_args(rotations, scales, means3D, viewmatrix, "gaussian_normals_torch")
    q = F.normalize(rotations, dim=1) if raw else rotations   # v / max(|v|, 1e-12): the fused-activation prologue's rule
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    s = scales.detach()
    k = (s[:, 1] < s[:, 0]).long()                              # argmin, ties to the lowest index
    k = torch.where(s[:, 2] < torch.minimum(s[:, 0], s[:, 1]), torch.full_like(k, 2), k)
    n_w = R.gather(2, k[:, None, None].expand(-1, 3, 1)).squeeze(2)
    V = viewmatrix.detach().reshape(4, 4)
    n_v = n_w @ V[:3, :3]
    p_v = means3D.detach() @ V[:3, :3] + V[3, :3]
    away = (n_v.detach() * p_v).sum(1) > 0
    return torch.where(away[:, None], -n_v, n_v)


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rotations, scales, means3D, viewmatrix, raw):
        from . import _capi
        dev = rotations.device
        P = int(rotations.shape[0])
        rot, sc, mean, view = (t.detach().contiguous() for t in (rotations, scales, means3D, viewmatrix))
        out = torch.empty((P, 3), dtype=torch.float32, device=dev)
        cx, stream = _capi.context_and_stream(dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(dev):
            cx.check(cx.lib.ggd_gaussian_normals(cx.handle, C.c_void_p(stream), P, p(rot), p(sc), p(mean), p(view), int(raw),
                                                 p(out)))
        ctx.save_for_backward(rot, sc, mean, view)
        ctx.raw = int(raw)
        return out

    @staticmethod
    def backward(ctx, grad_normals):
        from . import _capi
        rot, sc, mean, view = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        dev = rot.device
        P = int(rot.shape[0])
        g = grad_normals.contiguous()
        out = torch.empty((P, 4), dtype=torch.float32, device=dev)
        cx, stream = _capi.context_and_stream(dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(dev):
            cx.check(cx.lib.ggd_gaussian_normals_backward(cx.handle, C.c_void_p(stream), P, p(rot), p(sc), p(mean), p(view),
                                                          ctx.raw, p(g), p(out)))
        return out, None, None, None, None


def gaussian_normals(rotations, scales, means3D, viewmatrix, raw=False):
    """[P, 3] view-space normals of the Gaussians: per row, with k = argmin of `scales` (ties to the lowest index) and R the
    rotation matrix the rasterizer builds from the quaternion (w, x, y, z) -- used as given; raw=True: first normalised by the
    fused-activation rule q / max(|q|, 1e-12), and `scales` are the raw log-scales --
        n_v = R[:, k] . V[:3, :3],   p_v = mean . V[:3, :3] + V[3, :3],   n = -n_v if n_v . p_v > 0 else n_v,
    so that n faces the camera (n . p_v <= 0).  viewmatrix: the rasterizer's [4, 4] (or 16 values; world_view_transform).
    Differentiable in `rotations` only: the argmin and the facing sign are decisions, and the dependence on the means and the view
    matrix (through the sign alone) carries none.  Device float32 tensors: one HIP launch each way (csrc/ggd_normals.hip); CPU
    tensors: gaussian_normals_torch."""
    P = _normals_args(rotations, scales, means3D, viewmatrix, "gaussian_normals")
    if not rotations.is_cuda:
        return gaussian_normals_torch(rotations, scales, means3D, viewmatrix, raw)
    if rotations.dtype != torch.float32:
        raise TypeError(f"gaussian_normals: float32 tensors expected, got {rotations.dtype}")
    return _GaussianNormals.apply(rotations, scales, means3D, viewmatrix, bool(raw)) if P else rotations.new_zeros((0, 3))


def _loss_args(normals, depth, alpha, tanfovx, tanfovy, alpha_min, what, float32_only):
    """The three maps as contiguous [3,H,W], [H,W], [H,W] after the checks both forms share."""
    for name, t in (("depth", depth), ("alpha", alpha)):
        if t.dim() not in (2, 3) or (t.dim() == 3 and int(t.shape[0]) != 1):
            raise ValueError(f"{what}: {name} must be [H,W] or [1,H,W], got {tuple(t.shape)}")
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    if H <= 0 or W <= 0:
        raise ValueError(f"{what}: empty image")
    if tuple(alpha.shape[-2:]) != (H, W) or tuple(normals.shape) != (3, H, W):
        raise ValueError(f"{what}: normals [3,H,W], depth and alpha [H,W] of one size expected, got {tuple(normals.shape)}, "
                         f"{tuple(depth.shape)}, {tuple(alpha.shape)}")
    if not (float(tanfovx) > 0.0 and float(tanfovy) > 0.0):
        raise ValueError(f"{what}: tanfovx and tanfovy must be positive, got {tanfovx}, {tanfovy}")
    if not float(alpha_min) >= 0.0:
        raise ValueError(f"{what}: alpha_min must not be negative, got {alpha_min}")
    maps = (normals, depth, alpha)
    if any(t.dtype != (torch.float32 if float32_only else depth.dtype) for t in maps):
        raise TypeError(f"{what}: {'float32 tensors' if float32_only else 'tensors of one dtype'} expected, got "
                        f"{[t.dtype for t in maps]}")
    if any(t.device != depth.device for t in maps):
        raise RuntimeError(f"{what}: normals, depth and alpha must live on one device")
    return normals.contiguous(), depth.reshape(H, W).contiguous(), alpha.reshape(H, W).contiguous()


def normal_loss_torch(normals, depth, alpha, tanfovx, tanfovy, alpha_min=0.5):
    """fused_normal_loss as a torch expression in the tensors' own dtype and on their own device: the form CPU tensors take and, on
    device tensors, the ~30-launch composition the kernel is timed against.  Same arguments, same (total, surface_normals)."""
    N, Dm, A = _loss_args(normals, depth, alpha, tanfovx, tanfovy, alpha_min, "normal_loss_torch", False)
    H, W = Dm.shape
    surface = torch.zeros_like(N)
    if H < 3 or W < 3:
        return (N.sum() + Dm.sum() + A.sum()) * 0, surface
    ok = A.detach() > float(alpha_min)
    D = Dm / torch.where(ok, A, torch.ones_like(A))
    x = (2 * (torch.arange(W, dtype=D.dtype, device=D.device) + 0.5) / W - 1) * float(tanfovx)
    y = (2 * (torch.arange(H, dtype=D.dtype, device=D.device) + 0.5) / H - 1) * float(tanfovy)
    P = torch.stack([x[None, :] * D, y[:, None] * D, D])
    dU = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    dV = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    c = torch.cross(dV, dU, dim=0)
    valid = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1]
    len2 = (c * c).sum(0)
    nz = valid & (len2.detach() > 0)
    Ns = torch.where(nz, c / torch.sqrt(torch.where(nz, len2, torch.ones_like(len2))), torch.zeros_like(c))
    e = torch.where(valid, A[1:-1, 1:-1] - (N[:, 1:-1, 1:-1] * Ns).sum(0), torch.zeros_like(len2))
    surface[:, 1:-1, 1:-1] = Ns.detach()
    return e.sum() / (H * W), surface


class _FusedNormalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normals, depth, alpha, tanfovx, tanfovy, alpha_min):
        from . import _capi
        dev = depth.device
        H, W = (int(n) for n in depth.shape)
        cx, stream = _capi.context_and_stream(dev)
        nbytes = cx.lib.ggd_normal_loss_tmp_bytes(W, H)
        tmp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        term = torch.empty((1,), dtype=torch.float32, device=dev)
        grad_normals, surface = torch.empty_like(normals), torch.empty_like(normals)
        grad_depth, grad_alpha = torch.empty_like(depth), torch.empty_like(alpha)
        p = lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(dev):
            cx.check(cx.lib.ggd_normal_loss(cx.handle, C.c_void_p(stream), W, H, p(normals), p(depth), p(alpha), float(tanfovx),
                                            float(tanfovy), float(alpha_min), p(term), p(grad_normals), p(grad_depth),
                                            p(grad_alpha), p(surface), p(tmp), nbytes))
        ctx.save_for_backward(grad_normals, grad_depth, grad_alpha)
        ctx.mark_non_differentiable(surface)
        return term[0].clone(), surface

    @staticmethod
    def backward(ctx, g_total, _g_surface):
        grad_normals, grad_depth, grad_alpha = ctx.saved_tensors
        return grad_normals * g_total, grad_depth * g_total, grad_alpha * g_total, None, None, None


def fused_normal_loss(normals, depth, alpha, tanfovx, tanfovy, alpha_min=0.5):
    """(total, surface_normals [3,H,W]): the blended normal map `normals` = sum alpha_i T_i n_i ([3,H,W], unnormalised;
    out["normals"] of render_simple(..., render_normals=True)) against the normals of the surface that `depth` (sum alpha_i T_i z_i)
    and `alpha` ([H,W] or [1,H,W]; render_depth_alpha=True) describe.  With pixel centres x_j = (2 (j + 0.5) / W - 1) tanfovx,
    y_i = (2 (i + 0.5) / H - 1) tanfovy, ok = alpha > alpha_min, D = depth / alpha and P = (x D, y D, D), at every interior pixel
    whose own ok and its four axis neighbours' ok hold:
        dU = P(i, j+1) - P(i, j-1),  dV = P(i+1, j) - P(i-1, j),  N_s = dV x dU / |dV x dU|  (0 if the product vanishes),
        e = alpha - N_r . N_s;
    e = 0 and N_s = 0 everywhere else; total = sum e / (H W).  N_s faces the camera, as gaussian_normals does, so e >= 0 up to
    rounding and e = 0 exactly where every contributor's normal is the surface's; empty space contributes nothing.
    The gradients in all three maps are the exact derivative of this total -- nothing is detached (2DGS detaches the alpha factor),
    and the path through D into the neighbours' N_s is included.  surface_normals carries no gradient.
    Device float32 tensors: two HIP launches (csrc/ggd_imgloss.hip), one autograd node, bit-identical from run to run.  CPU tensors:
    normal_loss_torch.  ValueError: shapes, non-positive tanfov, negative alpha_min; TypeError: device tensors that are not float32;
    RuntimeError: tensors on different devices.
    alpha_min = 0.5 is an untuned placeholder: nobody has measured which threshold serves training best."""
    N, D, A = _loss_args(normals, depth, alpha, tanfovx, tanfovy, alpha_min, "fused_normal_loss", depth.is_cuda)
    if not depth.is_cuda:
        return normal_loss_torch(normals, depth, alpha, tanfovx, tanfovy, alpha_min)
    return _FusedNormalLoss.apply(N, D, A, tanfovx, tanfovy, alpha_min)


def depth_to_normal(depth, alpha, tanfovx, tanfovy, alpha_min=0.5):
    """The surface normals N_s [3,H,W] of fused_normal_loss alone (forward only, no gradient): camera-facing unit normals of the
    expected depth depth / alpha in view space, zero on the border and wherever a pixel or one of its four axis neighbours has
    alpha <= alpha_min (an untuned placeholder, as there)."""
    with torch.no_grad():
        H, W = int(depth.shape[-2]), int(depth.shape[-1])
        zeros = torch.zeros((3, H, W), dtype=depth.dtype, device=depth.device)
        return fused_normal_loss(zeros, depth, alpha, tanfovx, tanfovy, alpha_min)[1]
