"""Image losses of the decoder training step (main/train_pano2gaussian_decoder.py:246-261).

`fused_image_loss`: L1, L2, 1 - SSIM and the Sobel term (gaussian_splatting/utils/loss_utils.py:17-63,
main/loss_utils/sobel_loss.py:19-30) and d(loss)/d(image) in three HIP launches (csrc/ggd_imgloss.hip), as one autograd
node; pinned by vectors from the reference's own functions (tests/golden/losses.npz).  The PyTorch evaluation of the
same terms lives under tests/ (the checker).  With `mask=` the reference's --apply_mask_to_rendering
(main/train_pano2gaussian_decoder.py:237-241: the generator's mask upsampled bilinearly, image and target composited onto
white before every term) happens inside the same three launches.
`composite_mask`: that composite as an operator of its own, for what needs the composited image itself (the perceptual
term, logging, eval).
`fused_geometry_loss`: the rasterizer's differentiable depth and alpha maps against the teacher's depth and weight maps
(teacher.render_teacher) -- a mask term and a cross-multiplied depth term with both gradient maps in two HIP launches
(DESIGN.md section 6s); `geometry_loss_torch` is the same loss as a torch expression (CPU tensors, the timing baseline).
`PerceptualStandIn`: the slot of the reference's LPIPS term (main/loss_utils/lpips.py:6-34: VGG16 features of the image
and the target at 256 x 256, squared distance).  The pretrained VGG is an external download and out of scope; the
stand-in is a FIXED, seeded, random-initialised network of the same shape (VGG16's 13 3x3 convolutions, taps after
conv1_2 / 2_2 / 3_3 / 4_3 / 5_3, channel-normalised, per-channel weights), so that the training step carries the same
amount of convolution work and the same kind of gradient path into the rendered image.  It runs in PyTorch-ROCm (MIOpen)
like the reference's own VGG.  The identity term needs ArcFace and stays out.
`FusedPerceptual`: the same term on HIP kernels (csrc/ggd_perceptual.hip) -- NHWC activations, the twelve
convolutions behind conv1_1 and their backward-data passes as one implicit-GEMM MFMA kernel, pools, taps and the loss in a fixed
summation order; opt-in (DecoderTrainer(fused_perceptual=True)), two precision tiers like the fused decoder's.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F


def _mask_2d(mask, H, W, what, dtype=torch.float32):
    """The low-resolution mask as a contiguous float32 (`dtype`) [mh, mw]; ValueError unless its size divides the image's."""
    if mask.dim() not in (2, 3, 4) or any(int(n) != 1 for n in mask.shape[:-2]):
        raise ValueError(f"{what}: mask must be [mh,mw], [1,mh,mw] or [1,1,mh,mw], got {tuple(mask.shape)}")
    mh, mw = int(mask.shape[-2]), int(mask.shape[-1])
    if mh <= 0 or mw <= 0 or H % mh != 0 or W % mw != 0:
        raise ValueError(f"{what}: the mask size {mh} x {mw} must divide the image size {H} x {W}")
    return mask.detach().reshape(mh, mw).contiguous().to(dtype)


class _FusedImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, target, weights, mask):
        from . import _capi
        if not image.is_cuda:
            raise RuntimeError("fused_image_loss is a HIP kernel: HIP device tensors required (there is no CPU form in the package)")
        if image.dim() != 3 or image.shape[0] != 3 or image.shape != target.shape:
            raise ValueError("image and target must both be [3,H,W]")
        dev = image.device
        img = image.contiguous().float()
        tgt = target.contiguous().float()
        H, W = int(img.shape[1]), int(img.shape[2])
        if mask is not None and mask.device != dev:
            raise RuntimeError("fused_image_loss: the mask must live on the image's HIP device")
        cx = _capi.context_for(dev)
        nbytes = cx.lib.ggd_image_loss_tmp_bytes(W, H)
        tmp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        terms = torch.empty((5,), dtype=torch.float32, device=dev)
        grad = torch.empty_like(img)
        w4 = (C.c_float * 4)(*[float(x) for x in weights])
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        out = (w4, C.c_void_p(terms.data_ptr()), C.c_void_p(grad.data_ptr()), C.c_void_p(tmp.data_ptr()), nbytes)
        with torch.cuda.device(dev):
            if mask is None:
                cx.check(cx.lib.ggd_image_loss(cx.handle, stream, W, H, C.c_void_p(img.data_ptr()),
                                               C.c_void_p(tgt.data_ptr()), *out))
            else:
                cx.check(cx.lib.ggd_image_loss_masked(cx.handle, stream, W, H, C.c_void_p(img.data_ptr()),
                                                      C.c_void_p(tgt.data_ptr()), C.c_void_p(mask.data_ptr()),
                                                      int(mask.shape[1]), int(mask.shape[0]), *out))
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(terms)
        return terms[4].clone(), terms

    @staticmethod
    def backward(ctx, g_total, _g_terms):
        (grad,) = ctx.saved_tensors
        return grad * g_total, None, None, None


def fused_image_loss(image, target, l1_weight=0.2, l2_weight=0.1, ssim_weight=0.5, sobel_weight=0.2, mask=None):
    """(total, terms[5] = L1, L2, 1-SSIM, Sobel, total): same value and d/d(image) as the torch evaluation under tests/, three HIP
    launches instead of ~60 torch kernels.  `target` receives no gradient.
    mask (float32 device tensor [mh,mw], [1,mh,mw] or [1,1,mh,mw]; H % mh == 0 and W % mw == 0, else ValueError): the
    reference's --apply_mask_to_rendering -- m = the mask upsampled bilinearly (interpolate, align_corners=False) by H/mh,
    W/mw; image and target become x*m + 1 - m inside the same three launches; the terms are those of the composited pair,
    d/d(image) carries the factor m, and the mask receives no gradient (it comes out of a no_grad synthesis)."""
    if mask is not None:
        if image.dim() != 3:
            raise ValueError("image and target must both be [3,H,W]")
        mask = _mask_2d(mask, int(image.shape[1]), int(image.shape[2]), "fused_image_loss")
    return _FusedImageLoss.apply(image, target, (l1_weight, l2_weight, ssim_weight, sobel_weight), mask)


class _CompositeMask(torch.autograd.Function):
    """[C,H,W] device image, [mh,mw] device mask -> (image*m + 1) - m in one HIP launch; backward g*m in one launch."""

    @staticmethod
    def forward(ctx, image, mask):
        ctx.save_for_backward(mask)
        return _CompositeMask._launch(image, mask, 0)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return _CompositeMask._launch(g, mask, 1), None

    @staticmethod
    def _launch(src, mask, backward):
        from . import _capi
        dev = src.device
        src = src.contiguous().float()
        Cn, H, W = (int(n) for n in src.shape)
        dst = torch.empty_like(src)
        cx = _capi.context_for(dev)
        with torch.cuda.device(dev):
            cx.check(cx.lib.ggd_mask_composite(cx.handle, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), W, H, Cn,
                                               C.c_void_p(src.data_ptr()), C.c_void_p(mask.data_ptr()), int(mask.shape[1]),
                                               int(mask.shape[0]), backward, C.c_void_p(dst.data_ptr())))
        return dst


def composite_mask(image, mask):
    """image * m + 1 - m with m = `mask` upsampled bilinearly to the image (the reference's --apply_mask_to_rendering
    lines, main/train_pano2gaussian_decoder.py:239-241): the composited image itself, for the perceptual term, logging and
    eval (the loss terms take the mask directly: fused_image_loss(mask=)).  image [C,H,W] with a mask [mh,mw] / [1,mh,mw] /
    [1,1,mh,mw], or image [B,C,H,W] with such a mask (shared) or [B,1,mh,mw]; H % mh == 0 and W % mw == 0, else ValueError.
    Differentiable in `image` only.  Device tensors: the HIP kernel (one launch per mask); CPU tensors (the gloo trainer;
    not a hot path): the torch expression."""
    if image.dim() not in (3, 4):
        raise ValueError(f"composite_mask: image must be [C,H,W] or [B,C,H,W], got {tuple(image.shape)}")
    H, W = int(image.shape[-2]), int(image.shape[-1])
    B = int(image.shape[0]) if image.dim() == 4 else 1
    per_scene = image.dim() == 4 and mask.dim() == 4 and int(mask.shape[0]) == B and B > 1
    masks = [_mask_2d(mask[b:b + 1] if per_scene else mask, H, W, "composite_mask") for b in range(B if per_scene else 1)]
    if mask.device != image.device:
        raise RuntimeError("composite_mask: image and mask must live on the same device")
    if not image.is_cuda:
        m = torch.stack([F.interpolate(mk[None, None], scale_factor=(H // mk.shape[0], W // mk.shape[1]),
                                       mode="bilinear")[0] for mk in masks])         # [1 or B, 1, H, W]
        m = m if image.dim() == 4 else m[0]
        return image * m + 1 - m
    if not per_scene:      # one mask for everything: the batch folds into the channel axis of one launch
        return _CompositeMask.apply(image.reshape(-1, H, W), masks[0]).view(image.shape)
    return torch.stack([_CompositeMask.apply(image[b], masks[b]) for b in range(B)])


def _geometry_args(depth, alpha, teacher_depth, teacher_weights, tanfovx, tanfovy, what, float32_only):
    """The four maps as contiguous 2-D tensors ([H,W] twice, [th,tw] twice; the teacher's detached) after the checks both forms
    share: ValueError for shapes, a size that does not divide and a non-positive tanfov, TypeError for a dtype other than
    float32 (float32_only) or mixed dtypes, RuntimeError for tensors on different devices."""
    for name, t in (("depth", depth), ("alpha", alpha)):
        if t.dim() not in (2, 3) or (t.dim() == 3 and int(t.shape[0]) != 1):
            raise ValueError(f"{what}: {name} must be [H,W] or [1,H,W], got {tuple(t.shape)}")
    if tuple(depth.shape[-2:]) != tuple(alpha.shape[-2:]):
        raise ValueError(f"{what}: depth {tuple(depth.shape)} and alpha {tuple(alpha.shape)} must have one size")
    if not (float(tanfovx) > 0.0 and float(tanfovy) > 0.0):
        raise ValueError(f"{what}: tanfovx and tanfovy must be positive, got {tanfovx}, {tanfovy}")
    maps = (depth, alpha, teacher_depth, teacher_weights)
    if any(not torch.is_tensor(t) or t.dtype != (torch.float32 if float32_only else depth.dtype) for t in maps):
        raise TypeError(f"{what}: {'float32 tensors' if float32_only else 'tensors of one dtype'} expected, got "
                        f"{[getattr(t, 'dtype', type(t)) for t in maps]}")
    if any(t.device != depth.device for t in maps):
        raise RuntimeError(f"{what}: depth, alpha and the teacher's maps must live on one device")
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    if H <= 0 or W <= 0:
        raise ValueError(f"{what}: empty image")
    if tuple(teacher_depth.shape[-2:]) != tuple(teacher_weights.shape[-2:]):
        raise ValueError(f"{what}: the teacher's depth {tuple(teacher_depth.shape)} and weights "
                         f"{tuple(teacher_weights.shape)} must have one size")
    t, w = (_mask_2d(m, H, W, what, depth.dtype) for m in (teacher_depth, teacher_weights))
    return depth.reshape(H, W).contiguous(), alpha.reshape(H, W).contiguous(), t, w


def geometry_loss_torch(depth, alpha, teacher_depth, teacher_weights, tanfovx, tanfovy, mask_weight=1.0, depth_weight=1.0,
                        ray_depth=True):
    """fused_geometry_loss as a torch expression in the tensors' own dtype and on their own device: the form CPU tensors take
    (the gloo trainer, the host tests; float64 for gradcheck) and, on device tensors, the ~20-launch composition the kernel is
    timed against.  Not a hot path.  Same arguments, same (total, terms[3]); differentiable in depth and alpha only."""
    D, A, t, w = _geometry_args(depth, alpha, teacher_depth, teacher_weights, tanfovx, tanfovy, "geometry_loss_torch", False)
    (H, W), (th, tw) = D.shape, t.shape
    z = t
    if ray_depth:
        xl = (2 * (torch.arange(tw, dtype=t.dtype, device=t.device) + 0.5) / tw - 1) * float(tanfovx)
        yl = (2 * (torch.arange(th, dtype=t.dtype, device=t.device) + 0.5) / th - 1) * float(tanfovy)
        z = t / torch.sqrt(1 + xl[None, :] ** 2 + yl[:, None] ** 2)
    up = lambda v: F.interpolate(v[None, None], scale_factor=(H // th, W // tw), mode="bilinear")[0, 0]
    m, q = up(w), up(w * z)
    l_mask = (A - m).abs().mean()
    l_depth = (m * D - A * q).abs().mean()
    total = float(mask_weight) * l_mask + float(depth_weight) * l_depth
    return total, torch.stack([l_mask, l_depth, total]).detach()


class _FusedGeometryLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, t, w, tanfovx, tanfovy, weights, ray_depth):
        from . import _capi
        dev = depth.device
        H, W = (int(n) for n in depth.shape)
        cx = _capi.context_for(dev)
        nbytes = cx.lib.ggd_geometry_loss_tmp_bytes(W, H)
        tmp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        terms = torch.empty((3,), dtype=torch.float32, device=dev)
        grad_depth, grad_alpha = torch.empty_like(depth), torch.empty_like(alpha)
        w2 = (C.c_float * 2)(*[float(x) for x in weights])
        p = lambda x: C.c_void_p(x.data_ptr())
        with torch.cuda.device(dev):
            cx.check(cx.lib.ggd_geometry_loss(cx.handle, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), W, H, p(depth),
                                              p(alpha), p(t), p(w), int(t.shape[1]), int(t.shape[0]), float(tanfovx),
                                              float(tanfovy), int(bool(ray_depth)), w2, p(terms), p(grad_depth), p(grad_alpha),
                                              p(tmp), nbytes))
        ctx.save_for_backward(grad_depth, grad_alpha)
        ctx.mark_non_differentiable(terms)
        return terms[2].clone(), terms

    @staticmethod
    def backward(ctx, g_total, _g_terms):
        grad_depth, grad_alpha = ctx.saved_tensors
        return grad_depth * g_total, grad_alpha * g_total, None, None, None, None, None, None


def fused_geometry_loss(depth, alpha, teacher_depth, teacher_weights, tanfovx, tanfovy, mask_weight=1.0, depth_weight=1.0,
                        ray_depth=True):
    """(total, terms[3] = L_mask, L_depth, total): the student's `depth` (sum alpha_i T_i z_i) and `alpha` (1 - final T) renders
    -- render_simple(..., render_depth_alpha=True); float32 [H,W] or [1,H,W] -- against the teacher's depth t and weights w
    (teacher.TeacherRender.geometry; float32 [th,tw], leading 1-axes allowed, H % th == 0 and W % tw == 0):
      z = t / sqrt(1 + xl^2 + yl^2), xl = (2 (j + 0.5) / tw - 1) tanfovx, yl = (2 (i + 0.5) / th - 1) tanfovy   (ray_depth: t is a
          distance along a unit ray, the rasterizer's depth is view-space z; ray_depth=False: z = t);
      m = up(w), q = up(w z): the masked image loss's bilinear upsample (interpolate, align_corners=False) -- the teacher's depth
          is clamped garbage where w ~ 0, so only the premultiplied depth is interpolated;
      L_mask = mean |A - m|,  L_depth = mean |m D - A q|,  total = mask_weight L_mask + depth_weight L_depth.
    The depth residual is cross-multiplied: zero exactly where the expected depths D / A and q / m agree, no division (bounded
    gradients at low opacity), zero where the teacher sees nothing.  Differentiable in depth and alpha only; the teacher's maps
    come out of a no_grad synthesis.  Precondition (not checked): t is finite (render_teacher clamps it).
    Device tensors: two HIP launches (csrc/ggd_imgloss.hip), one autograd node, bit-identical from run to run.  CPU tensors:
    geometry_loss_torch.  ValueError: shapes, a size that does not divide, non-positive tanfov; TypeError: tensors that are not
    float32; RuntimeError: tensors on different devices.
    The default weights (1, 1) are placeholders: nobody has tuned them."""
    D, A, t, w = _geometry_args(depth, alpha, teacher_depth, teacher_weights, tanfovx, tanfovy, "fused_geometry_loss", True)
    if not depth.is_cuda:
        return geometry_loss_torch(depth, alpha, teacher_depth, teacher_weights, tanfovx, tanfovy, mask_weight, depth_weight,
                                   ray_depth)
    total, terms = _FusedGeometryLoss.apply(D, A, t, w, tanfovx, tanfovy, (mask_weight, depth_weight), ray_depth)
    return total, terms


class PerceptualStandIn(torch.nn.Module):
    """perc(target, image) of main/loss_utils/lpips.py:16-34 with a fixed random VGG16-shaped trunk (see the module
    docstring).  forward(image [3,H,W] or [B,3,H,W] in [0,1], target likewise) -> scalar (summed over the batch, as the
    reference evaluates the whole batch in one VGG call); gradients flow into `image` only."""
    CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512)
    TAPS = (1, 3, 6, 9, 12)       # index of the convolution after whose ReLU a feature map is taken

    def __init__(self, seed: int = 1234, width_div: int = 1):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        convs, cin = [], 3
        for v in self.CFG:
            if v == "M":
                continue
            cout = max(4, v // width_div)
            conv = torch.nn.Conv2d(cin, cout, 3, padding=1)
            with torch.no_grad():   # He initialisation keeps the activations O(1) through the 13 layers
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * cin)) ** 0.5)
                conv.bias.zero_()
            convs.append(conv)
            cin = cout
        self.convs = torch.nn.ModuleList(convs)
        self.lin = torch.nn.ParameterList([torch.nn.Parameter(torch.rand(self.convs[t].out_channels, generator=g))
                                           for t in self.TAPS])
        self.requires_grad_(False)

    def features(self, img):
        x = ((img if img.dim() == 4 else img.unsqueeze(0)) * 2.0 - 1.0)
        if x.shape[2] > 256:
            x = F.interpolate(x, size=(256, 256), mode="area")     # lpips.py:23-26
        feats, ci = [], 0
        for v in self.CFG:
            if v == "M":
                x = F.max_pool2d(x, 2)
                continue
            x = F.relu(self.convs[ci](x))
            if ci in self.TAPS:
                k = self.TAPS.index(ci)
                n = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
                feats.append((n * (self.lin[k] / (x.shape[2] * x.shape[3])).sqrt()[None, :, None, None]).flatten(1))
            ci += 1
        return torch.cat(feats, 1)

    def forward(self, image, target):
        with torch.no_grad():
            ft = self.features(target)
        return (self.features(image) - ft).square().sum()


# ---- the perceptual term on the device (csrc/ggd_perceptual.hip) ------------------------------------------------------------
_PERC_POOLS_AFTER = (1, 3, 6, 9)      # a 2x2 max pool follows these convolutions (PerceptualStandIn.CFG)
_PERC_FORMATS = {"f16": torch.float16, "bf16": torch.bfloat16, "split": torch.bfloat16}


def pack_conv_weights(weight, fmt):
    """weight [Cout, Cin, 3, 3] (Cin a multiple of 32) -> the image ggd_perceptual_* reads: [9 Cin / 32 K steps][parts][Cout' / 16
    tiles][64 lanes][8], Cout' = Cout rounded up to 64 (zero columns); K step = tap (ky * 3 + kx) * (Cin / 32) + channel chunk, lane
    l of tile t holds k = 8 (l >> 4) + j of the chunk for output channel 16 t + (l & 15): the A operand of
    v_mfma_f32_16x16x32.  fmt "f16" / "bf16": one part in that format; "split": two bf16 parts, hi = bf16(w), lo = bf16(w - hi)."""
    if fmt not in _PERC_FORMATS:
        raise ValueError(f"pack_conv_weights: fmt must be one of {tuple(_PERC_FORMATS)} (got {fmt!r})")
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or cin % 32 != 0:
        raise ValueError(f"pack_conv_weights: [Cout, Cin, 3, 3] with Cin a multiple of 32 expected, got {tuple(weight.shape)}")
    pad = -cout % 64
    w = F.pad(weight.detach().float().permute(2, 3, 1, 0).reshape(9, cin, cout), (0, pad))          # [tap][ci][co']
    tiles = (cout + pad) // 16
    w = w.reshape(9, cin // 32, 4, 8, tiles, 16).permute(0, 1, 4, 2, 5, 3).reshape(9 * cin // 32, 1, tiles, 64, 8)
    if fmt == "split":
        hi = w.to(torch.bfloat16)
        return torch.cat([hi, (w - hi.float()).to(torch.bfloat16)], 1).contiguous()
    return w.to(_PERC_FORMATS[fmt]).contiguous()


def unpack_conv_weights(packed, cout, cin):
    """The inverse of pack_conv_weights, as float32 [cout, cin, 3, 3] (the sum of the parts)."""
    tiles = int(packed.shape[2])
    w = packed.float().sum(1).reshape(9, cin // 32, tiles, 4, 16, 8).permute(0, 1, 3, 5, 2, 4).reshape(9, cin, tiles * 16)
    return w[:, :, :cout].reshape(3, 3, cin, cout).permute(3, 2, 0, 1).contiguous()


class _FusedPerceptualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, target, owner):
        loss, grad = owner._launch_loss(image, target, ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


class FusedPerceptual(torch.nn.Module):
    """PerceptualStandIn.forward(image, target) -> scalar on the HIP kernels of csrc/ggd_perceptual.hip:
    same definition, summed over the batch, gradient into `image` only, no float atomics, bit-identical from run to run.
    module: a PerceptualStandIn or anything of its shape -- 13 `convs` (3x3, padding 1), 5 `lin` vectors, pools and taps at the
        stand-in's places; its weights are packed once (`repack()` re-reads them).
    precision: "bf16" -- f16 operands forward, bf16 operands backward, fp32 accumulation; "fp32" -- split-bf16 operands (three
        MFMAs per product) both ways.
    max_size: a side above it is area-averaged down to it (the reference's 256; an integer factor only).
    input_affine: (scale[3], shift[3]) applied to the image before the trunk; default (2, -1), the stand-in's img * 2 - 1.
    Device tensors take the kernels, CPU tensors the wrapped module (which knows neither max_size nor input_affine).
    ValueError, before any native call: a module of another shape; a width that is not a multiple of 32 (or above 512; the first
    above 64); H or W that is not a multiple of 16; a side above max_size that is not a multiple of it."""
    TAPS = PerceptualStandIn.TAPS

    def __init__(self, module, precision="fp32", max_size=256, input_affine=None):
        super().__init__()
        from . import _capi
        if precision not in _capi.PERC_TIERS:
            raise ValueError(f"FusedPerceptual: precision must be 'fp32' or 'bf16' (got {precision!r})")
        self.widths = self._check_module(module)
        if int(max_size) <= 0 or int(max_size) % 16 != 0:
            raise ValueError(f"FusedPerceptual: max_size must be a positive multiple of 16 (got {max_size})")
        scale, shift = ((2.0, 2.0, 2.0), (-1.0, -1.0, -1.0)) if input_affine is None else input_affine
        scale, shift = [float(v) for v in scale], [float(v) for v in shift]
        if len(scale) != 3 or len(shift) != 3:
            raise ValueError("FusedPerceptual: input_affine must be (scale[3], shift[3])")
        self.module, self.precision, self.max_size, self.input_affine = module, precision, int(max_size), (scale, shift)
        self._packed = None

    @staticmethod
    def _check_module(module):
        convs, lin = getattr(module, "convs", None), getattr(module, "lin", None)
        if convs is None or lin is None or len(convs) != 13 or len(lin) != 5:
            raise ValueError("FusedPerceptual: the module must have 13 `convs` and 5 `lin` vectors")
        if tuple(getattr(module, "TAPS", PerceptualStandIn.TAPS)) != PerceptualStandIn.TAPS or \
                [v == "M" for v in getattr(module, "CFG", PerceptualStandIn.CFG)] != [v == "M" for v in PerceptualStandIn.CFG]:
            raise ValueError("FusedPerceptual: pools and taps must sit at PerceptualStandIn's places")
        cin, widths = 3, []
        for i, conv in enumerate(convs):
            w = getattr(conv, "weight", None)
            if w is None or w.dim() != 4 or tuple(w.shape[1:]) != (cin, 3, 3) or getattr(conv, "bias", None) is None or \
                    tuple(getattr(conv, "padding", (1, 1))) != (1, 1) or tuple(getattr(conv, "stride", (1, 1))) != (1, 1):
                raise ValueError(f"FusedPerceptual: convs[{i}] must be a biased 3x3 convolution, padding 1, of {cin} channels")
            cin = int(w.shape[0])
            widths.append(cin)
        for k, t in enumerate(PerceptualStandIn.TAPS):
            if tuple(lin[k].shape) != (widths[t],):
                raise ValueError(f"FusedPerceptual: lin[{k}] must have {widths[t]} entries")
        if any(w % 32 != 0 or w > 512 for w in widths) or widths[0] > 64:
            raise ValueError(f"FusedPerceptual: every width must be a multiple of 32 up to 512 (the first up to 64), got {widths}")
        return widths

    def trunk_size(self, H, W):
        """(H', W') at which the trunk runs an H x W input; the refusals of the class docstring."""
        H, W = int(H), int(W)
        if H > self.max_size:           # the stand-in's rule (lpips.py:23-26): decided by the height, both sides resized
            if H % self.max_size != 0 or W % self.max_size != 0:
                raise ValueError(f"FusedPerceptual: a side above max_size = {self.max_size} must be a multiple of it, got {H} x {W}")
            H = W = self.max_size
        if H <= 0 or W <= 0 or H % 16 != 0 or W % 16 != 0:
            raise ValueError(f"FusedPerceptual: H and W must be multiples of 16 (four 2x2 pools), got {H} x {W}")
        return H, W

    def _batch(self, img, what):
        x = img if img.dim() == 4 else img.unsqueeze(0)
        if x.dim() != 4 or int(x.shape[1]) != 3 or int(x.shape[0]) == 0:
            raise ValueError(f"FusedPerceptual: {what} must be [3,H,W] or [B,3,H,W], got {tuple(img.shape)}")
        return x, self.trunk_size(x.shape[2], x.shape[3])

    def repack(self, device=None):
        """Re-read the module's weights into the kernels' images (on `device`, default: the module's)."""
        m = self.module
        dev = torch.device(device) if device is not None else m.convs[0].weight.device
        fwd, bwd = ("f16", "bf16") if self.precision == "bf16" else ("split", "split")
        w = [c.weight.detach().to(dev, torch.float32) for c in m.convs]
        self._packed = dict(
            device=dev,
            w0=w[0].permute(2, 3, 1, 0).reshape(27, -1).contiguous(),
            w0_t=w[0].permute(2, 3, 0, 1).reshape(9, -1, 3).contiguous(),
            bias=[c.bias.detach().to(dev, torch.float32).contiguous() for c in m.convs],
            w_fwd=[None] + [pack_conv_weights(x, fwd) for x in w[1:]],
            w_bwd=[None] + [pack_conv_weights(x.flip(2, 3).transpose(0, 1), bwd) for x in w[1:]],
            lin=[p.detach().to(dev, torch.float32).contiguous() for p in m.lin])
        return self

    def _desc(self, B, H_in, W_in, H, W, dev):
        from . import _capi
        if self._packed is None or self._packed["device"] != dev:
            self.repack(dev)
        pk, d = self._packed, _capi.PerceptualDesc()
        d.tier, d.B, d.H_in, d.W_in, d.H, d.W = _capi.PERC_TIERS[self.precision], B, H_in, W_in, H, W
        d.widths[:] = self.widths
        d.scale[:], d.shift[:] = self.input_affine
        d.w0, d.w0_t = pk["w0"].data_ptr(), pk["w0_t"].data_ptr()
        for l in range(13):
            d.bias[l] = pk["bias"][l].data_ptr()
            d.w_fwd[l] = pk["w_fwd"][l].data_ptr() if l else None
            d.w_bwd[l] = pk["w_bwd"][l].data_ptr() if l else None
        for k in range(5):
            d.lin[k] = pk["lin"][k].data_ptr()
        return d

    def _launch_loss(self, image, target, with_grad):
        from . import _capi
        dev = image.device
        img, tgt = image.detach().contiguous().float(), target.detach().contiguous().float()
        B, _, H_in, W_in = (int(n) for n in img.shape)
        H, W = self.trunk_size(H_in, W_in)
        d = self._desc(B, H_in, W_in, H, W, dev)
        cx = _capi.context_for(dev)
        nbytes = cx.lib.ggd_perceptual_tmp_bytes(C.byref(d), 2 * B, int(with_grad))
        if nbytes == 0:
            raise ValueError("FusedPerceptual: ggd_perceptual_tmp_bytes refuses this shape")
        tmp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        grad = torch.empty_like(img) if with_grad else None
        with torch.cuda.device(dev):
            cx.check(cx.lib.ggd_perceptual_loss(cx.handle, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.byref(d),
                                                C.c_void_p(img.data_ptr()), C.c_void_p(tgt.data_ptr()), C.c_void_p(loss.data_ptr()),
                                                C.c_void_p(grad.data_ptr()) if with_grad else None, C.c_void_p(tmp.data_ptr()), nbytes))
        return loss[0].clone(), (grad if with_grad else torch.zeros((), device=dev))

    def features(self, img):
        """[B, F] rows as PerceptualStandIn.features returns them (no gradient on the device path)."""
        x, (H, W) = self._batch(img, "img")
        if not x.is_cuda:
            return self.module.features(img)
        from . import _capi
        dev = x.device
        x = x.detach().contiguous().float()
        B, _, H_in, W_in = (int(n) for n in x.shape)
        d = self._desc(B, H_in, W_in, H, W, dev)
        cx = _capi.context_for(dev)
        nbytes = cx.lib.ggd_perceptual_tmp_bytes(C.byref(d), B, 0)
        tmp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        n_feat = sum(self.widths[t] * (H >> k) * (W >> k) for k, t in enumerate(self.TAPS))
        feat = torch.empty((B, n_feat), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            cx.check(cx.lib.ggd_perceptual_features(cx.handle, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), C.byref(d),
                                                    C.c_void_p(x.data_ptr()), C.c_void_p(feat.data_ptr()), C.c_void_p(tmp.data_ptr()),
                                                    nbytes))
        return feat

    def forward(self, image, target):
        x, size = self._batch(image, "image")
        t, size_t = self._batch(target, "target")
        if tuple(x.shape) != tuple(t.shape):
            raise ValueError(f"FusedPerceptual: image {tuple(image.shape)} and target {tuple(target.shape)} must have one shape")
        if x.device != t.device:
            raise RuntimeError("FusedPerceptual: image and target must live on one device")
        if not x.is_cuda:
            return self.module(image, target)
        return _FusedPerceptualFn.apply(x, t, self)
