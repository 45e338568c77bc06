"""TEST-ONLY PyTorch restatement of the masked image loss (the reference's --apply_mask_to_rendering,
main/train_pano2gaussian_decoder.py:237-261): bilinear upsample of the low-resolution mask (interpolate, align_corners=False,
integer factors), composite of image and target onto white, then L1 / L2 / 1 - SSIM / Sobel.  The checker of
losses.fused_image_loss(mask=) and losses.composite_mask, and the masked loss of the CPU trainer.  Works in float32 and in
float64 (the yardstick of the GPU tests): every constant follows the input dtype -- tests/_torch_losses.py's Sobel kernels are
float32-only, so the Sobel term is restated here.  Pinned by vectors from the reference's own functions
(tests/golden/masked_losses.npz).  Never imported by the product."""
import torch
import torch.nn.functional as F

import _torch_losses as TL

CASES = ("A", "B", "C", "D", "E")


def _axis(n_out, n_in, dtype, device):
    """Source cells and weight of one axis: src = max((dst + 0.5) / f - 0.5, 0), i0 = min(floor(src), n - 1),
    i1 = min(i0 + 1, n - 1), lambda = src - i0."""
    f = n_out // n_in
    dst = torch.arange(n_out, dtype=dtype, device=device)
    src = ((dst + 0.5) / f - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, src - i0.to(dtype)


def upsample_mask(mask, H, W):
    """mask [..., mh, mw] with leading ones -> [H, W] in the mask's dtype: along x for both rows, then along y."""
    m = mask.reshape(mask.shape[-2], mask.shape[-1])
    assert H % m.shape[0] == 0 and W % m.shape[1] == 0
    y0, y1, ly = _axis(H, m.shape[0], m.dtype, m.device)
    x0, x1, lx = _axis(W, m.shape[1], m.dtype, m.device)
    top = m[y0][:, x0] * (1 - lx) + m[y0][:, x1] * lx
    bot = m[y1][:, x0] * (1 - lx) + m[y1][:, x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def composite(x, m):
    """x [..., H, W] onto white in the reference's order."""
    return x * m + 1 - m


def sobel_loss(render, target):
    """main/loss_utils/sobel_loss.py:19-30 with kernels of the input's dtype."""
    kx = torch.tensor(TL._SOBEL_X, dtype=render.dtype, device=render.device).unsqueeze(0).expand(1, 3, 3, 3)
    ky = torch.tensor(TL._SOBEL_Y, dtype=render.dtype, device=render.device).unsqueeze(0).expand(1, 3, 3, 3)
    rx = F.conv2d(render.unsqueeze(0), kx, stride=1, padding=1)
    tx = F.conv2d(target.unsqueeze(0), kx, stride=1, padding=1)
    ry = F.conv2d(render.unsqueeze(0), ky, stride=1, padding=1)
    ty = F.conv2d(target.unsqueeze(0), ky, stride=1, padding=1)
    diff = torch.square(rx - tx) + torch.square(ry - ty)
    return diff.mean(), diff


def masked_image_loss_torch(image, target, l1_weight=0.2, l2_weight=0.1, ssim_weight=0.5, sobel_weight=0.2, mask=None):
    """(total, terms[4]) with the signature of losses.fused_image_loss; mask=None: the unmasked loss."""
    if mask is not None:
        m = upsample_mask(mask.detach().to(image.dtype), image.shape[-2], image.shape[-1])
        image, target = composite(image, m), composite(target, m)
    terms = torch.stack([TL.l1_loss(image, target), TL.l2_loss(image, target), 1.0 - TL.ssim(image, target)[0],
                         sobel_loss(image, target)[0]])
    w = torch.tensor([l1_weight, l2_weight, ssim_weight, sobel_weight], dtype=terms.dtype, device=terms.device)
    return (terms * w).sum(), terms
