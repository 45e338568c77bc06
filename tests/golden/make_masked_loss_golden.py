"""Generate tests/golden/masked_losses.npz by IMPORTING the reference's loss functions in this container (CPU), as
make_loss_golden.py does, and applying the three lines of --apply_mask_to_rendering in front of them
(main/train_pano2gaussian_decoder.py:239-241):
  rescale_mask = torch.nn.functional.interpolate(mask, scale_factor=(fy, fx), mode="bilinear")[0]
  image  = image  * rescale_mask + 1 - rescale_mask
  target = target * rescale_mask + 1 - rescale_mask
Per case: image, target, the low-resolution mask, the upsampled mask, the four terms + total, the gradient (all from the
float32 evaluation), and the float32 evaluation's own deviation from the same functions run in float64 (dev_terms: absolute,
per term; dev_grad: largest absolute deviation of the gradient) -- the tests derive their bounds from it.  Only arrays travel.
Run:  python tests/golden/make_masked_loss_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "gaussian_splatting"))
sys.path.insert(0, os.path.join(REF, "main"))

_tensor = torch.tensor
def _tensor_cpu(*a, **k):
    k.pop("device", None)
    return _tensor(*a, **k)
torch.tensor = _tensor_cpu
from utils.loss_utils import l1_loss, l2_loss, ssim          # noqa: E402
import loss_utils.sobel_loss as sobel_mod                     # noqa: E402
torch.tensor = _tensor

# tag: (H, W, mask_h, mask_w)
CASES = {"A": (40, 56, 5, 7),      # x8: partial 32-pixel tiles, clamping at both ends of each axis
         "B": (96, 96, 12, 12),    # x8: a centre tile whose halo lies wholly inside the image
         "C": (24, 40, 6, 5),      # unequal factors 4 and 8
         "D": (6, 10, 3, 5),       # x2: smaller than the 11-tap window and than one tile
         "E": (33, 70, 33, 70)}    # factor 1, odd sizes: the mask is used as given


def evaluate(img, tgt, mask, dtype):
    """The reference's masked loss and its gradient in `dtype` (its Sobel kernels are module-level float32 tensors)."""
    k32 = sobel_mod.sobel_kernel_x, sobel_mod.sobel_kernel_y
    sobel_mod.sobel_kernel_x, sobel_mod.sobel_kernel_y = k32[0].to(dtype), k32[1].to(dtype)
    try:
        image = img.detach().to(dtype).clone().requires_grad_(True)
        target, m = tgt.to(dtype), mask.to(dtype)
        H, W = image.shape[1:]
        rescale_mask = F.interpolate(m[None, None], scale_factor=(H // m.shape[0], W // m.shape[1]), mode="bilinear")[0]
        im = image * rescale_mask + 1 - rescale_mask
        tg = target * rescale_mask + 1 - rescale_mask
        l1, l2 = l1_loss(im, tg), l2_loss(im, tg)
        s, _ = ssim(im, tg)
        sb, _ = sobel_mod.sobel_loss(im, tg)
        total = 0.2 * l1 + 0.1 * l2 + 0.5 * (1.0 - s) + 0.2 * sb   # train_pano2gaussian_decoder.py:36-40,261
        total.backward()
        terms = np.array([l1.item(), l2.item(), (1.0 - s).item(), sb.item(), total.item()], np.float64)
        return terms, image.grad.numpy(), rescale_mask[0].numpy()
    finally:
        sobel_mod.sobel_kernel_x, sobel_mod.sobel_kernel_y = k32


def main():
    g = torch.Generator().manual_seed(43)
    out = {}
    for tag, (H, W, mh, mw) in CASES.items():
        tgt = torch.rand(3, H, W, generator=g)
        img = (tgt + 0.15 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
        mask = torch.rand(mh, mw, generator=g)
        mask[:2, :2] = 0.0       # the upsampled mask then has an exact-0 and an exact-1 region
        mask[-2:, -2:] = 1.0
        t32, g32, up32 = evaluate(img, tgt, mask, torch.float32)
        t64, g64, _ = evaluate(img, tgt, mask, torch.float64)
        out.update({f"{tag}_image": img.numpy(), f"{tag}_target": tgt.numpy(), f"{tag}_mask": mask.numpy(),
                    f"{tag}_upmask": up32, f"{tag}_terms": t32, f"{tag}_grad": g32,
                    f"{tag}_dev_terms": np.abs(t32 - t64), f"{tag}_dev_grad": np.array(np.abs(g32 - g64).max())})
        print(tag, "terms", t32, "\n  relative deviation from float64: terms", np.abs(t32 - t64) / np.abs(t64),
              "gradient / max|g|", np.abs(g32 - g64).max() / np.abs(g64).max(),
              " exact 0 / 1 pixels of the upsampled mask:", int((up32 == 0).sum()), int((up32 == 1).sum()))
    np.savez_compressed(os.path.join(HERE, "masked_losses.npz"), **out)
    print("wrote masked_losses.npz", {k: v.shape for k, v in out.items() if k.startswith("A_")})


if __name__ == "__main__":
    main()
