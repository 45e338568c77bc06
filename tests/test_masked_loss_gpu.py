"""Masked image loss (the reference's --apply_mask_to_rendering) on the GPU: losses.fused_image_loss(mask=) and
losses.composite_mask against the float64 torch restatement (tests/_masked_loss_ref.py) on the cases of
tests/golden/masked_losses.npz, and DecoderTrainer(apply_mask_to_rendering=True) against the oracle-backed CPU trainer."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import losses as L
import _masked_loss_ref as MR

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masked_losses.npz"))
W4 = dict(l1_weight=0.2, l2_weight=0.1, ssim_weight=0.5, sobel_weight=0.2)
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _float64(tag):
    """(terms[5], gradient, upsampled mask) of the float64 restatement, computed once per case."""
    img = torch.from_numpy(GOLD[f"{tag}_image"]).double().requires_grad_(True)
    tgt, mask = torch.from_numpy(GOLD[f"{tag}_target"]).double(), torch.from_numpy(GOLD[f"{tag}_mask"]).double()
    total, terms = MR.masked_image_loss_torch(img, tgt, mask=mask, **W4)
    total.backward()
    up = MR.upsample_mask(mask, img.shape[1], img.shape[2])
    return np.append(terms.detach().numpy(), total.item()), img.grad.numpy(), up.numpy()


def _load(tag):
    return [torch.from_numpy(GOLD[f"{tag}_{k}"]).to(DEV) for k in ("image", "target", "mask")]


@pytest.mark.parametrize("tag", MR.CASES)
def test_masked_loss_matches_float64(native_lib, tag):
    """Terms and gradient against the float64 restatement.  Bound per quantity: the larger of the project's bar for the
    unmasked loss (tests/test_losses.py: terms rtol 2e-6 + atol 1e-7, gradient 1e-5 of its maximum) and 4 x the deviation
    of the float32 REFERENCE evaluation from float64 stored with the case (compositing onto white leaves flat regions where
    1 - SSIM is a small difference of near-equal sums, so the float32 reference is itself up to 1e-5 off there; the factor
    4: the kernel sums tile partials through float atomics, in another order than torch's tree)."""
    img, tgt, mask = _load(tag)
    img.requires_grad_(True)
    total, terms = L.fused_image_loss(img, tgt, mask=mask, **W4)
    (3.0 * total).backward()
    t64, g64, _ = _float64(tag)
    got = terms.cpu().numpy().astype(np.float64)
    err = np.abs(got - t64)
    bound = np.maximum(2e-6 * np.abs(t64) + 1e-7, 4.0 * GOLD[f"{tag}_dev_terms"])
    gerr = float(np.abs(img.grad.cpu().numpy() - 3.0 * g64).max())
    gbound = 3.0 * max(1e-5 * np.abs(g64).max(), 4.0 * float(GOLD[f"{tag}_dev_grad"]))
    print(f"\n  case {tag}: relative term errors (L1, L2, 1-SSIM, Sobel, total) {np.array2string(err / np.abs(t64), precision=2)}"
          f" of bounds {np.array2string(bound / np.abs(t64), precision=2)}; gradient error / max|g| "
          f"{gerr / (3.0 * np.abs(g64).max()):.2e} of bound {gbound / (3.0 * np.abs(g64).max()):.2e}")
    assert float(total) == float(terms[4])
    assert (err <= bound).all(), (err, bound)
    assert gerr <= gbound, (gerr, gbound)


@pytest.mark.parametrize("tag", MR.CASES)
def test_composite_mask_matches_torch_on_the_device(native_lib, tag):
    """Forward and backward within 1e-6 absolute of the reference's expression evaluated by torch on the same device (values
    in [0, 2], six roundings of at most 2^-23 each), for [C,H,W] and for [B,C,H,W] with a shared and a per-image mask."""
    img, tgt, mask = _load(tag)
    H, W = img.shape[1:]
    scale = (H // mask.shape[0], W // mask.shape[1])

    def ref(x, m4):
        rescale_mask = F.interpolate(m4, scale_factor=scale, mode="bilinear")
        rescale_mask = rescale_mask[0] if x.dim() == 3 else rescale_mask
        return x * rescale_mask + 1 - rescale_mask

    masks = torch.stack([mask[None], 1.0 - mask[None]])
    batch = torch.stack([img, tgt])
    g3, g4 = torch.rand_like(img), torch.rand_like(batch)
    for x, m, m4, g in ((img, mask, mask[None, None], g3), (img, mask[None, None], mask[None, None], g3),
                        (batch, mask, mask[None, None], g4), (batch, masks, masks, g4)):
        a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        mg = m.clone().requires_grad_(True)
        out, want = L.composite_mask(a, mg), ref(b, m4)
        assert out.shape == want.shape and float((out - want).abs().max()) <= 1e-6
        (out * g).sum().backward()
        (want * g).sum().backward()
        assert float((a.grad - b.grad).abs().max()) <= 1e-6 and mg.grad is None
    up = torch.from_numpy(_float64(tag)[2]).to(DEV)
    assert float((L.composite_mask(torch.zeros_like(img), mask) - (1.0 - up)).abs().max()) <= 1e-6


@pytest.mark.parametrize("tag", MR.CASES)
def test_gradient_masking_is_exact(native_lib, tag):
    """image.grad is exactly 0 wherever the upsampled mask is exactly 0 and non-zero somewhere it is positive; target and mask
    receive no gradient even when they ask for one."""
    img, tgt, mask = (t.requires_grad_(True) for t in _load(tag))
    total, _ = L.fused_image_loss(img, tgt, mask=mask, **W4)
    total.backward()
    up = torch.from_numpy(GOLD[f"{tag}_upmask"]).to(DEV)
    zero = (up == 0)[None].expand_as(img)
    assert zero.any() and bool((img.grad[zero] == 0.0).all())
    assert bool((img.grad[~zero] != 0.0).any()) and bool(torch.isfinite(img.grad).all())
    assert tgt.grad is None and mask.grad is None


def test_all_ones_mask_at_factor_one_is_the_unmasked_loss(native_lib):
    """Terms within rtol 2e-6 and gradient within 1e-5 of its maximum of the unmasked call.  Not bit-identical: the composite
    (x*1 + 1) - 1 rounds x to the spacing of floats in [1, 2) (2^-23), so x' is not x in float32."""
    img, tgt, _ = _load("E")
    a, b = img.clone().requires_grad_(True), img.clone().requires_grad_(True)
    ta, terms_a = L.fused_image_loss(a, tgt, mask=torch.ones(img.shape[1:], device=DEV), **W4)
    tb, terms_b = L.fused_image_loss(b, tgt, **W4)
    ta.backward(); tb.backward()
    np.testing.assert_allclose(terms_a.cpu().numpy(), terms_b.cpu().numpy(), rtol=2e-6)
    assert float((a.grad - b.grad).abs().max()) <= 1e-5 * float(b.grad.abs().max())


def test_c_abi_rejects_bad_arguments(native_lib):
    """GGD_E_INVALID (through ggd_fail, so the context carries a message) for a NULL pointer, an empty size and a mask size
    that does not divide the image; nothing is launched."""
    from gaussian_gan_decoder_amd import _capi
    cx = _capi.context_for(DEV)
    img, tgt, mask = _load("D")                    # 6 x 10, mask 3 x 5
    H, W = img.shape[1:]
    nbytes = cx.lib.ggd_image_loss_tmp_bytes(W, H)
    tmp = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    terms, grad = torch.zeros(5, device=DEV), torch.zeros_like(img)
    w4 = (C.c_float * 4)(0.2, 0.1, 0.5, 0.2)
    p = lambda t: C.c_void_p(t.data_ptr())

    def loss(W_, H_, m, mw, mh):
        return cx.lib.ggd_image_loss_masked(cx.handle, None, W_, H_, p(img), p(tgt), m, mw, mh, w4, p(terms), p(grad), p(tmp), nbytes)

    def comp(W_, H_, ch, m, mw, mh):
        return cx.lib.ggd_mask_composite(cx.handle, None, W_, H_, ch, p(img), m, mw, mh, 0, p(grad))
    for rc in (loss(W, H, None, 5, 3), loss(0, H, p(mask), 5, 3), loss(W, H, p(mask), 0, 3), loss(W, H, p(mask), 4, 3),
               loss(W, H, p(mask), 5, 4), comp(W, H, 3, None, 5, 3), comp(W, 0, 3, p(mask), 5, 3), comp(W, H, 0, p(mask), 5, 3),
               comp(W, H, 3, p(mask), 3, 3), comp(W, H, 3, p(mask), 5, 4)):
        assert rc != 0
        with pytest.raises(_capi.RasterError):
            cx.check(rc)
    torch.cuda.synchronize()
    assert float(grad.abs().max()) == 0.0 and float(terms.abs().max()) == 0.0


class TS:
    """The sizes and helpers of tests/test_train_step_gpu.py's composed-step test."""
    SMALL = dict(plane_res=32, plane_channels=32, hidden_dim=128, image_size=64, seed=7)
    N_POINTS = 2000

    @staticmethod
    def _flat(params):
        return torch.cat([p.detach().reshape(-1).cpu() for p in params])

    @staticmethod
    def _half_step(tr, batch):
        """step() up to (not including) the optimizer: returns the loss; the flat gradient is in tr.flat_grad."""
        tr.flat_grad.zero_()
        loss = tr.local_loss(batch)
        loss.backward()
        return float(loss.detach())


def test_composed_masked_step_matches_the_oracle_backed_cpu_trainer(native_lib):
    """DecoderTrainer(apply_mask_to_rendering=True) as in test_composed_step_matches_the_oracle_backed_cpu_trainer (64 x 64
    image, 8 x 8 mask, 2 000 points, tri-planes): the HIP step with the masked fused loss and composite_mask in front of the
    perceptual term against the CPU trainer with the oracle rasterizer and the masked torch loss -- the same bounds: loss
    1e-5 max(1, |loss|), every parameter tensor's gradient 1e-10 + 1e-3 max|g|, parameters after Adam 1e-4.  Also the
    stream-order check of the new kernels inside a real step."""
    from _cpu_render import render_simple_cpu
    from gaussian_gan_decoder_amd.train import DecoderTrainer, make_scene_batch

    def make(device, **kw):
        extra = dict(render_fn=render_simple_cpu, loss_fn=MR.masked_image_loss_torch) if str(device) == "cpu" else {}
        tr = DecoderTrainer(device, n_scenes_total=2, backbone_params=3000, perceptual_weight=0.05, perceptual_width_div=16,
                            **extra, **TS.SMALL, **kw)
        with torch.no_grad():    # splats large enough that the 64 x 64 image sees the 2 000 points (as in TS._make)
            tr.decoder.scale_decoder.backbone[-1].bias += 3.5
            tr.decoder.opacity_decoder.backbone[-1].bias += 1.0
        return tr
    cpu_tr, gpu_tr = make("cpu", apply_mask_to_rendering=True), make(DEV, apply_mask_to_rendering=True)
    assert torch.equal(TS._flat(cpu_tr.params), TS._flat(gpu_tr.params))
    size = TS.SMALL["image_size"]
    cb = make_scene_batch([0, 1], TS.N_POINTS, size, "cpu", seed=0, with_mask=True)
    gb = make_scene_batch([0, 1], TS.N_POINTS, size, DEV, seed=0, with_mask=True)
    assert gb.mask.shape == (2, 1, 8, 8) and gb.mask.device.type == "cuda"
    l_unmasked = TS._half_step(make(DEV), gb)
    lc, lg = TS._half_step(cpu_tr, cb), TS._half_step(gpu_tr, gb)
    torch.cuda.synchronize()
    print(f"\n  masked loss: cpu {lc:.7f} gpu {lg:.7f}; unmasked gpu {l_unmasked:.7f}")
    assert abs(lc - lg) <= 1e-5 * max(1.0, abs(lc)), (lc, lg)
    assert abs(lg - l_unmasked) > 1e-5 * max(1.0, abs(l_unmasked)), "the masked and the unmasked loss of one batch must differ"
    gc, gg = cpu_tr.flat_grad.clone(), gpu_tr.flat_grad.detach().cpu()
    assert torch.isfinite(gg).all()
    off, worst = 0, 0.0
    for p in cpu_tr.params:
        n = p.numel()
        a, b = gc[off:off + n], gg[off:off + n]
        worst = max(worst, float((a - b).abs().max()) / (1e-10 + 1e-3 * float(a.abs().max())))
        off += n
    print(f"  worst gradient |err| / tol = {worst:.3f}")
    assert worst <= 1.0, worst
    assert float(gc.abs().max()) > 1e-4, "the step has no gradient signal"
    cpu_tr.allreduce_and_step()
    gpu_tr.allreduce_and_step()
    torch.cuda.synchronize()
    d = (TS._flat(cpu_tr.params) - TS._flat(gpu_tr.params)).abs()
    assert float(d.max()) <= 1e-4, float(d.max())
    with pytest.raises(ValueError):
        gpu_tr.step(make_scene_batch([0, 1], TS.N_POINTS, size, DEV, seed=0))
