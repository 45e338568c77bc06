"""Masked image loss (the reference's --apply_mask_to_rendering), host side: the torch restatement (tests/_masked_loss_ref.py)
against vectors from the reference's own functions (tests/golden/masked_losses.npz, made by
tests/golden/make_masked_loss_golden.py), composite_mask on CPU tensors, the argument checks, make_scene_batch(with_mask=True)
and the CPU trainer with apply_mask_to_rendering."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import losses as L
import _masked_loss_ref as MR

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masked_losses.npz"))
W4 = dict(l1_weight=0.2, l2_weight=0.1, ssim_weight=0.5, sobel_weight=0.2)


def _reference_composite(x, mask4):
    """main/train_pano2gaussian_decoder.py:239-241, literally."""
    H, W = x.shape[-2:]
    rescale_mask = F.interpolate(mask4, scale_factor=(H // mask4.shape[2], W // mask4.shape[3]), mode="bilinear")[0]
    return x * rescale_mask + 1 - rescale_mask, rescale_mask


@pytest.mark.parametrize("tag", MR.CASES)
def test_restatement_matches_reference_vectors(tag):
    """float32 restatement against the reference's functions: the bars of test_torch_losses_match_reference_vectors;
    the upsampled mask within 3e-7 of F.interpolate's."""
    img = torch.from_numpy(GOLD[f"{tag}_image"]).requires_grad_(True)
    tgt = torch.from_numpy(GOLD[f"{tag}_target"])
    mask = torch.from_numpy(GOLD[f"{tag}_mask"])
    up = MR.upsample_mask(mask, img.shape[1], img.shape[2])
    assert np.abs(up.numpy() - GOLD[f"{tag}_upmask"]).max() <= 3e-7
    assert (GOLD[f"{tag}_upmask"] == 0).any() and (GOLD[f"{tag}_upmask"] == 1).any()
    if mask.shape == up.shape:
        assert torch.equal(up, mask), "a factor of 1 returns the mask unchanged"
    total, terms = MR.masked_image_loss_torch(img, tgt, mask=mask, **W4)
    np.testing.assert_allclose(terms.detach().numpy(), GOLD[f"{tag}_terms"][:4], rtol=1e-6, atol=1e-7)
    total.backward()
    np.testing.assert_allclose(img.grad.numpy(), GOLD[f"{tag}_grad"], atol=1e-8, rtol=1e-5)


def test_restatement_without_mask_is_the_unmasked_loss():
    import _torch_losses as TL
    img, tgt = torch.from_numpy(GOLD["A_image"]), torch.from_numpy(GOLD["A_target"])
    assert torch.equal(MR.masked_image_loss_torch(img, tgt, **W4)[1], TL.image_loss_torch(img, tgt, **W4)[1])


@pytest.mark.parametrize("tag", MR.CASES)
def test_composite_mask_on_cpu_is_the_reference_expression(tag):
    img = torch.from_numpy(GOLD[f"{tag}_image"]).requires_grad_(True)
    mask = torch.from_numpy(GOLD[f"{tag}_mask"]).requires_grad_(True)
    want, m = _reference_composite(img.detach(), mask.detach()[None, None])
    for mk in (mask, mask[None], mask[None, None]):
        assert torch.equal(L.composite_mask(img, mk), want)
    out = L.composite_mask(img, mask)
    g = torch.from_numpy(GOLD[f"{tag}_target"])
    (out * g).sum().backward()
    assert torch.equal(img.grad, m * g) and mask.grad is None
    # a batch: one shared mask, and one mask per image
    imgs = torch.stack([img.detach(), torch.from_numpy(GOLD[f"{tag}_target"])])
    masks = torch.stack([mask.detach()[None], 1.0 - mask.detach()[None]])
    shared, per = L.composite_mask(imgs, mask.detach()), L.composite_mask(imgs, masks)
    assert torch.equal(shared[0], want) and torch.equal(per[0], want)
    assert torch.equal(shared[1], _reference_composite(imgs[1], mask.detach()[None, None])[0])
    assert torch.equal(per[1], _reference_composite(imgs[1], masks[1][None])[0])


def test_fused_loss_with_a_cpu_mask_raises():
    with pytest.raises(RuntimeError):
        L.fused_image_loss(torch.zeros(3, 16, 16), torch.zeros(3, 16, 16), mask=torch.ones(2, 2))


def test_mask_size_must_divide_the_image():
    img = torch.zeros(3, 16, 24)
    for bad in (torch.ones(3, 4), torch.ones(4, 5), torch.ones(1, 1, 32, 24), torch.ones(2, 1, 4, 4)):
        with pytest.raises(ValueError):
            L.fused_image_loss(img, img, mask=bad)
    for bad in (torch.ones(3, 4), torch.ones(4, 5), torch.ones(1, 1, 32, 24)):
        with pytest.raises(ValueError):
            L.composite_mask(img, bad)
        with pytest.raises(ValueError):
            L.composite_mask(img[None], bad)


def test_make_scene_batch_with_mask_leaves_the_other_fields_alone():
    from gaussian_gan_decoder_amd.train import SceneBatch, make_scene_batch
    a = make_scene_batch([0, 3], 50, 64, "cpu", seed=2)
    b = make_scene_batch([0, 3], 50, 64, "cpu", seed=2, with_mask=True)
    assert a.mask is None
    for f in ("positions", "cam2world", "fov_deg", "target", "scene_id"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert b.mask.shape == (2, 1, 8, 8) and b.mask.dtype == torch.float32
    assert (b.mask == 0).any() and (b.mask == 1).any() and ((b.mask > 0) & (b.mask < 1)).any()
    assert b.mask[0, 0, 0, 0] == 0 and b.mask[0, 0, 3, 3] == 1      # an exact-0 rim around an exact-1 core
    assert SceneBatch(a.positions, a.cam2world, a.fov_deg, a.target, a.scene_id).mask is None   # positional construction


def test_cpu_trainer_with_apply_mask_to_rendering():
    from _cpu_render import render_simple_cpu
    from gaussian_gan_decoder_amd.train import DecoderTrainer, make_scene_batch
    cfg = dict(plane_res=16, plane_channels=8, hidden_dim=16, image_size=32, seed=3)

    def make(**kw):
        tr = DecoderTrainer("cpu", render_fn=render_simple_cpu, loss_fn=MR.masked_image_loss_torch, lr=1e-3,
                            perceptual_weight=0.05, perceptual_width_div=16, n_scenes_total=2, **cfg, **kw)
        tr.decoder.scale_decoder.backbone[-1].bias.data += 3.0   # splats large enough for the 32 x 32 image to see 300 points
        return tr
    batch = make_scene_batch([0, 1], 300, 32, "cpu", seed=0, with_mask=True)
    plain, masked = make(), make(apply_mask_to_rendering=True)
    before = torch.cat([p.detach().reshape(-1).clone() for p in masked.params])
    l_plain, l_masked = plain.step(batch), masked.step(batch)
    assert np.isfinite(l_masked) and abs(l_masked - l_plain) > 1e-4 * abs(l_plain), (l_plain, l_masked)
    after = torch.cat([p.detach().reshape(-1) for p in masked.params])
    assert torch.isfinite(after).all() and float((after - before).abs().max()) > 0
    with pytest.raises(ValueError):
        masked.step(make_scene_batch([0, 1], 300, 32, "cpu", seed=0))
