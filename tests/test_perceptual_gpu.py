"""losses.FusedPerceptual on the GPU (csrc/ggd_perceptual.hip) against float64 (tests/_perceptual_ref.py).

Every case runs at full width and width_div=2, in both tiers.  The bounds are measured, not fixed: per case and tier the TWIN --
the float64 network with the tier's operand rounding -- gives e = |g_twin - g64| / |g64|, and the kernels must stay within
|g_gpu - g64| <= 2 e |g64| (the same for the `features` rows): kernel and twin share the rounding model and differ in the
accumulation order, two draws of the same process of flipped ReLU masks and pool arg-maxes.  The scalar loss is held to twice the
LARGEST relative twin loss error over the file's cases (per tier and width), so that a cancellation in one twin sets no unreachable bar.
Every figure is printed before it is asserted (pytest -s).
"""
import copy
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SEED = 5
TIERS = ("bf16", "fp32")
WIDTHS = (1, 2)
AFFINE = ((1.7, 2.2, 1.9), (-0.8, -1.1, -0.9))
#        name: (B, H, W, max_size, input_affine, tied)
CASES = {
    "b2_32x32": (2, 32, 32, 256, None, False),
    "b3_16x48": (3, 16, 48, 256, None, False),       # rectangular, odd batch; deepest maps 1 x 3: an M tile spans images, ends partial
    "b1_16x16": (1, 16, 16, 256, None, False),       # deepest map 1 x 1: every tap but the centre is padding
    "mean2_32x32": (2, 32, 32, 16, None, False),     # 2 x 2 mean and its backward
    "mean3_48x48": (1, 48, 48, 16, None, False),     # 3 x 3 mean
    "affine_32x32": (2, 32, 32, 256, AFFINE, False),
    "tied_32x32": (2, 32, 32, 256, None, True),
}


def _inputs(name):
    B, H, W, _, _, tied = CASES[name]
    g = torch.Generator().manual_seed(100 + sorted(CASES).index(name))
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    target = torch.stack([torch.stack([0.5 + 0.4 * torch.sin(3 * xx + c + b) * torch.cos(2 * yy - b) for c in range(3)])
                          for b in range(B)])
    image = (target + 0.15 * torch.randn(target.shape, generator=g)).clamp(0, 1)
    if tied:
        # left half: a constant image (interior activations exactly equal: every pool window there is a non-zero tie);
        # right half: image == target (the difference is exactly 0)
        image[..., : W // 2] = torch.tensor([0.3, 0.6, 0.45])[None, :, None, None]
        image[..., W // 2:] = target[..., W // 2:]
    return image.float().contiguous(), target.float().contiguous()


_modules, _refs = {}, {}


def _module(width_div):
    from gaussian_gan_decoder_amd.losses import PerceptualStandIn
    if width_div not in _modules:
        _modules[width_div] = PerceptualStandIn(seed=SEED, width_div=width_div)
    return _modules[width_div]


def _ref(name, width_div):
    """float64 result and both twins of one case, computed once."""
    import _perceptual_ref as R
    key = (name, width_div)
    if key not in _refs:
        image, target = _inputs(name)
        _, _, _, max_size, affine, _ = CASES[name]
        m = _module(width_div)
        exact = R.evaluate(m, image, target, max_size, affine)
        twins = {t: R.evaluate(m, image, target, max_size, affine, tier=t) for t in TIERS}
        rel = lambda a, b: float((a - b).norm() / b.norm())
        _refs[key] = dict(exact=exact, e_grad={t: rel(twins[t]["grad"], exact["grad"]) for t in TIERS},
                          e_feat={t: rel(twins[t]["features"], exact["features"]) for t in TIERS},
                          e_loss={t: abs(twins[t]["loss"] - exact["loss"]) / abs(exact["loss"]) for t in TIERS})
    return _refs[key]


def _loss_bound(tier, width_div):
    return 2.0 * max(_ref(n, width_div)["e_loss"][tier] for n in CASES)


def _run(name, width_div, tier):
    from gaussian_gan_decoder_amd.losses import FusedPerceptual
    _, _, _, max_size, affine, _ = CASES[name]
    image, target = _inputs(name)
    fp = FusedPerceptual(copy.deepcopy(_module(width_div)).to("cuda"), precision=tier, max_size=max_size, input_affine=affine)
    x = image.cuda().requires_grad_(True)
    loss = fp(x, target.cuda())
    loss.backward()
    feat = fp.features(image.cuda())
    torch.cuda.synchronize()
    return fp, float(loss.detach()), x.grad.detach().cpu().double(), feat.cpu().double()


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("width_div", WIDTHS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_loss_gradient_and_features_against_float64(native_lib, name, width_div, tier):
    ref = _ref(name, width_div)
    exact = ref["exact"]
    _, loss, grad, feat = _run(name, width_div, tier)
    err_g = float((grad - exact["grad"]).norm() / exact["grad"].norm())
    err_f = float((feat - exact["features"]).norm() / exact["features"].norm())
    err_l = abs(loss - exact["loss"]) / abs(exact["loss"])
    bound_l = _loss_bound(tier, width_div)
    print(f"\nPERC {name} width_div={width_div} tier={tier}: grad gpu {err_g:.3e} twin {ref['e_grad'][tier]:.3e} | "
          f"features gpu {err_f:.3e} twin {ref['e_feat'][tier]:.3e} | loss gpu {err_l:.3e} twin {ref['e_loss'][tier]:.3e} "
          f"bound {bound_l:.3e}")
    assert torch.isfinite(grad).all() and torch.isfinite(feat).all()
    assert tuple(feat.shape) == tuple(exact["features"].shape)
    assert err_g <= 2.0 * ref["e_grad"][tier]
    assert err_f <= 2.0 * ref["e_feat"][tier]
    assert err_l <= bound_l


@pytest.mark.parametrize("tier", TIERS)
def test_two_calls_are_bit_identical(native_lib, tier):
    _, l0, g0, f0 = _run("b3_16x48", 1, tier)
    _, l1, g1, f1 = _run("b3_16x48", 1, tier)
    assert l0 == l1 and torch.equal(g0, g1) and torch.equal(f0, f1)


def test_repack_reads_the_weights_again(native_lib):
    from gaussian_gan_decoder_amd.losses import FusedPerceptual, PerceptualStandIn
    image, target = (t.cuda() for t in _inputs("b1_16x16"))
    m = PerceptualStandIn(seed=SEED, width_div=2).cuda()
    fp = FusedPerceptual(m, precision="fp32")
    before = float(fp(image, target))
    with torch.no_grad():
        m.convs[3].weight.mul_(1.5)
    assert float(fp(image, target)) == before          # the packed image is a copy
    after = float(fp.repack()(image, target))
    assert abs(after - float(m(image, target))) <= 1e-3 * abs(after) and after != before


@pytest.mark.parametrize("tier", TIERS)
def test_one_trainer_step(native_lib, tier):
    """2 scenes x 2048 points at 64 x 64: the step with fused_perceptual=True against the step without it.  The loss is held to the
    tier's pooled loss bound (the other terms are shared, so the relative error only shrinks); the decoder's flat gradient to
    2 e_max, e_max the largest twin gradient error of the tier over the file's full-width cases: the perceptual image gradient is
    off by at most that share of itself, the other terms' image gradient not at all, and both reach the parameters through one
    shared Jacobian."""
    from gaussian_gan_decoder_amd.train import DecoderTrainer, make_scene_batch
    dev = torch.device("cuda")
    res = {}
    for fused in (False, True):
        tr = DecoderTrainer(dev, n_scenes_total=2, plane_res=32, plane_channels=32, hidden_dim=128, image_size=64, seed=7,
                            perceptual_weight=1.0, perceptual_width_div=1, fused_perceptual=fused, perceptual_precision=tier)
        with torch.no_grad():     # splats large enough that the 64 x 64 image sees the points
            tr.decoder.scale_decoder.backbone[-1].bias += 3.5
            tr.decoder.opacity_decoder.backbone[-1].bias += 1.0
        batch = make_scene_batch([0, 1], 2048, 64, dev, seed=0)
        tr.flat_grad.zero_()
        loss = tr.local_loss(batch)
        loss.backward()
        res[fused] = (float(loss.detach()), tr.flat_grad.detach().cpu().double().clone())
    err_l = abs(res[True][0] - res[False][0]) / abs(res[False][0])
    err_g = float((res[True][1] - res[False][1]).norm() / res[False][1].norm())
    e_max = max(_ref(n, 1)["e_grad"][tier] for n in CASES)
    print(f"\nPERC trainer tier={tier}: loss {res[False][0]:.6f} -> {res[True][0]:.6f} (rel {err_l:.3e}, bound "
          f"{_loss_bound(tier, 1):.3e}); flat gradient rel {err_g:.3e}, bound {2 * e_max:.3e}")
    assert err_l <= _loss_bound(tier, 1)
    assert err_g <= 2.0 * e_max
