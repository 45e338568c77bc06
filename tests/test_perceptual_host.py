"""Host side of losses.FusedPerceptual (no GPU): the float64 restatement the GPU tests check against, the refusals, the CPU
path, the weight packer, the C entries and the trainer's keyword."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _perceptual_ref as R                                                                              # noqa: E402
from gaussian_gan_decoder_amd.losses import (FusedPerceptual, PerceptualStandIn, pack_conv_weights,      # noqa: E402
                                             unpack_conv_weights)


def _pair(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(B, 3, H, W, generator=g)
    return (target + 0.1 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1), target


@pytest.fixture
def no_native_calls(monkeypatch):
    """Any use of the library's contexts fails the test: the refusals must come first."""
    from gaussian_gan_decoder_amd import _capi

    def boom(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(_capi, "context_for", boom)
    monkeypatch.setattr(_capi, "context_and_stream", boom)


@pytest.mark.parametrize("width_div", [4, 16])
def test_float64_restatement_agrees_with_the_stand_in(width_div):
    """fp32 on the CPU against float64: 13 layers of fp32 rounding, K up to 9 * 128 -- 1e-5 relative on the loss and on the L2
    norm of gradient and features is an order above what fp32 leaves and orders below any error of definition."""
    m = PerceptualStandIn(seed=5, width_div=width_div)
    image, target = _pair(2, 32, 48)
    x = image.clone().requires_grad_(True)
    loss = m(x, target)
    loss.backward()
    ref = R.evaluate(m, image, target)
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    assert float((x.grad.double() - ref["grad"]).norm()) <= 1e-5 * float(ref["grad"].norm())
    assert float((m.features(image).double() - ref["features"]).norm()) <= 1e-5 * float(ref["features"].norm())


def test_float64_restatement_takes_max_size_and_affine():
    """max_size: the k x k mean is the stand-in's area interpolation; input_affine (2, -1) is its img * 2 - 1."""
    m = PerceptualStandIn(seed=5, width_div=16)
    image, target = _pair(1, 64, 64)
    small = R.evaluate(m, image, target, max_size=32)
    pooled = R.evaluate(m, torch.nn.functional.avg_pool2d(image.double(), 2), torch.nn.functional.avg_pool2d(target.double(), 2))
    assert abs(small["loss"] - pooled["loss"]) <= 1e-12 * abs(pooled["loss"])
    assert R.evaluate(m, image, target, input_affine=((2.0,) * 3, (-1.0,) * 3))["loss"] == R.evaluate(m, image, target)["loss"]
    assert R.evaluate(m, image, target, input_affine=((1.5, 2.0, 2.5), (-1.0, -0.9, -1.1)))["loss"] != small["loss"]


def test_twins_round_operands_only():
    """The twins stay close to float64 and the split pair is closer than f16 / bf16."""
    m = PerceptualStandIn(seed=5, width_div=2)
    image, target = _pair(1, 16, 16)
    exact = R.evaluate(m, image, target)
    err = {t: float((R.evaluate(m, image, target, tier=t)["grad"] - exact["grad"]).norm() / exact["grad"].norm()) for t in R.TIERS}
    assert 0 < err["fp32"] < err["bf16"] < 0.5


class _Shape(torch.nn.Module):
    def __init__(self, convs, lin):
        super().__init__()
        self.convs, self.lin = torch.nn.ModuleList(convs), torch.nn.ParameterList(lin)


def test_refusals_come_before_any_native_call(no_native_calls):
    fp = FusedPerceptual(PerceptualStandIn(seed=1, width_div=2), precision="bf16", max_size=32)
    for shape in ((1, 3, 24, 32), (1, 3, 32, 40), (3, 30, 32)):            # H or W not a multiple of 16
        with pytest.raises(ValueError, match="multiples of 16"):
            fp(torch.rand(shape), torch.rand(shape))
        with pytest.raises(ValueError, match="multiples of 16"):
            fp.features(torch.rand(shape))
    for shape in ((1, 3, 48, 48), (1, 3, 64, 80)):                         # above max_size, not a multiple of it
        with pytest.raises(ValueError, match="multiple of it"):
            fp(torch.rand(shape), torch.rand(shape))
    with pytest.raises(ValueError, match="one shape"):
        fp(torch.rand(1, 3, 32, 32), torch.rand(2, 3, 32, 32))
    for width_div in (4, 16):                                              # widths that are no multiple of 32
        with pytest.raises(ValueError, match="multiple of 32"):
            FusedPerceptual(PerceptualStandIn(seed=1, width_div=width_div))
    with pytest.raises(ValueError, match="precision"):
        FusedPerceptual(PerceptualStandIn(seed=1), precision="fp16")
    m = PerceptualStandIn(seed=1, width_div=2)
    with pytest.raises(ValueError, match="13 `convs`"):
        FusedPerceptual(_Shape(list(m.convs)[:12], list(m.lin)))
    with pytest.raises(ValueError, match="13 `convs`"):
        FusedPerceptual(_Shape(list(m.convs), list(m.lin)[:4]))
    with pytest.raises(ValueError, match="3x3"):
        FusedPerceptual(_Shape([torch.nn.Conv2d(3, 32, 5, padding=2)] + list(m.convs)[1:], list(m.lin)))
    with pytest.raises(ValueError, match="3x3"):                            # a chain that does not fit
        FusedPerceptual(_Shape(list(m.convs)[:5] + [torch.nn.Conv2d(64, 128, 3, padding=1)] + list(m.convs)[6:], list(m.lin)))
    with pytest.raises(ValueError, match="lin"):
        FusedPerceptual(_Shape(list(m.convs), [torch.nn.Parameter(torch.rand(7))] + list(m.lin)[1:]))

    class Moved(PerceptualStandIn):
        TAPS = (1, 3, 6, 9, 11)
    with pytest.raises(ValueError, match="taps"):
        FusedPerceptual(Moved(seed=1, width_div=2))


def test_cpu_tensors_take_the_wrapped_module(no_native_calls):
    m = PerceptualStandIn(seed=3, width_div=2)
    fp = FusedPerceptual(m, precision="fp32")
    image, target = _pair(2, 32, 32)
    x, y = image.clone().requires_grad_(True), image.clone().requires_grad_(True)
    a, b = fp(x, target), m(y, target)
    a.backward()
    b.backward()
    assert torch.equal(a, b) and torch.equal(x.grad, y.grad)
    assert torch.equal(fp(image[0], target[0]), m(image[0], target[0]))      # [3, H, W]
    assert torch.equal(fp.features(image), m.features(image))


@pytest.mark.parametrize("fmt,tol", [("f16", 2.0 ** -11), ("bf16", 2.0 ** -8), ("split", 2.0 ** -16)])
@pytest.mark.parametrize("cout,cin", [(32, 32), (96, 64), (128, 64)])
def test_weight_packer_round_trips(fmt, tol, cout, cin):
    """unpack(pack(w)) is w rounded to the format; the image has the documented shape, zero columns past cout, and lane l of
    tile t, element j, is k = 8 (l >> 4) + j of output channel 16 t + (l & 15)."""
    w = torch.randn(cout, cin, 3, 3, generator=torch.Generator().manual_seed(cout + cin))
    p = pack_conv_weights(w, fmt)
    tiles = (cout + 63) // 64 * 4
    assert tuple(p.shape) == (9 * cin // 32, 2 if fmt == "split" else 1, tiles, 64, 8)
    u = unpack_conv_weights(p, cout, cin)
    assert float((u - w).abs().max()) <= tol * float(w.abs().max())
    assert torch.equal(pack_conv_weights(u, fmt).float().sum(1), p.float().sum(1))     # a fixed point: nothing moves twice
    assert float(p.float()[:, :, cout // 16:].abs().max() if tiles * 16 > cout else 0.0) == 0.0
    tap, chunk, t, l, j = 5, cin // 32 - 1, 1, 37, 3
    want = w[16 * t + (l & 15), 32 * chunk + 8 * (l >> 4) + j, tap // 3, tap % 3]
    assert abs(float(p.float().sum(1)[tap * (cin // 32) + chunk, t, l, j]) - float(want)) <= tol * abs(float(want))
    with pytest.raises(ValueError):
        pack_conv_weights(torch.randn(32, 48, 3, 3), fmt)


def test_symbols_are_in_the_built_library(native_lib):
    from gaussian_gan_decoder_amd import _capi
    for name in ("ggd_perceptual_tmp_bytes", "ggd_perceptual_loss", "ggd_perceptual_features"):
        assert name in _capi.EXPORTS and hasattr(native_lib, name)


def test_tmp_bytes_sizes_the_workspace_and_refuses_what_the_kernels_do_not_take(native_lib):
    from gaussian_gan_decoder_amd import _capi
    fp = FusedPerceptual(PerceptualStandIn(seed=1, width_div=2), precision="bf16").repack("cpu")
    d = fp._desc(2, 32, 32, 32, 32, torch.device("cpu"))
    fwd, both = (native_lib.ggd_perceptual_tmp_bytes(C.byref(d), 4, g) for g in (0, 1))
    acts = 4 * sum(w * (32 >> l) ** 2 for w, l in zip(fp.widths, (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4))) * 2    # f16
    assert acts < fwd < both
    d.tier = _capi.PERC_TIERS["fp32"]
    assert native_lib.ggd_perceptual_tmp_bytes(C.byref(d), 4, 0) > fwd
    for field, value in (("H", 24), ("W", 40), ("tier", 7), ("B", 0), ("H_in", 48)):
        bad = fp._desc(2, 32, 32, 32, 32, torch.device("cpu"))
        setattr(bad, field, value)
        assert native_lib.ggd_perceptual_tmp_bytes(C.byref(bad), 4, 1) == 0
    bad = fp._desc(2, 32, 32, 32, 32, torch.device("cpu"))
    bad.widths[4] = 48
    assert native_lib.ggd_perceptual_tmp_bytes(C.byref(bad), 4, 1) == 0


def test_trainer_keyword_leaves_the_cpu_step_as_it_is():
    """On the CPU the trainer keeps the module itself: the step's loss and gradient are the default step's, bit for bit."""
    from _cpu_render import render_simple_cpu
    from _torch_losses import image_loss_torch
    from gaussian_gan_decoder_amd.train import DecoderTrainer, make_scene_batch
    out = []
    for kw in (dict(), dict(fused_perceptual=True), dict(fused_perceptual=True, perceptual_precision="fp32")):
        tr = DecoderTrainer("cpu", render_fn=render_simple_cpu, loss_fn=image_loss_torch, n_scenes_total=1, plane_res=16,
                            plane_channels=32, hidden_dim=128, image_size=32, seed=7, perceptual_weight=0.5,
                            perceptual_width_div=16, **kw)
        assert tr.perceptual_fn is tr.perceptual
        with torch.no_grad():
            tr.decoder.scale_decoder.backbone[-1].bias += 3.5
        batch = make_scene_batch([0], 300, 32, "cpu", seed=0)
        tr.flat_grad.zero_()
        loss = tr.local_loss(batch)
        loss.backward()
        out.append((float(loss.detach()), tr.flat_grad.clone()))
    assert out[0][0] == out[1][0] == out[2][0]
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][1], out[2][1])
