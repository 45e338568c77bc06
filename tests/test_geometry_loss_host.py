"""Geometry loss, host side (no GPU): losses.geometry_loss_torch against the float64 restatement (tests/_geometry_loss_ref.py)
and autograd's gradcheck, fused_geometry_loss on CPU tensors, the analytic teacher maps of make_scene_batch, the new SceneBatch
fields, TeacherRender.geometry, the refusals and the untouched default trainer."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import losses as L
from gaussian_gan_decoder_amd import teacher
from gaussian_gan_decoder_amd.train import DecoderTrainer, SceneBatch, make_scene_batch
import _geometry_loss_ref as GR


def test_torch_form_passes_gradcheck_in_float64():
    depth, alpha, t, w = (x.double() for x in GR.make_inputs(16, 16, 4, 4, seed=50))
    depth.requires_grad_(True), alpha.requires_grad_(True)
    for ray_depth in (True, False):
        fn = lambda D, A: L.geometry_loss_torch(D, A, t, w, 0.11, 0.07, 0.7, 0.3, ray_depth)[0]
        assert torch.autograd.gradcheck(fn, (depth, alpha), eps=1e-7, atol=1e-9)


@pytest.mark.parametrize("tag", GR.SMALL)
@pytest.mark.parametrize("ray_depth", (True, False))
def test_torch_form_is_the_restatement(tag, ray_depth):
    """geometry_loss_torch (F.interpolate) against the explicit-index restatement in float64: terms to 1e-12, gradients to
    1e-12 of the gradient scale; and in float32 on CPU tensors fused_geometry_loss IS geometry_loss_torch."""
    H, W, th, tw, tx, ty = GR.CASES[tag]
    for mw, dw in GR.WEIGHTS:
        inp, ref, _ = GR.case(tag, (mw, dw), ray_depth)
        D, A = inp[0].double().requires_grad_(True), inp[1].double().requires_grad_(True)
        total, terms = L.geometry_loss_torch(D[None], A[None], inp[2].double()[None], inp[3].double()[None, None], tx, ty, mw, dw,
                                             ray_depth)
        (3 * total).backward()
        np.testing.assert_allclose(terms.numpy(), ref["terms"], rtol=1e-12, atol=1e-15)
        assert not terms.requires_grad and float(total.detach()) == float(terms[2])
        for got, want in ((D.grad, ref["grad_depth"]), (A.grad, ref["grad_alpha"])):
            keep = ~ref["fragile"]
            assert np.abs(got.numpy() - 3 * want)[keep].max() <= 1e-12 * (mw + dw) / (H * W)
        a = [x.clone().requires_grad_(True) for x in inp[:2]]
        b = [x.clone().requires_grad_(True) for x in inp[:2]]
        fa = L.fused_geometry_loss(a[0], a[1], inp[2], inp[3], tx, ty, mw, dw, ray_depth)
        fb = L.geometry_loss_torch(b[0], b[1], inp[2], inp[3], tx, ty, mw, dw, ray_depth)
        fa[0].backward(), fb[0].backward()
        assert torch.equal(fa[1], fb[1]) and torch.equal(a[0].grad, b[0].grad) and torch.equal(a[1].grad, b[1].grad)


def test_float32_torch_form_meets_the_gpu_bounds_on_the_cpu():
    """The bounds of tests/test_geometry_loss_gpu.py hold for the float32 torch form on the CPU (so they are a statement about
    float32, not about one kernel): gradients per pixel outside the fragile pixels, at most 0.1 % of them left out."""
    for tag in GR.SMALL:
        H, W, th, tw, tx, ty = GR.CASES[tag]
        inp, ref, _ = GR.case(tag)
        D, A = inp[0].clone().requires_grad_(True), inp[1].clone().requires_grad_(True)
        L.fused_geometry_loss(D, A, inp[2], inp[3], tx, ty, *GR.WEIGHTS[0])[0].backward()
        worst, left_out = GR.check_gradients(D.grad.numpy(), A.grad.numpy(), ref, *GR.WEIGHTS[0])
        assert worst <= 1.0, (tag, worst, left_out)


def test_recipe_has_the_regions_the_exact_zero_tests_need():
    for tag in GR.SMALL:
        (depth, alpha, t, w), ref, _ = GR.case(tag)
        if tag != "one_cell":
            assert ((ref["m"] == 0) & (alpha.numpy() == 0)).any() and ((ref["m"] == 0) & (alpha.numpy() > 0)).any(), tag
        assert float(alpha.max()) < 1.0 and float(w.max()) < 1.0 and float(w.max()) > 0.5


def test_scene_batch_geometry():
    ids, size = [0, 1, 2, 3, 4, 5], 72       # 9 x 9 teacher maps: the central cell's ray is the optical axis
    plain = make_scene_batch(ids, 300, size, "cpu", seed=3, with_mask=True)
    geo = make_scene_batch(ids, 300, size, "cpu", seed=3, with_mask=True, with_geometry=True)
    for name in ("positions", "cam2world", "fov_deg", "target", "scene_id", "mask"):
        assert torch.equal(getattr(plain, name), getattr(geo, name)), name
    assert plain.teacher_depth is None and plain.teacher_weights is None
    R = size // 8
    assert geo.teacher_depth.shape == geo.teacher_weights.shape == (len(ids), 1, R, R)
    assert geo.teacher_depth.dtype == geo.teacher_weights.dtype == torch.float32
    w = geo.teacher_weights
    assert float(w.min()) == 0.0 and float(w.max()) == 1.0 and bool((w == 0).any()) and bool((w == 1).any())
    assert bool(torch.isfinite(geo.teacher_depth).all())
    for b in range(len(ids)):
        dist = float(geo.cam2world[b, :3, 3].double().norm())
        tan = math.tan(math.radians(float(geo.fov_deg[b])) / 2)
        c = (2 * (R // 2 + 0.5) / R - 1) * tan
        cos = 1 / math.sqrt(1 + 2 * c * c)
        assert c == 0.0 and abs(float(geo.teacher_depth[b, 0, R // 2, R // 2]) * cos - (dist - 0.3)) <= 1e-5
        assert float(w[b, 0, R // 2, R // 2]) == 1.0
    with pytest.raises(ValueError):
        make_scene_batch([0], 10, 60, "cpu", with_geometry=True)


def test_scene_batch_constructed_the_old_way():
    z = torch.zeros(1)
    assert SceneBatch(z, z, z, z, z).teacher_depth is None and SceneBatch(z, z, z, z, z, z).teacher_weights is None
    assert SceneBatch(z, z, z, z, z, z).mask is z


def test_teacher_render_geometry():
    depth, weights = torch.arange(18.0), torch.arange(18.0) / 18
    tr = teacher.TeacherRender(torch.zeros(18, 32), depth, weights, "sigmoid", None)
    d, w = tr.geometry(3)
    assert d.shape == w.shape == (2, 1, 3, 3)
    assert torch.equal(d, tr.images(3)[1]) and torch.equal(w.reshape(-1), weights) and float(w.min()) == 0.0
    assert torch.equal(d[1, 0, 1], torch.tensor([12.0, 13.0, 14.0]))
    with pytest.raises(ValueError):
        tr.geometry(4)


def test_refusals():
    depth, alpha, t, w = GR.make_inputs(16, 16, 4, 4, seed=51)
    f = L.fused_geometry_loss
    with pytest.raises(ValueError):
        f(depth, alpha, t[:3], w[:3], 0.1, 0.1)                    # 3 does not divide 16
    with pytest.raises(ValueError):
        f(depth, alpha, t, w[:2], 0.1, 0.1)                        # the teacher's maps differ in size
    with pytest.raises(ValueError):
        f(depth, alpha[:8], t, w, 0.1, 0.1)
    with pytest.raises(ValueError):
        f(depth[None, None], alpha, t, w, 0.1, 0.1)
    with pytest.raises(ValueError):
        f(depth, alpha, t, w, 0.0, 0.1)
    with pytest.raises(ValueError):
        f(depth, alpha, t, w, 0.1, -1.0)
    with pytest.raises(TypeError):
        f(depth.double(), alpha.double(), t.double(), w.double(), 0.1, 0.1)
    with pytest.raises(TypeError):
        f(depth, alpha, t.double(), w, 0.1, 0.1)
    with pytest.raises(RuntimeError):
        f(depth, alpha, t.to("meta"), w, 0.1, 0.1)
    assert f(depth[None], alpha, t[None, None], w[None], 0.1, 0.1)[1].shape == (3,)


SMALL = dict(n_scenes_total=2, plane_res=16, plane_channels=8, hidden_dim=16, image_size=16, seed=5, fused_planes=False)


def _fake_render(calls, strict):
    """A render function that records its keywords; strict: it does not know render_depth_alpha at all."""
    def body(cam, gs, bg_color, kw):
        calls.append(dict(kw))
        s = cam.image_width
        a = torch.sigmoid(gs._opacity.mean()) * torch.ones(1, s, s)
        out = {"render": bg_color[:, None, None] * a + 0.1 * gs._features_dc.mean()}
        if kw.get("render_depth_alpha"):
            out["depth"], out["alpha"] = a * (2.4 + gs._xyz.mean()), a
        return out
    if strict:
        return lambda cam, gs, bg_color=None: body(cam, gs, bg_color, {})
    return lambda cam, gs, bg_color=None, **kw: body(cam, gs, bg_color, kw)


def _image_loss(image, target, **kw):
    return ((image - target) ** 2).mean(), None


def test_default_trainer_passes_no_new_keyword():
    calls = []
    tr = DecoderTrainer("cpu", render_fn=_fake_render(calls, strict=True), loss_fn=_image_loss, **SMALL)
    loss = tr.local_loss(make_scene_batch([0, 1], 50, 16, "cpu"))
    assert len(calls) == 2 and math.isfinite(float(loss.detach())) and not tr.geometry and tr.render_kwargs == {}
    same = DecoderTrainer("cpu", render_fn=_fake_render([], strict=True), loss_fn=_image_loss, mask_weight=0.0, depth_weight=0.0,
                          **SMALL)
    assert all(torch.equal(a, b) for a, b in zip(tr.params, same.params))
    assert float(same.local_loss(make_scene_batch([0, 1], 50, 16, "cpu", with_geometry=True)).detach()) == float(loss.detach())


def test_trainer_adds_the_geometry_term():
    calls, seen = [], []

    def geometry_fn(depth, alpha, td, tw, tx, ty, mw, dw):
        seen.append((tuple(td.shape), tx, ty, mw, dw))
        return L.geometry_loss_torch(depth, alpha, td, tw, tx, ty, mw, dw)
    batch = make_scene_batch([0, 1], 50, 16, "cpu", with_geometry=True)
    base = DecoderTrainer("cpu", render_fn=_fake_render([], strict=False), loss_fn=_image_loss, **SMALL)
    tr = DecoderTrainer("cpu", render_fn=_fake_render(calls, strict=False), loss_fn=_image_loss, mask_weight=0.7, depth_weight=0.3,
                        geometry_loss_fn=geometry_fn, **SMALL)
    default = DecoderTrainer("cpu", render_fn=_fake_render([], strict=False), loss_fn=_image_loss, mask_weight=0.7,
                             depth_weight=0.3, **SMALL)
    l0, l1 = float(base.local_loss(batch).detach()), tr.local_loss(batch)
    assert calls == [{"render_depth_alpha": True}] * 2 and len(seen) == 2
    tan = math.tan(float(batch.fov_deg[1]) / 360 * 2 * math.pi / 2)
    assert seen[1] == ((1, 2, 2), tan, tan, 0.7, 0.3)
    assert float(l1.detach()) > l0 and float(default.local_loss(batch).detach()) == float(l1.detach())   # on the CPU the default is the torch form
    l1.backward()
    assert float(tr.flat_grad.abs().max()) > 0
    with pytest.raises(ValueError, match="with_geometry=True"):
        tr.local_loss(make_scene_batch([0, 1], 50, 16, "cpu"))
    with pytest.raises(ValueError):
        DecoderTrainer("cpu", render_fn=_fake_render([], strict=False), loss_fn=_image_loss, depth_weight=-1.0, **SMALL)
