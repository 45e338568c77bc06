"""Geometry loss on the GPU: losses.fused_geometry_loss (ggd_geometry_loss, two launches) against the float64 restatement of
tests/_geometry_loss_ref.py on its seeded cases, the raw C entry point, the loss behind the rasterizer's depth / alpha maps and
one DecoderTrainer step with the geometry term."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import losses as L
import _geometry_loss_ref as GR

DEV = torch.device("cuda:0")


def _run(tag, weights, ray_depth, scale=3.0):
    """One call on the device with the upstream scalar `scale`: (terms, depth.grad, alpha.grad) as numpy, and the case."""
    H, W, th, tw, tx, ty = GR.CASES[tag]
    inp, ref, terms32 = GR.case(tag, weights, ray_depth)
    D, A, t, w = (x.to(DEV) for x in inp)
    D.requires_grad_(True), A.requires_grad_(True)
    t.requires_grad_(True), w.requires_grad_(True)
    total, terms = L.fused_geometry_loss(D[None], A, t, w[None, None], tx, ty, weights[0], weights[1], ray_depth)
    (scale * total).backward()
    assert float(total.detach()) == float(terms[2]) and not terms.requires_grad
    assert t.grad is None and w.grad is None and D.grad.shape == D.shape and A.grad.shape == A.shape
    return terms.cpu().numpy(), D.grad.cpu().numpy(), A.grad.cpu().numpy(), inp, ref, terms32


def _check_case(tag, weights, ray_depth):
    terms, gd, ga, inp, ref, terms32 = _run(tag, weights, ray_depth)
    err = np.abs(terms.astype(np.float64) - ref["terms"])
    bound = GR.term_bounds(ref["terms"], terms32)
    print(f"\n  {tag} weights {weights} ray_depth {ray_depth}: terms {ref['terms']}, |err| {err} of bounds {bound}; float32 torch "
          f"reference |err| {np.abs(terms32 - ref['terms'])}")
    assert (err <= bound).all(), (err, bound)
    worst, left_out = GR.check_gradients(gd, ga, ref, weights[0], weights[1], scale=3.0)
    print(f"  worst gradient |err| / bound {worst:.3f}; {left_out} of {gd.size} pixels left out as fragile")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("ray_depth", (True, False))
@pytest.mark.parametrize("weights", GR.WEIGHTS)
@pytest.mark.parametrize("tag", GR.SMALL)
def test_terms_and_gradients_match_float64(native_lib, tag, weights, ray_depth):
    """Terms: the larger of rtol 2e-6 + atol 1e-7 and 4 x the float32 CPU reference's own deviation from float64.  Gradient maps
    under (3 * total).backward(), per pixel: |g - g64| <= 1e-5 |g64| + 1e-6 (mask_weight + depth_weight) / (H W), the pixels with a
    fragile sign decision (at most 0.1 %) left out."""
    _check_case(tag, weights, ray_depth)


def test_terms_and_gradients_match_float64_at_the_workload_shape(native_lib):
    _check_case("workload", GR.WEIGHTS[0], True)


@pytest.mark.parametrize("tag", GR.SMALL)
def test_exact_zeros(native_lib, tag):
    """Where the weights' four taps and A, D are all 0 both gradients are +0.0 (bit pattern 0); where m == 0 exactly and A > 0
    the depth residual contributes nothing: grad_depth is +0.0 and grad_alpha is bit for bit that of depth_weight = 0."""
    _, gd, ga, inp, ref, _ = _run(tag, GR.WEIGHTS[0], True, scale=1.0)
    _, gd0, ga0, _, _, _ = _run(tag, (GR.WEIGHTS[0][0], 0.0), True, scale=1.0)
    D, A = inp[0].numpy(), inp[1].numpy()
    bits = lambda a: a.view(np.int32)
    empty = (ref["m"] == 0) & (A == 0) & (D == 0)      # m == 0 in float64 with non-negative taps: every tap that counts is 0
    seen = (ref["m"] == 0) & (A > 0)
    if tag != "one_cell":
        assert empty.any() and seen.any()
    assert (bits(gd)[empty] == 0).all() and (bits(ga)[empty] == 0).all()
    assert (bits(gd)[seen] == 0).all() and (bits(ga)[seen] == bits(ga0)[seen]).all()
    assert (ga[seen] == np.float32(GR.WEIGHTS[0][0]) / np.float32(gd.size)).all()
    assert (gd0 == 0).all()


def test_run_to_run_bit_identical(native_lib):
    for tag in ("f2_odd", "workload"):
        a, b = _run(tag, GR.WEIGHTS[0], True), _run(tag, GR.WEIGHTS[0], True)
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))


def test_c_abi(native_lib):
    """ggd_geometry_loss_tmp_bytes is positive and monotone; every invalid argument returns GGD_E_INVALID with a message and
    writes nothing; a valid call writes H * W floats of either gradient map and not one more (guard words behind both)."""
    from gaussian_gan_decoder_amd import _capi
    cx = _capi.context_for(DEV)
    lib = cx.lib
    sizes = [lib.ggd_geometry_loss_tmp_bytes(s, s) for s in (1, 33, 64, 65, 512, 1024, 2048)]
    assert all(b > 0 for b in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert lib.ggd_geometry_loss_tmp_bytes(0, 8) == 0 and lib.ggd_geometry_loss_tmp_bytes(8, -1) == 0
    tag = "one_cell"                                    # 33 x 65: the last workgroup of a row and of a column is partial
    H, W, th, tw, tx, ty = GR.CASES[tag]
    inp, ref, _ = GR.case(tag)
    D, A, t, w = (x.to(DEV) for x in inp)
    nbytes = lib.ggd_geometry_loss_tmp_bytes(W, H)
    tmp = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    GUARD, PAD = 12345.0, 256
    gd, ga = (torch.full((H * W + PAD,), GUARD, device=DEV) for _ in range(2))
    terms = torch.zeros(3, device=DEV)
    w2 = (C.c_float * 2)(*GR.WEIGHTS[0])
    p = lambda x: C.c_void_p(x.data_ptr())
    good = dict(W=W, H=H, depth=p(D), alpha=p(A), t=p(t), w=p(w), tw=tw, th=th, tx=tx, ty=ty, w2=w2, terms=p(terms), gd=p(gd),
                ga=p(ga), tmp=p(tmp), nbytes=nbytes)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ggd_geometry_loss(cx.handle, None, a["W"], a["H"], a["depth"], a["alpha"], a["t"], a["w"], a["tw"], a["th"],
                                     a["tx"], a["ty"], 1, a["w2"], a["terms"], a["gd"], a["ga"], a["tmp"], a["nbytes"])
    bad = [dict(depth=None), dict(alpha=None), dict(t=None), dict(w=None), dict(w2=None), dict(terms=None), dict(gd=None),
           dict(ga=None), dict(tmp=None), dict(W=0), dict(H=0), dict(tw=0), dict(th=-1), dict(tw=2), dict(th=2),
           dict(nbytes=nbytes - 1), dict(nbytes=0)]
    for kw in bad:
        rc = call(**kw)
        assert rc != 0, kw
        with pytest.raises(_capi.RasterError, match="ggd_geometry_loss"):
            cx.check(rc)
    torch.cuda.synchronize()
    assert float(terms.abs().max()) == 0.0 and bool((gd == GUARD).all()) and bool((ga == GUARD).all())
    cx.check(call())
    torch.cuda.synchronize()
    for g in (gd, ga):
        assert bool((g[H * W:] == GUARD).all()) and bool((g[:H * W] != GUARD).all())
    worst, _ = GR.check_gradients(gd[:H * W].cpu().numpy(), ga[:H * W].cpu().numpy(), ref, *GR.WEIGHTS[0])
    assert worst <= 1.0
    assert (np.abs(terms.cpu().numpy() - ref["terms"]) <= GR.term_bounds(ref["terms"], GR.case(tag)[2])).all()


def test_through_the_rasterizer(native_lib):
    """256 Gaussians at 64 x 64, render_simple(render_depth_alpha=True): the gradients the loss leaves on out["depth"] and
    out["alpha"] satisfy the per-pixel bound against the float64 restatement evaluated on the rendered maps, the point
    gradients are finite and not all zero, and a second graph that reads only out["render"] still runs."""
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    from gaussian_gan_decoder_amd.synthetic import make_scene
    from gaussian_gan_decoder_amd.cameras import look_at_cam2world
    from gaussian_gan_decoder_amd.train import _sphere_geometry
    S, fov_deg, mw, dw = 64, 12.0, 0.7, 0.3
    sc = make_scene(256, S, "shell", seed=4, fov_deg=fov_deg, log_scale_mean=-4.0).to(DEV)
    t, w = _sphere_geometry(look_at_cam2world(), fov_deg, S // 8)
    tan = math.tan(sc.cam.FoVx * 0.5)
    pc = sc.gaussian_model(requires_grad=True)
    out = render_simple(sc.cam, pc, bg_color=sc.bg, render_depth_alpha=True)
    depth, alpha = out["depth"], out["alpha"]
    assert depth.shape == alpha.shape == (1, S, S)
    depth.retain_grad(), alpha.retain_grad()
    total, terms = L.fused_geometry_loss(depth, alpha, t.to(DEV), w.to(DEV), tan, tan, mw, dw)
    total.backward()
    ref = GR.float64_of(depth.detach().cpu()[0], alpha.detach().cpu()[0], t, w, tan, tan, mw, dw)
    assert float(alpha.detach().max()) > 0.1 and float(terms[1]) > 0
    worst, left_out = GR.check_gradients(depth.grad.cpu().numpy(), alpha.grad.cpu().numpy(), ref, mw, dw)
    print(f"\n  terms {terms.cpu().numpy()} (float64 {ref['terms']}); worst gradient |err| / bound {worst:.3f}, {left_out} left out")
    assert worst <= 1.0, worst
    for g in (pc._xyz.grad, pc._opacity.grad):
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    pc2 = sc.gaussian_model(requires_grad=True)
    out2 = render_simple(sc.cam, pc2, bg_color=sc.bg, render_depth_alpha=True)
    out2["render"].sum().backward()
    assert bool(torch.isfinite(pc2._xyz.grad).all()) and float(pc2._xyz.grad.abs().max()) > 0


def test_one_trainer_step(native_lib):
    """2 scenes x 4096 points, 64 x 64, PyTorch decoder.  DecoderTrainer(mask_weight=0.7, depth_weight=0.3) against the same
    trainer with geometry_loss_fn=geometry_loss_torch (the same render kernels on the same device): the step-0 loss and every
    decoder parameter tensor's gradient in flat relative L2 within the larger of 1e-6 and 4 x the deviation between two runs of
    the torch-expression trainer (the rasterizer backward's atomic-order noise).  With both weights 0 the loss is bit for bit
    that of a trainer constructed without the new arguments -- asserted under an image loss whose sums have one order (see
    below), and to the loss-term bar (rtol 2e-6) under the default fused image loss, whose atomics reorder from run to run."""
    from gaussian_gan_decoder_amd.train import DecoderTrainer, make_scene_batch
    kw = dict(n_scenes_total=2, plane_res=32, plane_channels=32, hidden_dim=128, image_size=64, seed=7)
    batch = make_scene_batch([0, 1], 4096, 64, DEV, seed=0, with_geometry=True)

    def half_step(**extra):
        tr = DecoderTrainer(DEV, **kw, **extra)
        tr.flat_grad.zero_()
        loss = tr.local_loss(batch)
        loss.backward()
        torch.cuda.synchronize()
        grads, off = {}, 0
        names = {id(p): n for n, p in tr.decoder.named_parameters()}
        for p in tr.params:
            if id(p) in names:
                grads[names[id(p)]] = tr.flat_grad[off:off + p.numel()].detach().clone()
            off += p.numel()
        return float(loss.detach()), grads
    on = dict(mask_weight=0.7, depth_weight=0.3)
    l_a, g_a = half_step(geometry_loss_fn=L.geometry_loss_torch, **on)
    l_b, g_b = half_step(geometry_loss_fn=L.geometry_loss_torch, **on)
    l_f, g_f = half_step(**on)
    l_plain, _ = half_step()
    l_zero, _ = half_step(mask_weight=0.0, depth_weight=0.0)
    assert abs(l_zero - l_plain) <= 2e-6 * abs(l_plain), (l_zero, l_plain)
    # bit for bit: under an image loss with one summation order.  fused_image_loss adds its tile sums with float atomics, so the
    # loss of one and the same trainer moves in the last bits from run to run (0.07626796 / 0.07626793 seen for two trainers
    # constructed alike): equality of those two numbers says nothing about the trainer.  torch's reductions have a fixed order.
    ordered = lambda image, target, **_: ((image - target).abs().mean() + (image - target).square().mean(), None)
    l_plain_o, _ = half_step(loss_fn=ordered)
    l_zero_o, _ = half_step(loss_fn=ordered, mask_weight=0.0, depth_weight=0.0)
    assert l_zero_o == l_plain_o, (l_zero_o, l_plain_o)
    assert abs(l_a - l_plain) > 1e-4 * abs(l_plain), "the geometry term must change the loss"
    rel = lambda a, b: float((a - b).norm() / a.norm())
    loss_dev = abs(l_a - l_b) / abs(l_a)
    print(f"\n  loss: torch form {l_a:.8f} / {l_b:.8f}, fused {l_f:.8f}, without the term {l_plain:.8f}")
    assert abs(l_f - l_a) / abs(l_a) <= max(1e-6, 4.0 * loss_dev), (l_f, l_a, loss_dev)
    assert len(g_a) > 0
    bad = []
    for name, a in g_a.items():
        assert float(a.norm()) > 0, name
        dev, err = rel(a, g_b[name]), rel(a, g_f[name])
        print(f"  {name:48s} two torch runs {dev:.2e}  fused against torch {err:.2e}")
        if not err <= max(1e-6, 4.0 * dev):
            bad.append((name, err, dev))
    assert not bad, bad
