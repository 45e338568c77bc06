"""The depth / alpha extension (render_depth_alpha; ggd_forward_aux / ggd_forward_render_aux / ggd_backward_aux) on the GPU.

References from the unchanged oracle (tests/_depth_alpha_ref.py): depth and alpha are the oracle's blend of the pseudo-colour
[z, 1, 0] over a zero background, their gradients the pseudo-colour backward plus the depth term of dL/dmean.  With the
extension on, colour, radii, final_T, n_contrib, the sorted list and num_rendered must be bit-identical to a run with it off."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from _util import (ATOL, adversarial_inputs, assert_blend_matches, check_gradients, decode_result, device_args, run_oracle,
                   same_frame, scene_inputs)
from _depth_alpha_ref import backward_ref, forward_ref
from gaussian_gan_decoder_amd.synthetic import make_dL_dpix

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _native(d, aux=True, raw=False, args=None):
    from gaussian_gan_decoder_amd import rasterizer as R
    args = device_args(d) if args is None else args
    return R.rasterize_gaussians_native(*args, raw, render_depth_alpha=aux)


def _check_forward(d, o, res, what):
    n = decode_result(d, res)
    frag, _ = assert_blend_matches(n, o, what=what)
    ok = ~frag
    depth, alpha = res[6].cpu().numpy()[0], res[7].cpu().numpy()[0]
    Dref, Aref = forward_ref(o)
    assert np.abs(alpha - Aref)[ok].max(initial=0.0) <= 1e-5, what
    assert np.abs(alpha - (1.0 - o["final_T"]))[ok].max(initial=0.0) <= 1e-5, what
    vis = o["radii"] > 0
    zmax = float(np.abs(o["depths"][vis]).max(initial=1.0))
    err = float(np.abs(depth - Dref)[ok].max(initial=0.0))
    assert err <= 1e-5 * zmax, f"{what}: max |ddepth| = {err} (max z {zmax})"
    return n, frag


FWD_SCENES = {
    "adversarial": adversarial_inputs,
    "cube256": lambda: scene_inputs(P=20000, size=256, kind="cube", seed=1),
    "cube512": lambda: scene_inputs(P=60000, size=512, kind="cube", seed=11),
    "shell256-sh3": lambda: scene_inputs(P=20000, size=256, kind="shell", seed=2, sh_degree=3),
    "shell512": lambda: scene_inputs(P=60000, size=512, kind="shell", seed=12),
    "colors_precomp": lambda: scene_inputs(P=20000, size=256, seed=3, use_colors=True),
    "cov3D_precomp": lambda: scene_inputs(P=20000, size=256, kind="shell", seed=4, use_cov=True),
    "96x80": lambda: scene_inputs(P=3000, size=96, width=96, height=80, lsm=-4.0, seed=6),
    "1600-tiles": lambda: scene_inputs(P=30000, size=1280, width=1280, height=320, lsm=-6.5, seed=7),
}


@pytest.mark.parametrize("name", list(FWD_SCENES))
def test_forward_depth_alpha_match_reference(native_lib, name):
    d = FWD_SCENES[name]()
    o = run_oracle(d)
    from gaussian_gan_decoder_amd import _capi
    _capi.context_for(DEV).capacity_hint.clear()
    _check_forward(d, o, _native(d), name + " (exact two-call path)")
    _check_forward(d, o, _native(d), name + " (single-call path)")


def test_forward_with_raw_attributes(native_lib):
    d = scene_inputs(P=20000, size=256, kind="shell", seed=8)
    raw = dict(d, opacities=torch.logit(d["opacities"].double()).float().contiguous(),
               scales=torch.log(d["scales"]).contiguous())
    plain_raw = _native(raw, aux=False, raw=True)
    aux_raw = _native(raw, aux=True, raw=True)
    assert same_frame(plain_raw, aux_raw[:6])
    ref = _native(d, aux=True)
    a, b = decode_result(d, aux_raw), decode_result(d, ref)
    same = a["n_contrib"] == b["n_contrib"]
    assert (~same).sum() <= 2
    for k in (6, 7):
        assert np.abs(aux_raw[k].cpu().numpy()[0] - ref[k].cpu().numpy()[0])[same].max() <= 1e-4


def test_nothing_else_moves(native_lib):
    """Bit-equality of everything the plain forward returns, on the first frame of a shape (exact two-call path), on later
    frames (hinted single call with the speculative sorts), and on a forced capacity overflow (retry path)."""
    from gaussian_gan_decoder_amd import _capi
    d = scene_inputs(P=100000, size=512, kind="cube", seed=21)
    args = device_args(d)
    ctx = _capi.context_for(DEV)
    key = (d["P"], d["W"], d["H"])

    def pair(hint):
        out = []
        for aux in (False, True):
            if hint is None:
                ctx.capacity_hint.pop(key, None)
            else:
                ctx.capacity_hint[key] = hint
            out.append(_native(d, aux=aux, args=args))
        return out

    plain, aux = pair(None)
    assert same_frame(plain, aux[:6]), "first frame"
    R = plain[0]
    assert R > 65537 * 2, R
    for k in range(16):           # enough frames for the flat-streak and two-launch sort speculation to start
        plain, aux = pair(R)
        assert same_frame(plain, aux[:6]), f"hinted frame {k}"
    retries = ctx.capacity_retries
    plain, aux = pair(0)
    assert ctx.capacity_retries == retries + 2, "the overflow path was not taken"
    assert same_frame(plain, aux[:6]), "capacity overflow"


def _backward(d, n, g, gD, gA, raw=False, opacities=None):
    from gaussian_gan_decoder_amd import rasterizer as R
    from gaussian_gan_decoder_amd import _capi
    _capi.context_for(DEV).poison_outputs = True
    t = lambda x: torch.empty(0, device=DEV) if x is None else x.to(DEV)
    outs = R.rasterize_gaussians_backward_native(
        t(d["bg"]), t(d["means3D"]), n["radii"], t(d["colors_precomp"]), t(d["scales"]), t(d["rotations"]),
        d["scale_modifier"], t(d["cov3D_precomp"]), t(d["viewmatrix"]), t(d["projmatrix"]), d["tanfovx"], d["tanfovy"],
        g.to(DEV), t(d["shs"]), d["sh_degree"], t(d["campos"]), n["geom"], n["num_rendered"], n["binning"], n["img"], False,
        raw, None if opacities is None else opacities.to(DEV), dL_ddepth=gD.to(DEV), dL_dalpha=gA.to(DEV))
    torch.cuda.synchronize()
    names = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drots")
    return {k: v.cpu().numpy() for k, v in zip(names, outs)}


def _grads(H, W, mode, seed, frag=None):
    """N(0,1) upstream gradients (colour zero for mode "zero_rgb"), zero on the oracle's fragile pixels `frag` for the HIP
    backward and the reference alike -- as in tests/test_full_size_gpu.py: there a record within 1e-6 of the alpha floor may
    be in or out in the two (1/255 of everything in front of it)."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(3, H, W, generator=gen)
    if mode == "zero_rgb":
        g.zero_()
    gD, gA = torch.randn(1, H, W, generator=gen), torch.randn(1, H, W, generator=gen)
    if frag is not None:
        m = torch.from_numpy(frag)
        g[:, m] = 0.0; gD[:, m] = 0.0; gA[:, m] = 0.0
    return g, gD, gA


@pytest.mark.parametrize("mode", ["random", "zero_rgb"])
@pytest.mark.parametrize("scene", ["adversarial", "cube100k"])
def test_backward_matches_reference(native_lib, scene, mode):
    d = adversarial_inputs() if scene == "adversarial" else scene_inputs(P=100000, size=512, kind="cube", seed=22)
    o = run_oracle(d)
    n, frag_px = _check_forward(d, o, _native(d), scene)
    g, gD, gA = _grads(d["H"], d["W"], mode, 7, frag_px)
    ref, bud, frag = backward_ref(d, o, n, g.numpy(), gD.numpy()[0], gA.numpy()[0])
    got = _backward(d, n, g, gD, gA)
    report = []
    worst = check_gradients(d, got, ref, bud, frag, report=report)
    assert worst <= 1.0, report


def test_backward_with_raw_attributes(native_lib):
    """The depth / alpha backward through the fused activation prologue: the position gradients (which the activations do
    not touch) match those of the same scene rendered with activated attributes."""
    d = scene_inputs(P=100000, size=512, kind="cube", seed=23)
    raw = dict(d, opacities=torch.logit(d["opacities"].double()).float().contiguous(),
               scales=torch.log(d["scales"]).contiguous())
    g, gD, gA = _grads(d["H"], d["W"], "random", 9)
    n = decode_result(d, _native(d))
    nr = decode_result(raw, _native(raw, raw=True))
    a = _backward(d, n, g, gD, gA)
    b = _backward(raw, nr, g, gD, gA, raw=True, opacities=raw["opacities"])
    for k in ("dL_dmeans3D", "dL_dmeans2D", "dL_dcolors"):
        scale = max(1.0, float(np.abs(a[k]).max()))
        assert np.isfinite(b[k]).all(), k
        assert float(np.abs(a[k] - b[k]).max()) <= 1e-4 * scale, k


def test_autograd_end_to_end(native_lib, monkeypatch):
    """render_simple(..., render_depth_alpha=True) under a mean-reduced L1(rgb) + mean|depth - D_t| + mean((alpha - A_t)^2):
    leaf gradients within 1e-5 of the composed reference; a graph that reads only the colour takes today's backward."""
    from gaussian_gan_decoder_amd import rasterizer as Rz
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    from gaussian_gan_decoder_amd.synthetic import make_scene
    S, P = 128, 8000
    sc_cpu = make_scene(P, S, "cube", seed=5, log_scale_mean=-5.0)
    sc = sc_cpu.to(DEV)
    pc = sc.gaussian_model(requires_grad=True)
    calls = []
    real = Rz.rasterize_gaussians_backward_native
    monkeypatch.setattr(Rz, "rasterize_gaussians_backward_native",
                        lambda *a, **k: (calls.append(sorted(k)), real(*a, **k))[1])
    out = render_simple(sc.cam, pc, bg_color=sc.bg, render_depth_alpha=True)
    assert out["depth"].shape == (1, S, S) and out["alpha"].shape == (1, S, S)
    gen = torch.Generator().manual_seed(3)
    t_rgb, t_D, t_A = torch.rand(3, S, S, generator=gen), 4.0 * torch.rand(1, S, S, generator=gen), torch.rand(1, S, S, generator=gen)
    loss = (out["render"] - t_rgb.to(DEV)).abs().mean() + (out["depth"] - t_D.to(DEV)).abs().mean() + \
        ((out["alpha"] - t_A.to(DEV)) ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    assert calls == [["dL_dalpha", "dL_ddepth"]]
    cpu = lambda t: t.detach().cpu()
    cam = sc_cpu.cam
    d = dict(P=P, W=S, H=S, sh_degree=0, scale_modifier=1.0, tanfovx=math.tan(cam.FoVx * 0.5),
             tanfovy=math.tan(cam.FoVy * 0.5), means3D=sc_cpu.xyz, opacities=cpu(pc.get_opacity),
             viewmatrix=cam.world_view_transform.contiguous(), projmatrix=cam.full_proj_transform.contiguous(),
             campos=cam.camera_center, bg=sc_cpu.bg, shs=sc_cpu.features_dc.contiguous(), colors_precomp=None,
             scales=cpu(pc.get_scaling).contiguous(), rotations=cpu(pc.get_rotation).contiguous(), cov3D_precomp=None)
    o = run_oracle(d)
    n = decode_result(d, _native(d))
    HW = S * S
    g_rgb = (torch.sign(cpu(out["render"]) - t_rgb) / (3 * HW)).numpy()
    g_D = (torch.sign(cpu(out["depth"]) - t_D) / HW).numpy()[0]
    g_A = (2.0 * (cpu(out["alpha"]) - t_A) / HW).numpy()[0]
    ref, _, frag = backward_ref(d, o, n, g_rgb, g_D, g_A)
    ok = frag == 0
    for got, r in ((cpu(pc._xyz.grad).numpy(), ref["dL_dmeans3D"]), (cpu(pc._features_dc.grad).numpy(), ref["dL_dsh"]),
                   (cpu(out["viewspace_points"].grad).numpy(), ref["dL_dmeans2D"])):
        err = float(np.abs(got.reshape(r.shape) - r)[ok].max())
        assert err <= ATOL, err
    # only the colour is read: today's backward (no aux gradients reach the wrapper)
    calls.clear()
    out = render_simple(sc.cam, pc, bg_color=sc.bg, render_depth_alpha=True)
    (out["render"] * make_dL_dpix(S).to(DEV)).sum().backward()
    assert calls == [[]]


def test_full_size_shipped_path(native_lib):
    """1 M Gaussians at 1024^2 (cube) on the shipped single-call path: forward parity and one backward within budget."""
    from gaussian_gan_decoder_amd import _capi
    d = scene_inputs(P=1_000_000, size=1024, kind="cube", seed=0)
    o = run_oracle(d)
    _native(d)                                        # first frame of the shape: leaves the capacity hint
    res = _native(d)
    assert _capi.context_for(DEV).capacity_hint.get((d["P"], d["W"], d["H"])) is not None
    n, frag_px = _check_forward(d, o, res, "1M / 1024^2")
    g, gD, gA = _grads(d["H"], d["W"], "random", 11, frag_px)
    ref, bud, frag = backward_ref(d, o, n, g.numpy(), gD.numpy()[0], gA.numpy()[0])
    got = _backward(d, n, g, gD, gA)
    report = []
    assert check_gradients(d, got, ref, bud, frag, report=report) <= 1.0, report
