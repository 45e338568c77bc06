"""The anti-aliasing option (ggd_params.antialiasing: the opacity-compensated 2D filter) on the GPU.

References are composed from the unchanged oracle and the fp64 helper tests/_antialias_ref.py: the forward is the oracle's
forward with every opacity replaced by o_eff = o h; the backward is the oracle's fp64 backward at o_eff with its dL/do_eff
replaced by dL/do = dL/do_eff h and the h chain added to the geometric gradients.  Everything that does not depend on the
opacity (radii, rect, tiles_touched, depth keys, the sorted list and ranges, the records' conic / centre / colour) must be
bit-identical to the plain render of the same inputs."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import _antialias_ref as AA
from _util import (ATOL, EPS32, adversarial_inputs, assert_blend_matches, backward_reference, check_gradients, decode_result,
                   device_args, run_oracle, same_frame, scene_inputs)
from _depth_alpha_ref import backward_ref as depth_alpha_backward_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _native(d, aa=True, raw=False, aux=False, args=None, **kw):
    from gaussian_gan_decoder_amd import rasterizer as R
    args = device_args(d) if args is None else args
    if aa is None:
        return R.rasterize_gaussians_native(*args, raw, render_depth_alpha=aux, **kw)
    return R.rasterize_gaussians_native(*args, raw, render_depth_alpha=aux, antialiasing=aa, **kw)


def _faint():
    """many Gaussians whose o_eff falls below 1/255 (never blended) next to ones just above it"""
    d = scene_inputs(P=20000, size=256, kind="cube", seed=31, lsm=-6.5)
    return dict(d, opacities=(0.05 * d["opacities"]).contiguous())


FWD_SCENES = {
    "sh0": lambda: scene_inputs(P=20000, size=256, kind="cube", seed=1),
    "sh3": lambda: scene_inputs(P=20000, size=256, kind="shell", seed=2, sh_degree=3),
    "colors_precomp": lambda: scene_inputs(P=20000, size=256, seed=3, use_colors=True),
    "cov3D_precomp": lambda: scene_inputs(P=20000, size=256, kind="shell", seed=4, use_cov=True),
    "scale_modifier": lambda: scene_inputs(P=20000, size=256, kind="cube", seed=5, scale_modifier=0.6),
    "adversarial": adversarial_inputs,
    "o_eff_below_floor": _faint,
}


def _same_geometry(a, b, what, sh=True):
    """everything of two decoded forwards that does not depend on the opacity, bit for bit (`clamped` is only written
    when the colour comes from SH)"""
    assert a["num_rendered"] == b["num_rendered"], what
    np.testing.assert_array_equal(a["radii"].cpu().numpy(), b["radii"].cpu().numpy(), err_msg=what)
    vis = b["radii"].cpu().numpy() > 0
    for k in ("tiles_touched", "point_offsets", "rect", "depths", "point_list", "ranges"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    for k in ("xy", "rgb"):
        np.testing.assert_array_equal(a[k][vis], b[k][vis], err_msg=f"{what}: {k}")
    np.testing.assert_array_equal(a["conic_opacity"][vis, :3], b["conic_opacity"][vis, :3], err_msg=f"{what}: conic")
    if sh:
        np.testing.assert_array_equal(a["clamped"], b["clamped"], err_msg=f"{what}: clamped")
    return vis


def _check_record_opacity(d, n, vis, what):
    """the records' opacity is the helper's o_eff within the fp32 rounding of h (det0 = x y - z^2 cancels: cond)"""
    oe = AA.o_eff(d)
    _, cond = AA.h_and_conditioning(d)
    got = n["conic_opacity"][:, 3].astype(np.float64)
    err = np.abs(got - oe)[vis]
    tol = 16.0 * EPS32 * cond[vis] * np.abs(oe[vis]) + 1e-30
    assert (err <= tol).all(), f"{what}: record opacity off by up to {float((err / tol).max()):.2f} x its bound"
    return oe


# The fp32 kernels know o_eff only to about cond ulps (det0 = x y - z^2 cancels; cond from h_and_conditioning).  A blend decision
# moves once alpha = o_eff G moves by more than the 1e-6 window of the oracle's fragile-pixel mask, i.e. o_eff by ~2.5e-4 of
# itself near the 1/255 floor: far beyond cond ulps while cond <= 1e3.  Above that -- the needles of adversarial_inputs reach
# 1.5e8, the random scenes stay below 120 -- the fp32 h is not pinned by the formula, so the blend comparison takes the
# kernel's value there (checked against the helper within its bound by _check_record_opacity) and the helper's everywhere else
COND_MAX = 1e3


def _oracle_opacities(d, n):
    """the opacities the composed oracle blends with: the helper's o_eff, the GPU record's where h is ill-conditioned"""
    oe = AA.o_eff(d)
    _, cond = AA.h_and_conditioning(d)
    vis = n["radii"].cpu().numpy() > 0
    use_gpu = vis & (cond > COND_MAX)
    op = np.where(use_gpu, n["conic_opacity"][:, 3], oe).astype(np.float32)
    return torch.from_numpy(op).reshape(d["opacities"].shape).contiguous()


@pytest.mark.parametrize("name", list(FWD_SCENES))
def test_forward_matches_composed_oracle(native_lib, name):
    from gaussian_gan_decoder_amd import _capi
    d = FWD_SCENES[name]()
    sh = d["shs"] is not None
    o, first = None, None
    for path in ("exact two-call path", "single-call path"):
        if path.startswith("exact"):
            _capi.context_for(DEV).capacity_hint.clear()
        res = _native(d, aa=True)
        aa = decode_result(d, res)
        plain = decode_result(d, _native(d, aa=False))
        vis = _same_geometry(aa, plain, f"{name} ({path})", sh)
        _check_record_opacity(d, aa, vis, f"{name} ({path})")
        if o is None:
            o = run_oracle(dict(d, opacities=_oracle_opacities(d, aa)))
            first = res
        else:
            assert same_frame(res, first), f"{name}: the two paths differ"
        np.testing.assert_array_equal(aa["radii"].cpu().numpy(), o["radii"])
        assert_blend_matches(aa, o, what=f"{name} ({path})")
        assert not torch.equal(aa["color"], plain["color"]), "the filter changed nothing"
    if name == "o_eff_below_floor":
        oe = AA.o_eff(d)
        assert ((oe < 1.0 / 255.0) & vis).sum() > 1000 and ((oe >= 1.0 / 255.0) & vis).sum() > 1000


def test_forward_with_raw_attributes(native_lib):
    """fused sigmoid / exp / normalize: the same records (up to the activations' own rounding) as with activated inputs"""
    d = scene_inputs(P=20000, size=256, kind="shell", seed=8)
    raw = dict(d, opacities=torch.logit(d["opacities"].double()).float().contiguous(),
               scales=torch.log(d["scales"]).contiguous())
    a = decode_result(d, _native(raw, raw=True))
    b = decode_result(d, _native(d))
    vis = b["radii"].cpu().numpy() > 0
    np.testing.assert_array_equal(a["radii"].cpu().numpy(), b["radii"].cpu().numpy())
    rel = np.abs(a["conic_opacity"][vis, 3] - b["conic_opacity"][vis, 3]) / b["conic_opacity"][vis, 3]
    assert float(rel.max()) <= 1e-5, float(rel.max())
    _check_record_opacity(d, a, vis, "raw attributes")
    same = a["n_contrib"] == b["n_contrib"]
    assert (~same).sum() <= 2
    assert float(np.abs(a["color"].cpu().numpy() - b["color"].cpu().numpy())[:, same].max()) <= 1e-4


def test_off_means_off(native_lib):
    """antialiasing=False is the call without the keyword, bit for bit: first frame (two-call path) and hinted frames."""
    from gaussian_gan_decoder_amd import _capi
    d = scene_inputs(P=100000, size=512, kind="cube", seed=21)
    args = device_args(d)
    ctx = _capi.context_for(DEV)
    ctx.capacity_hint.pop((d["P"], d["W"], d["H"]), None)
    for k in range(12):
        a, b = _native(d, aa=None, args=args), _native(d, aa=False, args=args)
        assert same_frame(a, b), f"frame {k}"
        da, db = decode_result(d, a), decode_result(d, b)
        vis = _same_geometry(da, db, f"frame {k}")
        np.testing.assert_array_equal(da["conic_opacity"][vis], db["conic_opacity"][vis])
        for key in ("power_threshold", "cull_extent"):
            np.testing.assert_array_equal(da[key][vis], db[key][vis])
        on = _native(d, aa=True, args=args)
        assert on[0] == a[0] and torch.equal(on[2], a[2]) and not torch.equal(on[1], a[1])


def _grads(H, W, seed, frag=None, aux=False):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(3, H, W, generator=gen)
    gD, gA = torch.randn(1, H, W, generator=gen), torch.randn(1, H, W, generator=gen)
    if frag is not None:
        m = torch.from_numpy(frag)
        g[:, m] = 0.0; gD[:, m] = 0.0; gA[:, m] = 0.0
    return (g, gD, gA) if aux else (g, None, None)


def _backward(d, n, g, gD=None, gA=None, raw=False, opacities=None, aa=True):
    from gaussian_gan_decoder_amd import rasterizer as R
    from gaussian_gan_decoder_amd import _capi
    _capi.context_for(DEV).poison_outputs = True
    t = lambda x: torch.empty(0, device=DEV) if x is None else x.to(DEV)
    kw = dict(dL_ddepth=gD.to(DEV), dL_dalpha=gA.to(DEV)) if gD is not None else {}
    outs = R.rasterize_gaussians_backward_native(
        t(d["bg"]), t(d["means3D"]), n["radii"], t(d["colors_precomp"]), t(d["scales"]), t(d["rotations"]),
        d["scale_modifier"], t(d["cov3D_precomp"]), t(d["viewmatrix"]), t(d["projmatrix"]), d["tanfovx"], d["tanfovy"],
        g.to(DEV), t(d["shs"]), d["sh_degree"], t(d["campos"]), n["geom"], n["num_rendered"], n["binning"], n["img"], False,
        raw, (d["opacities"] if opacities is None else opacities).to(DEV), antialiasing=aa, **kw)
    torch.cuda.synchronize()
    names = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drots")
    return {k: v.cpu().numpy() for k, v in zip(names, outs)}


def _gpu_opacity_inputs(d, n):
    """d with the opacities the GPU's records carry (o_eff in fp32) where visible: the oracle then blends exactly what the
    GPU blended, and backward_reference's bit-exact checks of the records hold"""
    vis = n["radii"].cpu().numpy() > 0
    op = np.where(vis, n["conic_opacity"][:, 3], d["opacities"].numpy().reshape(-1)).astype(np.float32)
    return dict(d, opacities=torch.from_numpy(op).reshape(d["opacities"].shape).contiguous())


def composed_reference(d, n, seed, aux=False):
    """(ref, budget, fragile, g, gD, gA) of the anti-aliasing backward for the AA forward n of d"""
    d_g = _gpu_opacity_inputs(d, n)
    o = run_oracle(d_g)
    frag_px, _ = assert_blend_matches(n, o, what="AA forward for the backward")
    g, gD, gA = _grads(d["H"], d["W"], seed, frag_px, aux)
    if aux:
        ref, bud, frag = depth_alpha_backward_ref(d_g, o, n, g.numpy(), gD.numpy()[0], gA.numpy()[0])
    else:
        ref, bud, frag = backward_reference(d_g, o, n, g.numpy())
    ref, bud = AA.compose_backward(d, ref, bud)
    return ref, bud, frag, g, gD, gA


BWD_SCENES = {
    "plain": lambda: scene_inputs(P=60000, size=384, kind="cube", seed=41),
    "cov3D_precomp": lambda: scene_inputs(P=40000, size=256, kind="shell", seed=42, use_cov=True),
    "sh3": lambda: scene_inputs(P=40000, size=256, kind="shell", seed=43, sh_degree=3),
    "scale_modifier": lambda: scene_inputs(P=40000, size=256, kind="cube", seed=44, scale_modifier=0.7),
    "adversarial": adversarial_inputs,
}


BWD_CASES = [(name, False) for name in BWD_SCENES] + [("plain", True), ("adversarial", True)]


@pytest.mark.parametrize("name,aux", BWD_CASES, ids=[f"{n}-{'depth_alpha' if a else 'rgb'}" for n, a in BWD_CASES])
def test_backward_matches_composed_reference(native_lib, name, aux):
    d = BWD_SCENES[name]()
    n = decode_result(d, _native(d, aux=aux))
    ref, bud, frag, g, gD, gA = composed_reference(d, n, seed=7, aux=aux)
    got = _backward(d, n, g, gD, gA)
    report = []
    worst = check_gradients(d, got, ref, bud, frag, report=report)
    assert worst <= 1.0, report
    # the h chain is really in there: the plain backward of the same frame differs
    plain = _backward(d, n, g, gD, gA, aa=False)
    assert np.abs(plain["dL_dopacity"] - got["dL_dopacity"]).max() > 1e-6
    assert np.abs(plain["dL_dmeans3D"] - got["dL_dmeans3D"]).max() > 1e-6


def test_backward_with_raw_attributes(native_lib):
    """the AA backward through the fused activations: the gradients equal those of the activated inputs pushed through
    the activations' Jacobians (the h chain sits before them)"""
    d = scene_inputs(P=60000, size=384, kind="cube", seed=45)
    raw = dict(d, opacities=torch.logit(d["opacities"].double()).float().contiguous(),
               scales=torch.log(d["scales"]).contiguous())
    g, _, _ = _grads(d["H"], d["W"], 9)
    n = decode_result(d, _native(d))
    nr = decode_result(raw, _native(raw, raw=True))
    same = n["n_contrib"] == nr["n_contrib"]
    g[:, torch.from_numpy(~same)] = 0.0
    a = _backward(d, n, g)
    b = _backward(raw, nr, g, raw=True)
    s = d["opacities"].double().numpy().reshape(-1, 1)
    expect = {"dL_dmeans3D": a["dL_dmeans3D"], "dL_dmeans2D": a["dL_dmeans2D"], "dL_dcolors": a["dL_dcolors"],
              "dL_dopacity": a["dL_dopacity"] * s * (1.0 - s), "dL_dscales": a["dL_dscales"] * d["scales"].double().numpy()}
    for k, e in expect.items():
        scale = max(1.0, float(np.abs(e).max()))
        assert np.isfinite(b[k]).all(), k
        assert float(np.abs(e - b[k]).max()) <= 2e-4 * scale, (k, float(np.abs(e - b[k]).max()), scale)


def test_backward_needs_the_opacities(native_lib):
    """the C ABI refuses an AA backward without opacities (GGD_E_INVALID) and writes nothing"""
    import ctypes as C
    from gaussian_gan_decoder_amd import _capi, rasterizer as R
    d = scene_inputs(P=2000, size=64, seed=46)
    n = decode_result(d, _native(d))
    ctx = _capi.context_for(DEV)
    keep = []
    rs = R.GaussianRasterizationSettings(d["H"], d["W"], d["tanfovx"], d["tanfovy"], d["bg"].to(DEV), 1.0,
                                         d["viewmatrix"].to(DEV), d["projmatrix"].to(DEV), 0, d["campos"].to(DEV), False,
                                         False, antialiasing=True)
    prm = R._params(rs, d["P"], 1, DEV, keep)
    assert prm.antialiasing == 1
    t = {k: d[k].to(DEV).contiguous() for k in ("means3D", "shs", "scales", "rotations")}
    P = d["P"]
    outs = [torch.zeros(sh, device=DEV) for sh in ((P, 3), (P, 3), (P, 1), (P, 3), (P, 6), (P, 1, 3), (P, 3), (P, 4))]
    gpix = torch.zeros(3, d["H"], d["W"], device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = ctx.lib.ggd_backward(ctx.handle, C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream), C.byref(prm),
                              p(t["means3D"]), p(t["shs"]), None, None, p(t["scales"]), p(t["rotations"]), None,
                              p(n["radii"]), p(n["geom"]), p(n["binning"]), p(n["img"]), n["num_rendered"], p(gpix),
                              *[p(x) for x in outs])
    assert rc == -1, rc
    assert "opacities" in ctx.lib.ggd_last_error(ctx.handle).decode()


@pytest.mark.parametrize("fused", [False, True], ids=["torch-getters", "fused-activations"])
@pytest.mark.parametrize("aux", [False, True], ids=["rgb", "depth_alpha"])
def test_autograd_end_to_end(native_lib, fused, aux):
    """render_simple(..., antialiasing=True) under sum(rgb * g) (+ depth / alpha terms): leaf gradients against the composed
    reference of test_backward_matches_composed_reference"""
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    from gaussian_gan_decoder_amd.synthetic import make_scene
    S, P = 128, 8000
    sc_cpu = make_scene(P, S, "cube", seed=5, log_scale_mean=-5.0)
    sc = sc_cpu.to(DEV)
    pc = sc.gaussian_model(requires_grad=True)
    out = render_simple(sc.cam, pc, bg_color=sc.bg, fused_activations=fused, render_depth_alpha=aux, antialiasing=True)
    cpu = lambda t: t.detach().cpu()
    cam = sc_cpu.cam
    d = dict(P=P, W=S, H=S, sh_degree=0, scale_modifier=1.0, tanfovx=math.tan(cam.FoVx * 0.5),
             tanfovy=math.tan(cam.FoVy * 0.5), means3D=sc_cpu.xyz, opacities=cpu(pc.get_opacity).contiguous(),
             viewmatrix=cam.world_view_transform.contiguous(), projmatrix=cam.full_proj_transform.contiguous(),
             campos=cam.camera_center, bg=sc_cpu.bg, shs=sc_cpu.features_dc.contiguous(), colors_precomp=None,
             scales=cpu(pc.get_scaling).contiguous(), rotations=cpu(pc.get_rotation).contiguous(), cov3D_precomp=None)
    n = decode_result(d, _native(d, aux=aux))
    ref, _, frag, g, gD, gA = composed_reference(d, n, seed=3, aux=aux)
    loss = (out["render"] * g.to(DEV)).sum()
    if aux:
        loss = loss + (out["depth"] * gD.to(DEV)).sum() + (out["alpha"] * gA.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    ok = frag == 0
    s = d["opacities"].double().numpy().reshape(-1)
    checks = ((cpu(pc._xyz.grad).numpy(), ref["dL_dmeans3D"], "xyz"),
              (cpu(pc._features_dc.grad).numpy(), ref["dL_dsh"], "features_dc"),
              (cpu(out["viewspace_points"].grad).numpy(), ref["dL_dmeans2D"], "means2D"),
              (cpu(pc._opacity.grad).numpy().reshape(-1), ref["dL_dopacity"].reshape(-1) * s * (1.0 - s), "opacity logit"))
    for got, r, what in checks:
        err = float(np.abs(got.reshape(r.shape) - r)[ok].max())
        tol = ATOL + 2e-4 * float(np.abs(r).max())
        assert err <= tol, (what, err, tol)


def test_filter_matches_its_purpose(native_lib):
    """One isotropic Gaussian of 2D variance 0.25 px^2 (std 0.5 px): with the filter its alpha mass is that of the
    UNDILATED footprint, 2 pi o sqrt(det0); without it that of the dilated one, 2 pi o sqrt(det1) -- the zoom-out artefact."""
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    from gaussian_gan_decoder_amd.synthetic import make_camera
    S = 65                                   # odd: the image centre is a pixel centre
    cam = make_camera(S, 12.0, device=DEV)   # looks at the origin from 2.7
    fx = S / (2.0 * math.tan(cam.FoVx * 0.5))
    s = 0.5 * 2.7 / fx                       # 3D std that projects to 0.5 px
    o = 0.8
    pc = GaussianModel(0)
    pc._xyz = torch.zeros(1, 3, device=DEV)
    pc._scaling = torch.full((1, 3), math.log(s), device=DEV)
    pc._rotation = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=DEV)
    pc._opacity = torch.logit(torch.tensor([[o]], dtype=torch.float64)).float().to(DEV)
    pc._features_dc = torch.ones(1, 1, 3, device=DEV)
    bg = torch.zeros(3, device=DEV)
    mass = {}
    for aa in (False, True):
        out = render_simple(cam, pc, bg_color=bg, render_depth_alpha=True, antialiasing=aa)
        mass[aa] = float(out["alpha"].detach().sum())
    d = dict(W=S, H=S, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
             viewmatrix=cam.world_view_transform.cpu(), means3D=torch.zeros(1, 3), scales=torch.full((1, 3), s),
             rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]]), scale_modifier=1.0, cov3D_precomp=None)
    m, _, _, cov6 = AA._inputs(d, False)
    x, z, y = (float(v) for v in AA.cov2d(d, m, cov6))
    assert abs(x - 0.25) < 0.01 and abs(y - 0.25) < 0.01 and abs(z) < 1e-6
    det0, det1 = x * y - z * z, (x + 0.3) * (y + 0.3) - z * z
    want_aa, want_plain = 2 * math.pi * o * math.sqrt(det0), 2 * math.pi * o * math.sqrt(det1)
    assert abs(mass[True] / want_aa - 1.0) <= 0.03, (mass, want_aa)
    assert abs(mass[False] / want_plain - 1.0) <= 0.03, (mass, want_plain)
    assert mass[False] > 1.8 * mass[True], mass


def _pose(d, h, v, fov_deg=12.0):
    from gaussian_gan_decoder_amd.synthetic import make_camera
    cam = make_camera(d["W"], fov_deg, h, v)
    return dict(d, viewmatrix=cam.world_view_transform.contiguous(), projmatrix=cam.full_proj_transform.contiguous(),
                campos=cam.camera_center.contiguous(), tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5))


def test_full_size_shipped_path(native_lib):
    """1 M Gaussians at 1024^2 along a slowly moving camera on the shipped single-call forward: the two-launch depth sort must
    run, the last frame (one of its frames) matches the composed oracle, and its AA backward runs and differs from the plain."""
    from gaussian_gan_decoder_amd import _capi, rasterizer as R
    base = scene_inputs(P=1_000_000, size=1024, kind="cube", seed=0)
    ctx = _capi.context_and_stream(DEV)[0]
    ctx.set_option(_capi.OPT_BINNING, 1)
    ctx.set_option(_capi.OPT_MSD_SORT, 1)
    m0 = ctx.get_option(_capi.STAT_MSD_FRAMES)
    frames = [_pose(base, math.pi / 2 + 0.004 * k, math.pi / 2 - 0.002 * k) for k in range(24)]
    dev_base = device_args(base)
    res = None
    for k, d in enumerate(frames):
        args = list(dev_base)
        args[8], args[9], args[10], args[11], args[16] = (d["viewmatrix"].to(DEV), d["projmatrix"].to(DEV), d["tanfovx"],
                                                          d["tanfovy"], d["campos"].to(DEV))
        before = ctx.get_option(_capi.STAT_MSD_FRAMES)
        res = R.rasterize_gaussians_native(*args, False, antialiasing=True)
        last_msd = ctx.get_option(_capi.STAT_MSD_FRAMES) > before
    assert ctx.get_option(_capi.STAT_MSD_FRAMES) >= m0 + 4, "the two-launch sort never ran"
    assert last_msd, "the last frame did not use the two-launch sort"
    d = frames[-1]
    n = decode_result(d, res)
    o = run_oracle(dict(d, opacities=_oracle_opacities(d, n)))
    np.testing.assert_array_equal(n["radii"].cpu().numpy(), o["radii"])
    np.testing.assert_array_equal(n["point_list"], o["point_list"])
    np.testing.assert_array_equal(n["ranges"], o["ranges"])
    vis = o["radii"] > 0
    _check_record_opacity(d, n, vis, "1M / 1024^2")
    frag, _ = assert_blend_matches(n, o, what="1M / 1024^2 AA, two-launch-sort frame")
    g, _, _ = _grads(d["H"], d["W"], 11, frag)
    got = _backward(d, n, g)
    plain = _backward(d, n, g, aa=False)
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    assert np.abs(got["dL_dopacity"] - plain["dL_dopacity"]).max() > 1e-6


def test_frame_pipeline_with_antialiasing(native_lib):
    """FramePipeline.submit(..., antialiasing=True): every collected frame is the direct AA render, not the plain one"""
    from gaussian_gan_decoder_amd import rasterizer as R
    d = scene_inputs(P=200_000, size=512, kind="cube", seed=51)
    args = device_args(d)
    ref = _native(d, args=args)
    plain = _native(d, aa=False, args=args)
    assert not torch.equal(ref[1], plain[1])
    pipe = R.FramePipeline(DEV, slots=2)
    got = []
    for _ in range(10):
        r_ = pipe.submit(*args, antialiasing=True)
        if r_ is not None:
            got.append(r_)
    got += pipe.drain()
    assert len(got) == 10
    for i, r_ in enumerate(got):
        r_[-1].synchronize()
        assert same_frame(r_, ref), f"pipelined frame {i}"
    assert pipe.synchronous_frames < 10, "no frame took the enqueue / collect route"


def test_trainer_step_with_antialiasing(native_lib):
    """one DecoderTrainer step with antialiasing=True: finite loss and gradients, and not the gradients of the plain step"""
    from gaussian_gan_decoder_amd.train import DecoderTrainer, make_scene_batch
    cfg = dict(plane_res=32, plane_channels=32, hidden_dim=128, image_size=64, seed=7)

    def make(aa):
        tr = DecoderTrainer(DEV, n_scenes_total=2, fused_activations=True, antialiasing=aa, backbone_params=3000,
                            perceptual_weight=0.05, perceptual_width_div=16, **cfg)
        with torch.no_grad():   # splats large enough for the 64 x 64 image to see them (as tests/test_train_step_gpu.py)
            tr.decoder.scale_decoder.backbone[-1].bias += 3.5
            tr.decoder.opacity_decoder.backbone[-1].bias += 1.0
        return tr
    batch = make_scene_batch([0, 1], 2000, cfg["image_size"], DEV, seed=0)
    grads, losses = {}, {}
    for aa in (False, True):
        tr = make(aa)
        assert tr.render_kwargs.get("antialiasing", False) is aa
        tr.flat_grad.zero_()
        loss = tr.local_loss(batch)
        loss.backward()
        torch.cuda.synchronize()
        losses[aa], grads[aa] = float(loss.detach()), tr.flat_grad.detach().clone()
        assert math.isfinite(losses[aa]) and torch.isfinite(grads[aa]).all()
        assert float(grads[aa].abs().max()) > 0.0
    assert losses[True] != losses[False]
    rel = float((grads[True] - grads[False]).norm() / grads[False].norm())
    assert rel > 1e-4, rel
