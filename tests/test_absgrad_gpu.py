"""The absgrad extension (GaussianRasterizationSettings(absgrad=True); ggd_backward_abs) on the GPU: means2D.absgrad, the sum
over pixels of the ABSOLUTE per-pixel screen-space gradient contributions, against the float64 restatement of
tests/_absgrad_ref.py (vouched for by tests/test_absgrad_host.py) under the unchanged oracle's budget for dL_dmeans2D and
tests/_util.py's ATOL / KAPPA.  Every backward here runs with poison_outputs: the library writes every element itself.
Each test prints its measured figures before it asserts."""
from __future__ import annotations

import contextlib
import math

import numpy as np
import pytest
import torch

import _absgrad_ref as AG
import _instance_cases as IC
from _util import (ATOL, EPS32, KAPPA, assert_blend_matches, check_gradients, decode_result, device_args, run_oracle)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drots",
         "dL_dmeans2D_abs")


def _forward(d, aux=False, aa=False, raw=False):
    from gaussian_gan_decoder_amd import rasterizer as R
    kw = dict(antialiasing=True) if aa else {}
    return R.rasterize_gaussians_native(*device_args(d), raw, render_depth_alpha=aux, **kw)


def _backward(d, n, g, gD=None, gA=None, raw=False, aa=False, absgrad=True):
    from gaussian_gan_decoder_amd import _capi, rasterizer as R
    _capi.context_for(DEV).poison_outputs = True
    t = lambda x: torch.empty(0, device=DEV) if x is None else x.to(DEV)
    kw = dict(dL_ddepth=gD.to(DEV), dL_dalpha=gA.to(DEV)) if gD is not None else {}
    if aa:
        kw["antialiasing"] = True
    if absgrad:
        kw["absgrad"] = True
    outs = R.rasterize_gaussians_backward_native(
        t(d["bg"]), t(d["means3D"]), n["radii"], t(d["colors_precomp"]), t(d["scales"]), t(d["rotations"]),
        d["scale_modifier"], t(d["cov3D_precomp"]), t(d["viewmatrix"]), t(d["projmatrix"]), d["tanfovx"], d["tanfovy"],
        g.to(DEV), t(d["shs"]), d["sh_degree"], t(d["campos"]), n["geom"], n["num_rendered"], n["binning"], n["img"], False,
        raw, d["opacities"].to(DEV) if (raw or aa) else None, **kw)
    torch.cuda.synchronize()
    assert len(outs) == (9 if absgrad else 8)
    return {k: v.cpu().numpy() for k, v in zip(NAMES, outs)}


@contextlib.contextmanager
def _options(**opts):
    from gaussian_gan_decoder_amd import _capi
    ctx = _capi.context_for(DEV)
    keys = dict(exp_mode=_capi.OPT_EXP_MODE, cull=_capi.OPT_BLEND_CULL, split=_capi.OPT_BLEND_SPLIT)
    saved = {k: ctx.get_option(keys[k]) for k in opts}
    try:
        for k, v in opts.items():
            ctx.set_option(keys[k], v)
        yield ctx
    finally:
        for k, v in saved.items():
            ctx.set_option(keys[k], v)


def _check(d, got, ref, bud, frag, what):
    """tests/_util.py::check_gradients' rule over the eight signed arrays and dL_dmeans2D_abs; returns the worst ratios"""
    assert got["dL_dmeans2D_abs"].shape == (d["P"], 3) and got["dL_dmeans2D_abs"].dtype == np.float32
    assert np.isfinite(got["dL_dmeans2D_abs"]).all(), f"{what}: an element of absgrad was never written"
    assert (got["dL_dmeans2D_abs"] >= 0).all() and (got["dL_dmeans2D_abs"][:, 2] == 0).all()
    report = []
    worst = check_gradients(d, got, ref, bud, frag, report=report)
    worst_abs = next(r["worst_ratio"] for r in report if r["array"] == "dL_dmeans2D_abs")
    print(f"[absgrad] {what}: worst error / bound {worst:.3f} (absgrad {worst_abs:.3f}), max absgrad "
          f"{np.abs(ref['dL_dmeans2D_abs']).max():.3e}, max |signed| {np.abs(ref['dL_dmeans2D']).max():.3e}")
    assert worst <= 1.0, report
    return worst, worst_abs


# ---- crafted cases: camera at the origin looking down +z, tan(fov / 2) = 1, background 0, dL/dpix = 1 ----------------------
def _crafted(W, H, xyz, opacity, scale, colors):
    P = len(xyz)
    zf, zn = 100.0, 0.01
    proj = torch.zeros(4, 4)
    proj[0, 0] = proj[1, 1] = 1.0
    proj[2, 2], proj[2, 3], proj[3, 2] = zf / (zf - zn), 1.0, -(zf * zn) / (zf - zn)
    rot = torch.zeros(P, 4); rot[:, 0] = 1.0
    return dict(P=P, W=W, H=H, sh_degree=0, scale_modifier=1.0, tanfovx=1.0, tanfovy=1.0,
                means3D=torch.tensor(xyz, dtype=torch.float32).reshape(P, 3), opacities=torch.full((P, 1), float(opacity)),
                viewmatrix=torch.eye(4), projmatrix=proj.contiguous(), campos=torch.zeros(3), bg=torch.zeros(3), shs=None,
                colors_precomp=colors.reshape(P, 3).float().contiguous(), scales=torch.full((P, 3), float(scale)),
                rotations=rot, cov3D_precomp=None)


def _run_crafted(d, what):
    o = run_oracle(d)
    n = decode_result(d, _forward(d))
    assert_blend_matches(n, o, what=what)
    g = torch.ones(3, d["H"], d["W"])
    ref, bud, frag, _ = AG.reference(d, o, n, g.numpy())
    got = _backward(d, n, g)
    return o, got, ref, bud, frag


def test_symmetric_gaussian_signed_cancels_absolute_does_not(native_lib):
    """one isotropic Gaussian centred at (7.5, 7.5) of a 16 x 16 image: the per-pixel contributions cancel in pairs, so the signed
    gradient vanishes; the absolute one is the reference's and far from zero.  The signed gradient cannot pass this."""
    d = _crafted(16, 16, [[0.0, 0.0, 4.0]], 0.8, 1.0, torch.tensor([[0.9, 0.5, 0.2]]))
    o, got, ref, bud, frag = _run_crafted(d, "centred")
    np.testing.assert_array_equal(o["xy"][0], np.float32([7.5, 7.5]))
    assert int(frag.sum()) == 0
    _check(d, got, ref, bud, frag, "centred 16 x 16")
    signed, absg = got["dL_dmeans2D"][0, :2], got["dL_dmeans2D_abs"][0, :2]
    print(f"[absgrad] centred: signed {signed}, absgrad {absg}, reference {ref['dL_dmeans2D_abs'][0, :2]}")
    assert (np.abs(signed) <= 1e-5).all()
    assert (absg > 1e-3).all() and (ref["dL_dmeans2D_abs"][0, :2] > 1e-3).all()


def test_gaussian_on_the_corner_of_four_tiles(native_lib):
    """the same Gaussian centred at (16, 16) of a 32 x 32 image: four tiles, sixteen waves -- the cross-wave and cross-tile atomics"""
    d = _crafted(32, 32, [[0.125, 0.125, 4.0]], 0.8, 1.0, torch.tensor([[0.9, 0.5, 0.2]]))
    o, got, ref, bud, frag = _run_crafted(d, "corner")
    np.testing.assert_array_equal(o["xy"][0], np.float32([16.0, 16.0]))
    assert int(frag.sum()) == 0 and int((o["n_contrib"].reshape(2, 16, 2, 16).max(axis=(1, 3)) > 0).sum()) == 4
    _check(d, got, ref, bud, frag, "corner of four tiles")
    assert (got["dL_dmeans2D_abs"][0, :2] > 1e-3).all()


def test_two_hundred_faint_gaussians_on_one_tile(native_lib):
    """200 low-opacity Gaussians stacked on one 16 x 16 tile: four 64-entry rounds of the backward, no early stop"""
    P = 200
    gen = torch.Generator().manual_seed(11)
    xyz = [[0.3 * math.cos(0.7 * i), 0.3 * math.sin(1.3 * i), 4.0 + 0.01 * i] for i in range(P)]
    d = _crafted(16, 16, xyz, 0.01, 1.0, torch.rand(P, 3, generator=gen))
    o, got, ref, bud, frag = _run_crafted(d, "stack")
    assert int(o["n_contrib"].max()) > 192 and float(o["final_T"].min()) > 1e-2      # four rounds, nobody stops early
    _check(d, got, ref, bud, frag, "200 faint Gaussians")
    assert (got["dL_dmeans2D_abs"][:, :2].max(axis=1) > 0).sum() >= P - int((frag > 0).sum()) - 1


def test_one_pixel_image(native_lib):
    d = _crafted(1, 1, [[0.5, -0.25, 4.0]], 0.8, 1.0, torch.tensor([[0.9, 0.5, 0.2]]))
    o, got, ref, bud, frag = _run_crafted(d, "1 x 1")
    assert o["radii"][0] > 0 and int(frag.sum()) == 0
    _check(d, got, ref, bud, frag, "1 x 1 image")
    # one pixel: the absolute sum is the absolute value of the signed one
    np.testing.assert_allclose(got["dL_dmeans2D_abs"][0, :2], np.abs(got["dL_dmeans2D"][0, :2]), rtol=1e-6, atol=0)
    assert (got["dL_dmeans2D_abs"][0, :2] > 0).all()


def test_point_behind_the_camera(native_lib):
    d = _crafted(16, 16, [[0.0, 0.0, -1.0]], 0.8, 1.0, torch.tensor([[0.9, 0.5, 0.2]]))
    n = decode_result(d, _forward(d))
    assert int(n["radii"][0]) == 0
    got = _backward(d, n, torch.ones(3, 16, 16))
    for k in ("dL_dmeans2D", "dL_dmeans2D_abs", "dL_dmeans3D", "dL_dopacity"):
        assert np.isfinite(got[k]).all() and not got[k].any(), k


# ---- every ABS and AUX + ABS instance of the blend backward ------------------------------------------------------------------
def _instance_cases():
    out = []
    for scene in ("A1", "A2"):
        for em in (0, 1, 2, 3):
            for cull in (0, 1):
                for aux in (False, True):
                    split = 3 if len(out) % 2 else 1     # every second case: an absgrad backward must ignore the option
                    out.append(dict(id=f"{scene}-exp{em}-cull{cull}-{'aux+abs' if aux else 'abs'}" + ("-split3" if split == 3 else ""),
                                    scene=scene, exp_mode=em, cull=cull, aux=aux, split=split))
    return out


INSTANCES = _instance_cases()


@pytest.mark.parametrize("case", INSTANCES, ids=[c["id"] for c in INSTANCES])
def test_blend_instance(native_lib, case):
    d = IC.inputs(dict(scene=case["scene"]))
    o = IC.reference(dict(scene=case["scene"], seed=None, feature="aux"))["o"]
    aux = case["aux"]
    with _options(exp_mode=case["exp_mode"], cull=case["cull"], split=case["split"]):
        n = decode_result(d, _forward(d, aux=aux))
        frag_px, _ = assert_blend_matches(n, o, what=case["id"])
        g, gD, gA = IC.upstream_gradients(d["H"], d["W"], frag_px)
        got = _backward(d, n, g, gD if aux else None, gA if aux else None)
    ref, bud, frag, signed = AG.reference(d, o, n, g.numpy(), *((gD.numpy()[0], gA.numpy()[0]) if aux else ()))
    # (the helper over the native state agrees with the oracle it is compared next to)
    assert (np.abs(signed - ref["dL_dmeans2D"]) <= 1e-12 * np.maximum(ref["dL_dmeans2D_abs"], 1e-300) + 1e-300).all()
    _check(d, got, ref, bud, frag, case["id"])
    assert (ref["dL_dmeans2D_abs"] > 2.0 * np.abs(ref["dL_dmeans2D"])).any()      # cancellation is really there


# ---- the per-Gaussian kernel forms ------------------------------------------------------------------------------------------
FORMS = [("M1", False, False), ("M4", False, False), ("M9", False, False), ("P257-M9", False, False), ("colors", False, False),
         ("M1", True, False), ("M9", True, False), ("P257-M9", True, False), ("colors", True, False), ("M9", False, True),
         ("M4", True, True)]


def _written_for_every_row(got, n, what):
    a = got["dL_dmeans2D_abs"]
    vis = n["radii"].cpu().numpy() > 0
    assert np.isfinite(a).all(), f"{what}: an element of absgrad was never written"
    assert not a[~vis].any(), f"{what}: a culled Gaussian has a gradient"
    assert (a[:, 2] == 0).all() and (a >= 0).all()
    assert (a[vis, :2].max(axis=1) > 0).sum() > 0.5 * vis.sum(), f"{what}: most visible Gaussians reach a pixel"
    assert (a[:, :2] >= np.abs(got["dL_dmeans2D"][:, :2]) * (1 - 1e-4) - ATOL).all()


@pytest.mark.parametrize("scene,raw,aa", FORMS, ids=[f"{s}{'-raw' if r else ''}{'-aa' if a else ''}" for s, r, a in FORMS])
def test_per_gaussian_kernel_form(native_lib, scene, raw, aa):
    """plain (M = 1, precomputed colours), _vec (M = 4) and _staged (M = 9; 257 rows: a second workgroup of one Gaussian) forms,
    activated and raw attributes, with and without the anti-aliasing chain: absgrad is written for every row, and is the
    reference's (the raw form: the activated form's, at the bar of the raw-attribute instance tests)"""
    what = f"{scene}{'-raw' if raw else ''}{'-aa' if aa else ''}"
    d = IC.inputs(dict(scene=scene))
    n = decode_result(d, _forward(d, aa=aa))
    # the oracle blends what the GPU blended: with anti-aliasing the records' own o_eff
    vis = n["radii"].cpu().numpy() > 0
    op = np.where(vis, n["conic_opacity"][:, 3], d["opacities"].numpy().reshape(-1)).astype(np.float32)
    d_o = dict(d, opacities=torch.from_numpy(op).reshape(d["opacities"].shape).contiguous()) if aa else d
    o = run_oracle(d_o) if aa else IC.reference(dict(scene=scene, seed=None, feature="aux"))["o"]
    frag_px, _ = assert_blend_matches(n, o, what=what)
    if raw:
        dr = IC.raw_inputs(d)
        nr = decode_result(dr, _forward(dr, aa=aa, raw=True))
        differ = (n["n_contrib"] != nr["n_contrib"]) | IC.raw_fragile_pixels(dict(scene=scene, seed=None, feature="aa" if aa else "aux"))
        assert int((n["n_contrib"] != nr["n_contrib"]).sum()) <= 2
        frag_px = frag_px | differ
    g, _, _ = IC.upstream_gradients(d["H"], d["W"], frag_px)
    ref, bud, frag, _ = AG.reference(d_o, o, n, g.numpy())
    got = _backward(d, n, g, aa=aa)
    _written_for_every_row(got, n, what)
    # (with anti-aliasing only the blend-level arrays are the plain oracle's; the h chain has its own tests)
    keys = ("dL_dmeans2D", "dL_dmeans2D_abs") if aa else tuple(ref)
    _check(d, got, {k: ref[k] for k in keys}, bud, frag, what)
    if raw:
        got_r = _backward(dr, nr, g, raw=True, aa=aa)
        _written_for_every_row(got_r, nr, what + " (raw run)")
        for k in ("dL_dmeans2D_abs", "dL_dmeans2D"):
            scale = max(1.0, float(np.abs(got[k]).max()))
            err = float(np.abs(got[k] - got_r[k]).max())
            print(f"[absgrad] {what}: raw / activated {k} differ by {err:.2e} (bar {(2e-4 if aa else 1e-4) * scale:.2e})")
            assert err <= (2e-4 if aa else 1e-4) * scale, (k, err, scale)


# ---- the Python interface ----------------------------------------------------------------------------------------------------
def _scene_and_oracle(P=2000, S=64):
    from gaussian_gan_decoder_amd.synthetic import make_scene
    sc_cpu = make_scene(P, S, "cube", seed=5, log_scale_mean=-4.5)
    sc = sc_cpu.to(DEV)
    pc = sc.gaussian_model(requires_grad=True)
    cam = sc_cpu.cam
    cpu = lambda t: t.detach().cpu()
    d = dict(P=P, W=S, H=S, sh_degree=0, scale_modifier=1.0, tanfovx=math.tan(cam.FoVx * 0.5),
             tanfovy=math.tan(cam.FoVy * 0.5), means3D=sc_cpu.xyz, opacities=cpu(pc.get_opacity),
             viewmatrix=cam.world_view_transform.contiguous(), projmatrix=cam.full_proj_transform.contiguous(),
             campos=cam.camera_center, bg=sc_cpu.bg, shs=sc_cpu.features_dc.contiguous(), colors_precomp=None,
             scales=cpu(pc.get_scaling).contiguous(), rotations=cpu(pc.get_rotation).contiguous(), cov3D_precomp=None)
    return sc, pc, d


def _spy(monkeypatch):
    """records which backward entry point of the library is called"""
    from gaussian_gan_decoder_amd import _capi
    lib = _capi.context_for(DEV).lib
    calls = []
    for name in ("ggd_backward", "ggd_backward_aux", "ggd_backward_abs"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    return calls


def test_render_simple_sets_absgrad(native_lib, monkeypatch):
    """render_simple(..., absgrad=True) then backward(): viewspace_points.absgrad, float32 [P, 3], the reference's; overwritten
    (not accumulated) by the next backward.  Without the keyword the attribute is absent, the call made is ggd_backward, and
    its gradients meet the same reference."""
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    from gaussian_gan_decoder_amd.synthetic import make_dL_dpix
    sc, pc, d = _scene_and_oracle()
    _capi.context_for(DEV).poison_outputs = True
    calls = _spy(monkeypatch)
    g = make_dL_dpix(d["W"])
    o = run_oracle(d)
    n = decode_result(d, _forward(d))
    frag_px, _ = assert_blend_matches(n, o, what="api scene")
    g[:, torch.from_numpy(frag_px)] = 0.0
    ref, bud, frag, _ = AG.reference(d, o, n, g.numpy())
    ok = frag == 0

    def run(**kw):
        for p in (pc._xyz, pc._features_dc):
            p.grad = None
        out = render_simple(sc.cam, pc, bg_color=sc.bg, **kw)
        (out["render"] * g.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        return out["viewspace_points"]

    def within(got, name):
        r = ref[name]
        tol = ATOL + KAPPA * EPS32 * bud[name]
        ratio = float((np.abs(got.detach().cpu().numpy().reshape(r.shape) - r) / tol)[ok].max())
        print(f"[absgrad] api {name}: worst error / bound {ratio:.3f}")
        return ratio <= 1.0

    pts = run()
    assert calls == ["ggd_backward"] and not hasattr(pts, "absgrad")
    assert within(pts.grad, "dL_dmeans2D") and within(pc._xyz.grad, "dL_dmeans3D")
    calls.clear()
    pts = run(absgrad=True)
    assert calls == ["ggd_backward_abs"]
    a = pts.absgrad
    assert a.shape == (d["P"], 3) and a.dtype == torch.float32 and a.device == pts.device and not a.requires_grad
    assert within(a, "dL_dmeans2D_abs") and within(pts.grad, "dL_dmeans2D") and within(pc._xyz.grad, "dL_dmeans3D")
    assert float(a.max()) > 1e-3
    # a second backward through another graph of the same call overwrites: same values, not twice them
    pts2 = run(absgrad=True)
    assert within(pts2.absgrad, "dL_dmeans2D_abs")
    # with the depth / alpha maps read as well the call is the same entry point, with their gradients
    calls.clear()
    out = render_simple(sc.cam, pc, bg_color=sc.bg, render_depth_alpha=True, absgrad=True)
    ((out["render"] * g.to(DEV)).sum() + out["depth"].mean() + out["alpha"].mean()).backward()
    assert calls == ["ggd_backward_abs"] and torch.isfinite(out["viewspace_points"].absgrad).all()


@pytest.mark.parametrize("form", ["radii", "filter"])
def test_densification_statistics_from_absgrad(native_lib, form):
    """update_densification_stats / add_densification_stats(..., use_absgrad=True): on the visible rows accum += the norm of
    absgrad[:, :2] and denom += 1, bit for bit: torch.norm's accumulation on the device (the 3DGS loop's own line) and
    sqrt(x * x + y * y) from IEEE float32 operations rounded one at a time, which is what the unchanged statistics kernel
    computes; .grad is not looked at."""
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    from gaussian_gan_decoder_amd.synthetic import make_dL_dpix
    sc, pc, d = _scene_and_oracle()
    P = d["P"]
    gen = torch.Generator().manual_seed(4)
    accum0, denom0 = torch.rand((P, 1), generator=gen) * 1e-3, torch.randint(0, 9, (P, 1), generator=gen).float()
    radii0 = torch.randint(0, 40, (P,), generator=gen).float()
    pc.xyz_gradient_accum, pc.denom, pc.max_radii2D = accum0.clone().to(DEV), denom0.clone().to(DEV), radii0.clone().to(DEV)
    out = render_simple(sc.cam, pc, bg_color=sc.bg, absgrad=True)
    (out["render"] * make_dL_dpix(d["W"]).to(DEV)).sum().backward()
    pts, radii = out["viewspace_points"], out["radii"]
    with torch.no_grad():
        if form == "radii":
            pc.update_densification_stats(pts, radii, use_absgrad=True)
        else:
            pc.add_densification_stats(pts, radii > 0, use_absgrad=True)
    torch.cuda.synchronize()
    a, vis = pts.absgrad.cpu(), (radii > 0).cpu()
    assert vis.any()
    got_a = pc.xyz_gradient_accum.cpu()
    # the 3DGS loop's own line, on the device
    on_dev = accum0.to(DEV) + torch.where((radii > 0)[:, None], torch.norm(pts.absgrad[:, :2], dim=-1, keepdim=True), 0.0)
    # and the same from IEEE float32 operations rounded one at a time (numpy on the host)
    x, y = a[:, 0].numpy(), a[:, 1].numpy()
    norm = torch.from_numpy(np.sqrt(x * x + y * y).astype(np.float32)).reshape(P, 1)
    want = torch.where(vis[:, None], accum0 + norm, accum0)
    print(f"[absgrad] statistics ({form}): {int((got_a != on_dev.cpu()).sum())} of {int(vis.sum())} visible rows differ from "
          f"torch.norm's accumulation, {int((got_a != want).sum())} from numpy's")
    assert torch.equal(got_a, on_dev.cpu())
    assert torch.equal(got_a, want)
    assert torch.equal(pc.denom.cpu(), denom0 + vis[:, None].float())
    # the signed statistic of the same frame is another number
    signed = pts.grad.cpu()
    assert not torch.equal(norm, torch.sqrt(signed[:, 0] * signed[:, 0] + signed[:, 1] * signed[:, 1]).reshape(P, 1))
    want_r = torch.maximum(radii0, radii.cpu().float()) if form == "radii" else radii0
    assert torch.equal(pc.max_radii2D.cpu(), torch.where(vis, want_r, radii0))
