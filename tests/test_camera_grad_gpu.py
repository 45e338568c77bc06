"""The camera's gradients (camera_grad=True; ggd_backward_camera) on the GPU.

Reference and bar from tests/_camera_grad_ref.py: float64 over the float64 sums of the reference backward on the NATIVE run's
lists, |gpu - ref64| <= 1e-5 + carried + K 2^-24 budget.  The translation identity ties the new sums to dL_dmeans3D of the same call
with no reference in between.  The antialiasing, depth / alpha and feature + distortion instances take their float64 accumulators
from those extensions' references; the fused-activation run is held to the activated one.  Each test prints its figures before it
asserts."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import _camera_grad_ref as CR
from _util import EPS32, assert_blend_matches, backward_reference, check_gradients, decode_result, device_args, run_oracle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drots")


def _forward(d, raw=False, **kw):
    from gaussian_gan_decoder_amd import rasterizer as R
    return R.rasterize_gaussians_native(*device_args(d), raw, **kw)


def _backward(d, res, g, camera=True, raw=False, aa=False, **kw):
    """the tuple of rasterize_gaussians_backward_native, on the host, with poisoned outputs"""
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd import rasterizer as R
    _capi.context_for(DEV).poison_outputs = True   # the library must write every element itself
    t = lambda x: torch.empty(0, device=DEV) if x is None else x.to(DEV)
    kw = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}
    if camera:
        kw["camera_grad"] = True
    outs = R.rasterize_gaussians_backward_native(
        t(d["bg"]), t(d["means3D"]), res[2], t(d["colors_precomp"]), t(d["scales"]), t(d["rotations"]), d["scale_modifier"],
        t(d["cov3D_precomp"]), t(d["viewmatrix"]), t(d["projmatrix"]), d["tanfovx"], d["tanfovy"], g.to(DEV), t(d["shs"]),
        d["sh_degree"], t(d["campos"]), res[3], res[0], res[4], res[5], False, raw,
        d["opacities"].to(DEV) if (raw or aa) else None, antialiasing=aa, **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _camera35(outs):
    dV, dPV, dc = outs[-3:]
    assert dV.shape == (4, 4) and dPV.shape == (4, 4) and dc.shape == (3,)
    v = np.concatenate([dV.reshape(16), dPV.reshape(16), dc]).astype(np.float64)
    assert np.isfinite(v).all(), "a value the library never wrote"
    assert (v[CR.UNREAD] == 0).all(), "entries no kernel reads must be exactly 0"
    return v


def _identity(d, outs, what):
    """sum_i dL_dmeans3D[i] (float64) = V dV[12 + r] + PV dPV[12 + r] - dcampos, within K 2^-24 of the absolute-value sum"""
    v = _camera35(outs)
    V, PV = d["viewmatrix"].double().numpy().reshape(16), d["projmatrix"].double().numpy().reshape(16)
    dm = outs[3].astype(np.float64)
    lhs, scale = dm.sum(0), np.abs(dm).sum(0)
    for c in range(3):
        parts = [V[4 * c + r] * v[12 + r] for r in range(3)] + [PV[4 * c + r] * v[16 + 12 + r] for r in (0, 1, 3)] + [-v[32 + c]]
        rhs = sum(parts)
        bound = CR.K * EPS32 * (scale[c] + sum(abs(x) for x in parts)) + 1e-30
        print(f"[camera_grad] {what}: identity column {c}: sum dL_dmeans3D {lhs[c]:.6e}, from the camera's sums {rhs:.6e}, "
              f"difference / bound {abs(lhs[c] - rhs) / bound:.4f}")
        assert abs(lhs[c] - rhs) <= bound, what
    return v


@functools.lru_cache(maxsize=None)
def _case(name):
    """one scene: forward, reference backward on the native lists, camera backward (shared by the tests that need it)"""
    d = CR.SCENES[name]()
    o = run_oracle(d)
    res = _forward(d)
    n = decode_result(d, res)
    frag_px, _ = assert_blend_matches(n, o, what=name)
    g = torch.randn(3, d["H"], d["W"], generator=torch.Generator().manual_seed(11))
    g[:, torch.from_numpy(frag_px)] = 0.0
    ref, bud, frag = backward_reference(d, o, n, g.numpy())
    assert int((frag > 0).sum()) == 0, f"{name}: a sum cannot leave a Gaussian on the alpha floor out"
    outs = _backward(d, res, g)
    return d, o, res, g, ref, bud, frag, outs


@pytest.mark.parametrize("name", list(CR.SCENES))
def test_matches_reference(native_lib, name):
    d, o, res, g, ref, bud, frag, outs = _case(name)
    assert len(outs) == 11
    worst8 = check_gradients(d, dict(zip(NAMES, outs)), ref, bud, frag)
    val, b, car, _ = CR.reference(o, ref, bud)
    v = _identity(d, outs, name)
    print(f"[camera_grad] {name}: eight gradients error / bound {worst8:.4f}")
    assert worst8 <= 1.0
    _check_camera(v, val, b, car, name)
    if d["colors_precomp"] is not None or d["sh_degree"] == 0:
        assert (v[32:] == 0).all(), "dL_dcampos is exactly 0 at degree 0 and with colors_precomp"
    else:
        assert np.abs(v[32:]).max() > 0


def _check_camera(v, val, b, car, what):
    ratio = np.abs(v - val) / CR.tolerance(b, car)
    k = int(ratio.argmax())
    print(f"[camera_grad] {what}: camera: worst error / bound {ratio.max():.4f} at entry {k} (gpu {v[k]:.6e}, ref {val[k]:.6e}, "
          f"budget {b[k]:.3e}); |dV| up to {np.abs(val[:16]).max():.3e}, |dPV| {np.abs(val[16:32]).max():.3e}, "
          f"|dcampos| {np.abs(val[32:]).max():.3e}")
    assert ratio.max() <= 1.0, what
    assert np.abs(val[:12]).max() > 0 and np.abs(val[16:28]).max() > 0     # the rotation part is exercised


def _instance(**fwd):
    d = CR.SCENES[CR.INSTANCE_SCENE]()
    res = _forward(d, **fwd)
    return d, res, decode_result(d, res)


def _upstream(d, frag_px, seed=5, planes=()):
    gen = torch.Generator().manual_seed(seed)
    out = [torch.randn(c, d["H"], d["W"], generator=gen) for c in (3,) + tuple(planes)]
    for g in out:
        g[:, torch.from_numpy(frag_px)] = 0.0
    return out


def test_antialiasing_matches_reference(native_lib):
    """the h chain in dT and dt: the oracle at the opacities the GPU's records carry (o h in fp32), the reference with the chain"""
    import _antialias_ref as AA
    from test_antialiasing_gpu import _gpu_opacity_inputs
    d, res, n = _instance(antialiasing=True)
    d_o = _gpu_opacity_inputs(d, n)
    o = run_oracle(d_o)
    frag_px, _ = assert_blend_matches(n, o, what="antialiasing")
    g, = _upstream(d, frag_px)
    ref, bud, frag = backward_reference(d_o, o, n, g.numpy())
    assert int((frag > 0).sum()) == 0
    outs = _backward(d, res, g, aa=True)
    val, b, car, _ = CR.reference(o, ref, bud, aa_opacity=d["opacities"].numpy())
    plain, _, _, _ = CR.reference(o, ref, bud)
    assert np.abs(val - plain)[:12].max() > 1e-3 * np.abs(val[:12]).max(), "the scene must make the h chain count"
    ref8, bud8 = AA.compose_backward(d, ref, bud)
    worst8 = check_gradients(d, dict(zip(NAMES, outs)), ref8, bud8, frag)
    print(f"[camera_grad] antialiasing: eight gradients error / bound {worst8:.4f}")
    assert worst8 <= 1.0
    _check_camera(_identity(d, outs, "antialiasing"), val, b, car, "antialiasing")


def test_depth_and_alpha_gradients_match_reference(native_lib):
    """random dL_ddepth / dL_dalpha: the depth slot on dtz p_c, the joined accumulators everywhere else"""
    import _depth_alpha_ref as DA
    d, res, n = _instance(render_depth_alpha=True)
    o = run_oracle(d)
    frag_px, _ = assert_blend_matches(n, o, what="depth_alpha")
    g, gD, gA = _upstream(d, frag_px, planes=(1, 1))
    ref, bud, frag = DA.backward_ref(d, o, n, g.numpy(), gD.numpy()[0], gA.numpy()[0])
    assert int((frag > 0).sum()) == 0
    gz, gzb = CR.depth_slot(o, gD.numpy()[0], gA.numpy()[0], n)
    outs = _backward(d, res, g, dL_ddepth=gD, dL_dalpha=gA)
    worst8 = check_gradients(d, dict(zip(NAMES, outs)), ref, bud, frag)
    print(f"[camera_grad] depth_alpha: eight gradients error / bound {worst8:.4f}")
    assert worst8 <= 1.0
    val, b, car, _ = CR.reference(o, ref, bud, gz, gzb)
    without, _, _, _ = CR.reference(o, ref, bud)
    assert np.abs(val - without)[:12].max() > 1e-3 * np.abs(val[:12]).max(), "the depth slot must count"
    _check_camera(_identity(d, outs, "depth_alpha"), val, b, car, "depth_alpha")


def test_antialiasing_with_depth_and_alpha_matches_reference(native_lib):
    """antialiasing and the depth / alpha maps in one call (camera_partial_kernel<true, true>): the oracle at the opacities the
    GPU's records carry, the depth / alpha reference on it, the h chain over the JOINED opacity sum and the depth slot on dtz p_c"""
    import _antialias_ref as AA
    import _depth_alpha_ref as DA
    from test_antialiasing_gpu import _gpu_opacity_inputs
    what = "antialiasing + depth_alpha"
    d, res, n = _instance(antialiasing=True, render_depth_alpha=True)
    d_o = _gpu_opacity_inputs(d, n)
    o = run_oracle(d_o)
    frag_px, _ = assert_blend_matches(n, o, what=what)
    g, gD, gA = _upstream(d, frag_px, planes=(1, 1))
    ref, bud, frag = DA.backward_ref(d_o, o, n, g.numpy(), gD.numpy()[0], gA.numpy()[0])
    assert int((frag > 0).sum()) == 0
    gz, gzb = CR.depth_slot(o, gD.numpy()[0], gA.numpy()[0], n)
    outs = _backward(d, res, g, aa=True, dL_ddepth=gD, dL_dalpha=gA)
    assert len(outs) == 11
    op = d["opacities"].numpy()
    val, b, car, _ = CR.reference(o, ref, bud, gz, gzb, aa_opacity=op)
    no_chain, _, _, _ = CR.reference(o, ref, bud, gz, gzb)
    no_slot, _, _, _ = CR.reference(o, ref, bud, aa_opacity=op)
    scale = np.abs(val[:12]).max()
    print(f"[camera_grad] {what}: the h chain moves the reference by {np.abs(val - no_chain)[:12].max() / scale:.2e} of its scale, "
          f"the depth slot by {np.abs(val - no_slot)[:12].max() / scale:.2e}")
    assert np.abs(val - no_chain)[:12].max() > 1e-3 * scale, "the scene must make the h chain count"
    assert np.abs(val - no_slot)[:12].max() > 1e-3 * scale, "the depth slot must count"
    ref8, bud8 = AA.compose_backward(d, ref, bud)
    worst8 = check_gradients(d, dict(zip(NAMES, outs)), ref8, bud8, frag)
    print(f"[camera_grad] {what}: eight gradients error / bound {worst8:.4f}")
    assert worst8 <= 1.0
    _check_camera(_identity(d, outs, what), val, b, car, what)


def test_features_with_distortion_match_reference(native_lib):
    """features C = 5 with the distortion map: three kernels' sums joined in the accumulator records, the map's dL/dz in the depth
    slot.  The distortion reference's budgets enter at its own K (DR.K / KAPPA of the others'), as its composition test does."""
    import _distortion_ref as DR
    import _features_ref as FR
    from _util import KAPPA
    d = CR.SCENES[CR.INSTANCE_SCENE]()
    f = torch.rand(d["P"], 5, generator=torch.Generator().manual_seed(6))
    res = _forward(d, render_depth_alpha=True, render_distortion=True, features=f.to(DEV))
    n = decode_result(d, res)
    o = run_oracle(d)
    frag_px, _ = assert_blend_matches(n, o, what="features_distortion")
    g, gF, gX = _upstream(d, frag_px, planes=(5, 1))
    ref, bud, frag = FR.backward_ref(d, o, n, g.numpy(), f.numpy(), None, gF.numpy())
    ref_d, bud_d, frag_d, r = DR.backward_ref(d, o, n, gX.numpy()[0])
    for k in ref_d:
        if ref.get(k) is None or ref_d[k] is None or k in ("dL_dcolors", "dL_dsh"):
            continue
        ref[k] = ref[k] + ref_d[k].reshape(ref[k].shape)
        bud[k] = bud[k] + (DR.K / KAPPA) * bud_d[k].reshape(bud[k].shape)
    frag = np.maximum(frag, frag_d)
    assert int((frag > 0).sum()) == 0
    vis = o["radii"] > 0
    gz, gzb = r["z"] * vis, (DR.K / KAPPA) * r["S_z"] * vis
    outs = _backward(d, res, g, features=f, dL_dfeatmap=gF, dL_ddistortion=gX)
    assert len(outs) == 12
    worst8 = check_gradients(d, dict(zip(NAMES + ("dL_dfeatures",), outs)), ref, bud, frag)
    print(f"[camera_grad] features_distortion: nine gradients error / bound {worst8:.4f}")
    assert worst8 <= 1.0
    val, b, car, _ = CR.reference(o, ref, bud, gz, gzb)
    _check_camera(_identity(d, outs, "features_distortion"), val, b, car, "features_distortion")


def test_fused_activations_follow_the_activated_run(native_lib):
    """raw_attributes: cov3D recomputed from the raw scales and quaternions.  The activated form of this scene is held to the float64
    reference (test_matches_reference); the raw form blends records that differ by the rounding of the activations, so, as in the
    raw tests of the other extensions, it is held to the activated run: 1e-4 of an array's scale (the camera's gradients do not
    pass through an activation's Jacobian), no upstream gradient on a pixel where the two runs may blend another set."""
    import _instance_cases as IC
    from oracle import ggd_oracle as O
    d, o, res, *_ = _case(CR.INSTANCE_SCENE)
    raw = IC.raw_inputs(d)
    raw["rotations"] = (d["rotations"] * 1.7).contiguous()        # (the kernels normalise)
    res_raw = _forward(raw, raw=True)
    n, nr = decode_result(d, res), decode_result(raw, res_raw)
    np.testing.assert_array_equal(nr["point_list"], n["point_list"])
    differ = (n["n_contrib"] != nr["n_contrib"]) | O.fragile_pixels(o, window=IC.RAW_WINDOW)
    assert int(differ.sum()) <= 4
    g, = _upstream(d, differ)
    a, b = _backward(d, res, g), _backward(raw, res_raw, g, raw=True)
    _identity(raw, b, "raw_attributes")
    for name, x, y in zip(("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"), a[-3:], b[-3:]):
        scale = max(1.0, float(np.abs(x).max()))
        err = float(np.abs(x.astype(np.float64) - y).max())
        print(f"[camera_grad] raw / activated {name}: {err:.2e} of scale {scale:.2e}")
        assert err <= 1e-4 * scale, name


def test_empty_frames_write_zeros(native_lib):
    d = CR.SCENES["p65"]()
    d = dict(d); d["means3D"] = (d["means3D"] + torch.tensor([50.0, 0.0, 0.0])).contiguous()   # everything off screen
    res = _forward(d)
    assert res[0] == 0
    outs = _backward(d, res, torch.randn(3, d["H"], d["W"]))
    assert all((o == 0).all() for o in outs[-3:]) and all(np.isfinite(o).all() for o in outs)


def test_c_entry_point_refuses_a_null_bundle(native_lib):
    import ctypes as C
    from gaussian_gan_decoder_amd import _capi
    ctx = _capi.context_for(DEV)
    d = CR.SCENES["p65"]()
    res = _forward(d)
    prm_keep = []
    from gaussian_gan_decoder_amd import rasterizer as R
    rs = R.GaussianRasterizationSettings(d["H"], d["W"], d["tanfovx"], d["tanfovy"], d["bg"].to(DEV), 1.0, d["viewmatrix"].to(DEV),
                                         d["projmatrix"].to(DEV), 0, d["campos"].to(DEV), False, False)
    prm = R._params(rs, d["P"], 1, DEV, prm_keep)
    P = d["P"]
    t = {k: d[k].to(DEV).contiguous() for k in ("means3D", "shs", "scales", "rotations")}
    grads = [torch.zeros(P * n, device=DEV) for n in (3, 3, 1, 3, 6, 3, 3, 4)]
    g = torch.zeros(3, d["H"], d["W"], device=DEV)
    cam = [torch.zeros(16, device=DEV), torch.zeros(16, device=DEV), torch.zeros(3, device=DEV)]
    p = lambda x: C.c_void_p(x.data_ptr())
    head = [ctx.handle, None, C.byref(prm), p(t["means3D"]), p(t["shs"]), None, None, p(t["scales"]), p(t["rotations"]), None,
            p(res[2]), p(res[3]), p(res[4]), p(res[5]), int(res[0]), p(g), None, None] + [p(x) for x in grads] + [None, None]
    assert ctx.lib.ggd_backward_camera(*head, None) == -1                                   # GGD_E_INVALID
    assert b"camera" in ctx.lib.ggd_last_error(ctx.handle)
    bundle = _capi.CameraGrads(cam[0].data_ptr(), None, cam[2].data_ptr())
    assert ctx.lib.ggd_backward_camera(*head, C.byref(bundle)) == -1
    bundle = _capi.CameraGrads(*(x.data_ptr() for x in cam))
    assert ctx.lib.ggd_backward_camera(*head, C.byref(bundle)) == 0
    torch.cuda.synchronize()


def _pose_model(S=64, P=2000, seed=5):
    from gaussian_gan_decoder_amd.synthetic import make_scene
    sc = make_scene(P, S, "cube", seed=seed, log_scale_mean=-4.6).to(DEV)
    return sc, sc.gaussian_model(requires_grad=True)


def test_autograd_through_render_simple_reaches_the_pose(native_lib):
    """extr.grad of a CustomCam equals the REFERENCE's 35 values chained through the same CustomCam ops in float64 torch.  Bar: the
    reference's own (1e-5 + carried + K 2^-24 budget per value) taken through the chain's Jacobian in absolute value, plus the float32
    arithmetic of the chain itself in torch's backward -- the inverse's -V^T G V^T (two nested 4 x 4 products), the bmm's product and
    the sum of the three paths: at most 16 products and sums per entry, 2^-24 each, taken as 64 2^-24 of sum |J| |value|."""
    from gaussian_gan_decoder_amd.cameras import CustomCam
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    sc, pc = _pose_model()
    S = 64
    extr0 = sc.cam.world_view_transform.T.inverse().detach()          # the cam2world pose of the scene's camera
    extr = extr0.clone().requires_grad_(True)
    cam = CustomCam(S, sc.cam.FoVx, extr)
    assert cam.world_view_transform.requires_grad
    # the same frame for the oracle: what render_simple hands to the rasterizer
    cpu = lambda t: t.detach().cpu().contiguous()
    d = dict(P=pc.get_xyz.shape[0], W=S, H=S, sh_degree=0, scale_modifier=1.0, tanfovx=math.tan(cam.FoVx * 0.5),
             tanfovy=math.tan(cam.FoVy * 0.5), means3D=cpu(pc.get_xyz), opacities=cpu(pc.get_opacity),
             viewmatrix=cpu(cam.world_view_transform), projmatrix=cpu(cam.full_proj_transform), campos=cpu(cam.camera_center),
             bg=cpu(sc.bg), shs=cpu(pc.get_features), colors_precomp=None, scales=cpu(pc.get_scaling),
             rotations=cpu(pc.get_rotation), cov3D_precomp=None)
    o = run_oracle(d)
    n = decode_result(d, _forward(d))
    frag_px, _ = assert_blend_matches(n, o, what="pose")
    w = torch.randn(3, S, S, generator=torch.Generator().manual_seed(2))
    w[:, torch.from_numpy(frag_px)] = 0.0
    ref, bud, frag = backward_reference(d, o, n, w.numpy())
    assert int((frag > 0).sum()) == 0
    val, b, car, _ = CR.reference(o, ref, bud)
    tol = CR.tolerance(b, car)

    out = render_simple(cam, pc, bg_color=sc.bg, camera_grad=True)
    assert set(out) == set(render_simple(cam, pc, bg_color=sc.bg))
    (out["render"] * w.to(DEV)).sum().backward()
    got = extr.grad.double().cpu().numpy()

    def chain(e):   # CustomCam's ops: the 35 values' inputs as one vector
        V = e.T.inverse().contiguous()
        PV = V.unsqueeze(0).bmm(cam.projection_matrix.double().cpu().unsqueeze(0)).squeeze(0)
        return torch.cat([V.reshape(16), PV.reshape(16), V[3, :3]])
    J = torch.autograd.functional.jacobian(chain, extr0.double().cpu()).numpy()      # [35, 4, 4]
    want = np.einsum("k,kij->ij", val, J)
    bar = np.einsum("k,kij->ij", tol, np.abs(J)) + 64 * EPS32 * np.einsum("k,kij->ij", np.abs(val), np.abs(J))
    ratio = np.abs(got - want) / bar
    print(f"[camera_grad] extr.grad: max |got - chained reference| {np.abs(got - want).max():.3e} at scale {np.abs(want).max():.3e}, "
          f"worst error / bound {ratio.max():.4f}")
    assert ratio.max() <= 1.0
    assert pc._xyz.grad is not None and float(pc._xyz.grad.abs().max()) > 0


def test_no_camera_call_without_the_keyword_or_a_gradient(native_lib, monkeypatch):
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd.cameras import CustomCam
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    sc, pc = _pose_model()
    lib = _capi.load()
    calls = []
    for name in [n for n in _capi.EXPORTS if n.startswith(("ggd_forward", "ggd_backward"))]:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _r=real: (calls.append(_n), _r(*a))[1])

    def run(cam, **kw):
        calls.clear()
        render_simple(cam, pc, bg_color=sc.bg, **kw)["render"].sum().backward()
        return [c for c in calls if c.startswith("ggd_backward")]
    extr = sc.cam.world_view_transform.T.inverse().detach().clone().requires_grad_(True)
    assert run(sc.cam) == ["ggd_backward"]
    assert run(CustomCam(64, sc.cam.FoVx, extr)) == ["ggd_backward"]                       # no keyword: no camera call
    assert extr.grad is None
    assert run(sc.cam, camera_grad=True) == ["ggd_backward"]                               # nothing requires a gradient
    assert run(CustomCam(64, sc.cam.FoVx, extr), camera_grad=True) == ["ggd_backward_camera"]
    assert extr.grad is not None
    d = CR.SCENES["p65"]()
    res = _forward(d)
    assert len(_backward(d, res, torch.zeros(3, d["H"], d["W"]), camera=False)) == 8
