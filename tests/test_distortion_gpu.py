"""The depth-distortion map (render_distortion=True; ggd_forward_distortion / ggd_backward_distortion) on the GPU.

Reference and bars from tests/_distortion_ref.py: float64 over the NATIVE run's decoded lists and the fp32 oracle's records,
|gpu - ref64| <= 1e-5 + K 2^-24 budget with K from the reference's float32 twin; pixels are excluded by cause only (the
oracle's fragile-pixel mask).  Each test prints its measured figures before it asserts."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _antialias_ref as AA
import _distortion_ref as DR
import _features_ref as FR
import _instance_cases as IC
from _util import ATOL, EPS32, KAPPA, assert_blend_matches, check_gradients, decode_result, device_args, run_oracle
from test_antialiasing_gpu import _gpu_opacity_inputs
from test_instances_gpu import _options

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drots")


def _native(d, dist=True, aa=False, raw=False, f=None, bg=None):
    """(num_rendered, colour, radii, geom, binning, img, depth, alpha[, distortion][, features])"""
    from gaussian_gan_decoder_amd import rasterizer as R
    kw = {} if f is None else dict(features=f.to(DEV), feature_bg=None if bg is None else bg.to(DEV))
    if dist:
        kw["render_distortion"] = True
    return R.rasterize_gaussians_native(*device_args(d), raw, render_depth_alpha=True, antialiasing=aa, **kw)


def _backward(d, n, gDist, g=None, gD=None, gA=None, aa=False, raw=False, opacities=None, f=None, bg=None, gF=None):
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd import rasterizer as R
    _capi.context_for(DEV).poison_outputs = True   # the library must write every element itself
    t = lambda x: torch.empty(0, device=DEV) if x is None else x.to(DEV)
    kw = {}
    if gD is not None:
        kw.update(dL_ddepth=gD.to(DEV), dL_dalpha=gA.to(DEV))
    if f is not None:
        kw.update(features=f.to(DEV), feature_bg=None if bg is None else bg.to(DEV), dL_dfeatmap=gF.to(DEV))
    if gDist is not None:
        kw["dL_ddistortion"] = gDist.to(DEV)
    if g is None:
        g = torch.zeros(3, d["H"], d["W"])
    op = d["opacities"] if opacities is None else opacities
    outs = R.rasterize_gaussians_backward_native(
        t(d["bg"]), t(d["means3D"]), n["radii"], t(d["colors_precomp"]), t(d["scales"]), t(d["rotations"]),
        d["scale_modifier"], t(d["cov3D_precomp"]), t(d["viewmatrix"]), t(d["projmatrix"]), d["tanfovx"], d["tanfovy"],
        g.to(DEV), t(d["shs"]), d["sh_degree"], t(d["campos"]), n["geom"], n["num_rendered"], n["binning"], n["img"], False,
        raw, op.to(DEV) if (raw or aa) else None, antialiasing=aa, **kw)
    torch.cuda.synchronize()
    assert len(outs) == 8 + (f is not None)
    return {k: v.cpu().numpy() for k, v in zip(NAMES + ("dL_dfeatures",), outs)}


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return run_oracle(DR.scene(name))


def _upstream(H, W, frag_px, seed=11):
    g = torch.randn(1, H, W, generator=torch.Generator().manual_seed(seed))
    g[:, torch.from_numpy(frag_px)] = 0.0
    return g


_REF = {}


def _reference(key, d_o, o, n, g):
    """backward_ref of one (scene, variant) over the native lists; shared by the runs whose lists, bounds and gradient agree"""
    sig = (key, n["point_list"].tobytes(), n["ranges"].tobytes(), n["n_contrib"].tobytes(), g.numpy().tobytes())
    if sig not in _REF:
        _REF[sig] = DR.backward_ref(d_o, o, n, g.numpy()[0])
    return _REF[sig]


def _check_forward(D, r, frag_px, what, kappa=DR.K):
    ratio = np.abs(D.astype(np.float64) - r["D"]) / (ATOL + kappa * EPS32 * r["D_budget"])
    worst = float(ratio[~frag_px].max(initial=0.0))
    err = float(np.abs(D - r["D"])[~frag_px].max(initial=0.0))
    print(f"[distortion] {what}: max |dD| = {err:.2e} (D up to {float(r['D'].max()):.3f}), error / bound {worst:.4f}")
    assert np.isfinite(D).all() and worst <= 1.0, what
    assert (D[(r["count"] < 2) & ~frag_px] == 0.0).all(), "fewer than two contributors: D = 0"


def _check_backward(d, got, ref, bud, frag, what, kappa=DR.K):
    report = []
    worst = check_gradients(d, got, ref, bud, frag, kappa=kappa, report=report)
    print(f"[distortion] {what}: worst gradient error / bound {worst:.4f} "
          + ", ".join(f"{r['array'][3:]} {r['worst_ratio']:.3f}" for r in report))
    assert worst <= 1.0, report


def _run(name, aa=False, what=""):
    """forward and backward of one scene under the options in effect against the reference"""
    d = DR.scene(name)
    res = _native(d, aa=aa)
    assert len(res) == 9 and res[8].shape == (1, d["H"], d["W"]) and res[8].dtype == torch.float32
    n = decode_result(d, res)
    if aa:   # the oracle at the opacities the GPU's records carry (o h in fp32), as tests/test_antialiasing_gpu.py builds it
        d_o = _gpu_opacity_inputs(d, n)
        o = run_oracle(d_o)
    else:
        d_o, o = d, _oracle(name)
    frag_px, _ = assert_blend_matches(n, o, what=what)          # (asserts the cap on the fragile pixels)
    g = _upstream(d["H"], d["W"], frag_px)
    ref, bud, frag, r = _reference((name, aa), d_o, o, n, g)
    _check_forward(res[8][0].cpu().numpy(), r, frag_px, what)
    if aa:
        ref, bud = AA.compose_backward(d, ref, bud, kappa=DR.K)
    got = _backward(d, n, g, aa=aa)
    _check_backward(d, got, ref, bud, frag, what)
    return d, o, n, res, got, frag_px


# ---- 1. forward and backward against the reference
@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("em", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["shell", "adversarial"])
def test_matches_reference_in_every_exp_mode(native_lib, name, em, cull):
    with _options(dict(IC.DEFAULTS, exp_mode=em, cull=cull)):
        _run(name, what=f"{name} exp{em} cull{cull}")


@pytest.mark.parametrize("name", ["shell", "adversarial"])
def test_matches_reference_with_antialiasing(native_lib, name):
    _run(name, aa=True, what=f"{name} antialiasing")


def test_fused_activations_follow_the_activated_run(native_lib):
    """The raw-attribute form of the shell scene.  Its activated form is held to the float64 reference (above); the raw form
    blends records that differ by the rounding of the activations, so it is held to the activated run pushed through the
    activations' Jacobians at the bars of the depth / alpha, anti-aliasing and feature raw tests: forward 1e-4, gradients 1e-4 of
    an array's scale where the activations do not enter, 2e-4 where they do; no upstream gradient on a pixel where the two runs
    may blend another set (the oracle's fragile mask at IC.RAW_WINDOW)."""
    from oracle import ggd_oracle as O
    d, o = DR.scene("shell"), _oracle("shell")
    raw = IC.raw_inputs(d)
    res, res_raw = _native(d), _native(raw, raw=True)
    n, nr = decode_result(d, res), decode_result(raw, res_raw)
    frag_px, _ = assert_blend_matches(n, o, what="shell")
    np.testing.assert_array_equal(nr["point_list"], n["point_list"])
    differ = n["n_contrib"] != nr["n_contrib"]
    assert int(differ.sum()) <= 2
    differ = differ | O.fragile_pixels(o, window=IC.RAW_WINDOW) | frag_px
    assert int(differ.sum()) <= 4
    err = float(np.abs(res_raw[8].cpu().numpy() - res[8].cpu().numpy())[:, ~differ].max(initial=0.0))
    print(f"[distortion] raw / activated forward: {err:.2e}")
    assert err <= 1e-4
    g = _upstream(d["H"], d["W"], differ)
    a = _backward(d, n, g)
    b = _backward(raw, nr, g, raw=True)
    s = d["opacities"].double().numpy().reshape(-1, 1)
    expect = {"dL_dmeans3D": (a["dL_dmeans3D"], 1e-4), "dL_dmeans2D": (a["dL_dmeans2D"], 1e-4),
              "dL_dopacity": (a["dL_dopacity"] * s * (1.0 - s), 2e-4),
              "dL_dscales": (a["dL_dscales"] * d["scales"].double().numpy(), 2e-4)}
    for k, (e, rel) in expect.items():
        scale = max(1.0, float(np.abs(e).max(initial=0.0)))
        assert np.isfinite(b[k]).all(), k
        err = float(np.abs(e - b[k].reshape(e.shape)).max(initial=0.0))
        print(f"[distortion] raw / activated {k}: {err:.2e} of scale {scale:.2e}")
        assert err <= rel * scale, (k, err, scale)


# ---- 2. three hand-built pixels
def test_hand_built_pixels(native_lib):
    """no contributor: D = 0 and no gradient; one contributor: D = 0 and nothing reaches anybody's alpha; two Gaussians of equal
    depth in front of a third: the tie contributes 0 (the reference's literal sum says so, test_distortion_host.py)"""
    d, o, n, res, got, frag_px = _run("hand", what="hand-built")
    r = DR.evaluate(o, n)
    D = res[8][0].cpu().numpy()
    assert not frag_px.any()
    assert (D[r["count"] < 2] == 0.0).all() and (r["count"] == 0).any() and (r["count"] == 1).any() and D.max() > 1e-2
    z = n["depths"]
    assert z[0] == z[1] < z[2]
    # upstream gradient ONLY on the pixels with fewer than two contributors: the reference is zero in every array, and the
    # bar is the budget of the terms that cancel (the back-to-front walk forms w_1 - w_1 from two differently rounded w_1)
    g = torch.ones(1, d["H"], d["W"]) * torch.from_numpy(r["count"] < 2)[None]
    ref0, bud0, frag0, _ = _reference(("hand", "lone"), d, o, n, g)
    assert all(float(np.abs(v).max(initial=0.0)) == 0.0 for v in ref0.values() if v is not None)
    lone = _backward(d, n, g)
    _check_backward(d, lone, ref0, bud0, frag0, "hand-built, gradient on pixels with < 2 contributors only")
    assert max(float(np.abs(v).max(initial=0.0)) for v in lone.values()) <= 1e-4
    # ... and with colour and alpha gradients beside it, the others' results are those of the backward without the map
    gc, gD, gA = IC.upstream_gradients(d["H"], d["W"])
    with_map = _backward(d, n, g, g=gc, gD=gD, gA=gA)
    without = _backward(d, n, None, g=gc, gD=gD, gA=gA)
    for k in without:
        scale = max(1.0, float(np.abs(without[k]).max(initial=0.0)))
        assert float(np.abs(with_map[k] - without[k]).max(initial=0.0)) <= 2.0 * ATOL * scale, k


# ---- 3. an opaque front layer ends the walk long before the list does
def test_opaque_front_layer_truncates_the_walk(native_lib):
    d, o, n, res, got, frag_px = _run("opaque-front", what="opaque front")
    assert (n["n_contrib"] == 4).all() and int((n["ranges"][:, 1] - n["ranges"][:, 0]).max()) == 36
    r = DR.evaluate(o, n)
    assert (r["count"] == 4).all() and float(res[8].min()) > 0.0
    behind = np.ones(d["P"], bool)
    behind[np.unique(n["point_list"].reshape(-1, 36)[:, :4])] = False
    assert behind.sum() == 32
    for k, v in got.items():
        if v.size:
            assert (v.reshape(d["P"], -1)[behind] == 0.0).all(), f"{k}: a Gaussian behind the last contributor received gradient"
    assert np.abs(got["dL_dmeans3D"][~behind]).max() > 0.0


# ---- 4. closed form
def test_two_constant_layers_in_closed_form(native_lib):
    """two image-filling splats at z1 < z2: D = 2 a1 a2 (1 - a1) (z2 - z1) on every pixel, with the pixel's own alphas evaluated
    in float64 from the records the GPU blended (constant to 4e-6).  Bar: ATOL + K eps32 budget, budget = the two terms of the
    recurrence, 2 w2 (z2 w1 + w1 z1)."""
    d = DR.scene("two-layers")
    res = _native(d)
    n = decode_result(d, res)
    assert (n["n_contrib"] == 2).all()
    ys, xs = np.mgrid[0:d["H"], 0:d["W"]]
    al = []
    for i in (int(n["point_list"][0]), int(n["point_list"][1])):
        x0, y0 = n["xy"][i].astype(np.float64)
        cA, cB, cC, op = n["conic_opacity"][i].astype(np.float64)
        dx, dy = x0 - xs, y0 - ys
        al.append(op * np.exp(-0.5 * (cA * dx * dx + cC * dy * dy) - cB * dx * dy))
    z1, z2 = (float(n["depths"][int(n["point_list"][k])]) for k in (0, 1))
    assert z1 < z2 and abs(al[0] - 0.6).max() < 1e-4 and abs(al[1] - 0.5).max() < 1e-4
    want = DR.closed_form_two_layers(al[0], al[1], z1, z2)
    budget = 2.0 * al[0] * al[1] * (1.0 - al[0]) * (z2 + z1)
    D = res[8][0].cpu().numpy()
    ratio = float((np.abs(D - want) / (ATOL + DR.K * EPS32 * budget)).max())
    print(f"[distortion] two layers: D = {float(D.mean()):.6f}, closed form {float(want.mean()):.6f}, error / bound {ratio:.4f}")
    assert ratio <= 1.0


# ---- 5. every map in one backward
def test_composition_with_every_other_map(native_lib):
    """upstream gradients on colour, depth, alpha, features and distortion at once: the result is the sum of the separate
    references (each at its own bar: KAPPA for the others', K for the map's); everything the call returned before is bit-identical
    with the keyword"""
    d, o = DR.scene("shell"), _oracle("shell")
    gen = torch.Generator().manual_seed(77)
    f, bg = torch.rand(d["P"], 5, generator=gen), 0.1 + 0.8 * torch.rand(5, generator=gen)
    res = _native(d, f=f, bg=bg)
    base = _native(d, dist=False, f=f, bg=bg)
    assert len(res) == 10 and len(base) == 9
    assert res[0] == base[0]
    for i, j, what in ((1, 1, "colour"), (2, 2, "radii"), (6, 6, "depth"), (7, 7, "alpha"), (9, 8, "features")):
        assert torch.equal(res[i], base[j]), what
    n = decode_result(d, res)
    frag_px, _ = assert_blend_matches(n, o, what="composition")
    gc, gD, gA = IC.upstream_gradients(d["H"], d["W"], frag_px)
    gF = torch.randn(5, d["H"], d["W"], generator=gen)
    gF[:, torch.from_numpy(frag_px)] = 0.0
    g = _upstream(d["H"], d["W"], frag_px)
    ref, bud, frag = FR.backward_ref(d, o, n, gc.numpy(), f.numpy(), bg.numpy(), gF.numpy(), gD.numpy()[0], gA.numpy()[0])
    ref_d, bud_d, frag_d, _ = _reference(("shell", False), d, o, n, g)
    for k in ref_d:
        if ref.get(k) is None or ref_d[k] is None or k in ("dL_dcolors", "dL_dsh"):
            continue
        ref[k] = ref[k] + ref_d[k].reshape(ref[k].shape)
        bud[k] = bud[k] + (DR.K / KAPPA) * bud_d[k].reshape(bud[k].shape)
    got = _backward(d, n, g, g=gc, gD=gD, gA=gA, f=f, bg=bg, gF=gF)
    report = []
    worst = check_gradients(d, got, ref, bud, np.maximum(frag, frag_d), report=report)
    print(f"[distortion] composition: worst gradient error / bound {worst:.4f}")
    assert worst <= 1.0, report


# ---- 6. two calls on one stream
def test_two_calls_without_a_host_wait(native_lib):
    """scene A then scene B, forward and backward, enqueued with no host wait between them: each result is its solo run's (the
    forward bit for bit; the backward, whose sums are float atomics, to 1e-5 of the array's scale)"""
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    from gaussian_gan_decoder_amd.synthetic import make_scene

    def step(seed, kind):
        sc = make_scene(2000, 72, kind, seed=seed, log_scale_mean=-4.2).to(DEV)
        pc = sc.gaussian_model(requires_grad=True)
        out = render_simple(sc.cam, pc, bg_color=sc.bg, render_depth_alpha=True, render_distortion=True)
        (out["distortion"].mean() + out["render"].mean()).backward()
        return out["distortion"].detach(), pc._xyz.grad, pc._opacity.grad

    solo = []
    for seed, kind in ((5, "cube"), (6, "shell")):
        solo.append(step(seed, kind))
        torch.cuda.synchronize()
    a, b = step(5, "cube"), step(6, "shell")     # no synchronisation between the two
    torch.cuda.synchronize()
    for got, want in ((a, solo[0]), (b, solo[1])):
        assert torch.equal(got[0], want[0]) and float(got[0].max()) > 0.0
        for x, y in zip(got[1:], want[1:]):
            scale = max(1.0, float(y.abs().max()))
            assert float((x - y).abs().max()) <= 1e-5 * scale


# ---- 7. refused calls
def test_entry_points_refuse_bad_arguments(native_lib):
    """GGD_E_INVALID (-1) with a message and nothing launched: a NULL map, and calls without a completed forward's buffers"""
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd import rasterizer as R
    d = DR.scene("hand")
    res = _native(d)
    _, _, inputs, prm, keep = R._marshal_forward(*device_args(d), False)
    ctx, stream = _capi.context_and_stream(DEV)
    out = torch.full((d["H"], d["W"]), float("nan"), device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def fwd(geom, binning, img, R_, dst):
        return ctx.lib.ggd_forward_distortion(ctx.handle, C.c_void_p(stream), C.byref(prm), p(geom), p(binning), p(img), R_, p(dst))
    for args, word in (((res[3], res[4], res[5], int(res[0]), None), "NULL"), ((res[3], res[4], None, int(res[0]), out), "NULL"),
                       ((None, res[4], res[5], int(res[0]), out), "NULL"), ((res[3], None, res[5], int(res[0]), out), "NULL"),
                       ((res[3], res[4], res[5], -1, out), "num_rendered")):
        assert fwd(*args) == -1
        assert word in ctx.lib.ggd_last_error(ctx.handle).decode()
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote its output"
    assert fwd(res[3], res[4], res[5], int(res[0]), out) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, res[8][0])
    # the backward without the map's gradient: refused, the NaN-filled gradient arrays untouched
    P, M = d["P"], d["shs"].shape[1]
    grads = [torch.full(s, float("nan"), device=DEV) for s in ((P, 3), (P, 3), (P, 1), (P, 3), (P, 6), (P, M, 3), (P, 3), (P, 4))]
    g = torch.zeros(3, d["H"], d["W"], device=DEV)
    args = [ctx.handle, C.c_void_p(stream), C.byref(prm), *map(p, inputs), p(res[2]), p(res[3]), p(res[4]), p(res[5]), int(res[0]),
            p(g), None, None, *map(p, grads)]
    assert ctx.lib.ggd_backward_distortion(*args, None, None) == -1
    assert "dL_ddistortion" in ctx.lib.ggd_last_error(ctx.handle).decode()
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in grads), "a refused call wrote a gradient array"
    gd = torch.ones(d["H"], d["W"], device=DEV)
    assert ctx.lib.ggd_backward_distortion(*args, p(gd), None) == 0
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in grads)


# ---- 8. the default path
def _model(S=96, P=3000, seed=5):
    from gaussian_gan_decoder_amd.synthetic import make_scene
    sc = make_scene(P, S, "cube", seed=seed, log_scale_mean=-4.6).to(DEV)
    return sc, sc.gaussian_model(requires_grad=True)


def test_no_distortion_call_without_the_keyword(native_lib, monkeypatch):
    """without the keyword a render makes exactly the calls it makes today; a graph that reads only the colour of a
    render_distortion call runs the plain backward"""
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    sc, pc = _model()
    lib = _capi.load()
    calls = []
    names = [n for n in _capi.EXPORTS if n.startswith(("ggd_forward", "ggd_backward"))]
    for name in names:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _r=real: (calls.append(_n), _r(*a))[1])

    def run(loss, **kw):
        calls.clear()
        out = render_simple(sc.cam, pc, bg_color=sc.bg, **kw)
        loss(out).backward()
        return [c for c in calls if c != "ggd_forward_can_speculate"]
    render_simple(sc.cam, pc, bg_color=sc.bg)            # (the first frame of a shape takes the two-call forward)
    assert run(lambda o: o["render"].sum()) == ["ggd_forward", "ggd_backward"]
    assert run(lambda o: o["render"].sum() + o["depth"].sum(), render_depth_alpha=True) == ["ggd_forward_aux", "ggd_backward_aux"]
    kw = dict(render_depth_alpha=True, render_distortion=True)
    assert run(lambda o: o["distortion"].mean(), **kw) == ["ggd_forward_aux", "ggd_forward_distortion", "ggd_backward_distortion"]
    assert run(lambda o: o["render"].sum(), **kw) == ["ggd_forward_aux", "ggd_forward_distortion", "ggd_backward"]
    assert run(lambda o: o["depth"].sum(), **kw) == ["ggd_forward_aux", "ggd_forward_distortion", "ggd_backward_aux"]
    f = torch.rand(3000, 4, device=DEV, requires_grad=True)
    assert run(lambda o: o["features"].sum() + o["distortion"].mean(), features=f, **kw) == [
        "ggd_forward_aux", "ggd_forward_distortion", "ggd_forward_features", "ggd_backward_distortion"]
    assert float(f.grad.abs().max()) > 0.0
    assert run(lambda o: o["features"].sum(), features=f, **kw) == [
        "ggd_forward_aux", "ggd_forward_distortion", "ggd_forward_features", "ggd_backward_features"]


def test_render_surface_and_tuple_order(native_lib):
    from gaussian_gan_decoder_amd.gaussian_renderer import render, render_simple
    from gaussian_gan_decoder_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    import math
    sc, pc = _model()
    S, P = 96, 3000
    f = torch.rand(P, 4, device=DEV)
    with torch.no_grad():
        for kw in (dict(), dict(antialiasing=True, fused_activations=True), dict(override_color=torch.rand(P, 3, device=DEV)),
                   dict(features=f)):
            a = render_simple(sc.cam, pc, bg_color=sc.bg, render_depth_alpha=True, **kw)
            b = render_simple(sc.cam, pc, bg_color=sc.bg, render_depth_alpha=True, render_distortion=True, **kw)
            assert "distortion" not in a and b["distortion"].shape == (1, S, S) and float(b["distortion"].max()) > 0.0
            for key in ("render", "radii", "depth", "alpha") + (("features",) if "features" in kw else ()):
                assert torch.equal(a[key], b[key]), (key, kw)

        class Pipe:
            debug = False; compute_cov3D_python = False; convert_SHs_python = False
        b = render(sc.cam, pc, Pipe, sc.bg, render_depth_alpha=True, render_distortion=True)
        assert b["distortion"].shape == (1, S, S)
        rs = GaussianRasterizationSettings(S, S, math.tan(sc.cam.FoVx * 0.5), math.tan(sc.cam.FoVy * 0.5), sc.bg, 1.0,
                                           sc.cam.world_view_transform, sc.cam.full_proj_transform, 0, sc.cam.camera_center, False,
                                           False, render_depth_alpha=True, render_distortion=True)
        tup = GaussianRasterizer(rs)(pc.get_xyz, torch.zeros_like(pc.get_xyz), pc.get_opacity, shs=pc.get_features,
                                     scales=pc.get_scaling, rotations=pc.get_rotation, features=f)
    assert [tuple(t.shape) for t in tup] == [(3, S, S), (P,), (1, S, S), (1, S, S), (1, S, S), (4, S, S)]
    assert torch.equal(tup[4], b["distortion"])


def test_trainer_step_with_a_distortion_weight(native_lib):
    """DecoderTrainer(distortion_weight > 0): the loss is the default step's plus weight * mean(D), and its gradient is finite"""
    from gaussian_gan_decoder_amd.train import DecoderTrainer, make_scene_batch
    cfg = dict(plane_res=32, plane_channels=32, hidden_dim=128, image_size=64, seed=7)
    batch = make_scene_batch([0], 2000, cfg["image_size"], DEV, seed=0)
    losses = {}
    for w in (0.0, 0.5):
        tr = DecoderTrainer(DEV, n_scenes_total=1, distortion_weight=w, **cfg)
        with torch.no_grad():   # splats large enough for the 64 x 64 image to see them (as tests/test_train_step_gpu.py)
            tr.decoder.scale_decoder.backbone[-1].bias += 3.5
            tr.decoder.opacity_decoder.backbone[-1].bias += 1.0
        tr.flat_grad.zero_()
        loss = tr.local_loss(batch)
        loss.backward()
        torch.cuda.synchronize()
        losses[w] = float(loss.detach())
        assert torch.isfinite(tr.flat_grad).all() and float(tr.flat_grad.abs().max()) > 0.0
    print(f"[distortion] trainer loss without / with the term: {losses}")
    assert losses[0.5] > losses[0.0]
