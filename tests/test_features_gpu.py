"""The feature maps (features= / feature_bg=; ggd_forward_features / ggd_backward_features) on the GPU.

References from the unchanged oracle (tests/_features_ref.py): the C channels are cut into pseudo-colour triples, the oracle's
fp32 blend gives the forward, backward_ref64 over the native run's own final_T / n_contrib / lists gives reference and budget.
Scenes are those of tests/_instance_cases.py, whose fragile-pixel counts the host tests hold under the cap.  Each test prints
its measured figures before it asserts."""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import _antialias_ref as AA
import _features_ref as FR
import _instance_cases as IC
from _util import (ATOL, EPS32, KAPPA, assert_blend_matches, check_gradients, decode_result, device_args, fragile_pixels,
                   run_oracle, scene_inputs)
from test_antialiasing_gpu import _gpu_opacity_inputs
from test_instances_gpu import _options

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drots",
         "dL_dfeatures")


@functools.lru_cache(maxsize=None)
def _features(P, Cn, seed=0):
    """(features [P, C] uniform in [0, 1), a non-zero background [C]); cached: do not modify"""
    gen = torch.Generator().manual_seed(9000 + 37 * Cn + seed)
    return torch.rand(P, Cn, generator=gen), 0.1 + 0.8 * torch.rand(Cn, generator=gen)


def _native(d, f=None, bg=None, aux=False, aa=False, raw=False):
    from gaussian_gan_decoder_amd import rasterizer as R
    kw = {} if f is None else dict(features=f.to(DEV), feature_bg=None if bg is None else bg.to(DEV))
    return R.rasterize_gaussians_native(*device_args(d), raw, render_depth_alpha=aux, antialiasing=aa, **kw)


def _backward(d, n, g, f, bg, gF, gD=None, gA=None, aa=False, raw=False, opacities=None):
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd import rasterizer as R
    _capi.context_for(DEV).poison_outputs = True   # the library must write every element itself
    t = lambda x: torch.empty(0, device=DEV) if x is None else x.to(DEV)
    kw = dict(dL_ddepth=gD.to(DEV), dL_dalpha=gA.to(DEV)) if gD is not None else {}
    op = d["opacities"] if opacities is None else opacities
    outs = R.rasterize_gaussians_backward_native(
        t(d["bg"]), t(d["means3D"]), n["radii"], t(d["colors_precomp"]), t(d["scales"]), t(d["rotations"]),
        d["scale_modifier"], t(d["cov3D_precomp"]), t(d["viewmatrix"]), t(d["projmatrix"]), d["tanfovx"], d["tanfovy"],
        g.to(DEV), t(d["shs"]), d["sh_degree"], t(d["campos"]), n["geom"], n["num_rendered"], n["binning"], n["img"], False,
        raw, op.to(DEV) if (raw or aa) else None, antialiasing=aa, features=f.to(DEV),
        feature_bg=None if bg is None else bg.to(DEV), dL_dfeatmap=gF.to(DEV), **kw)
    torch.cuda.synchronize()
    assert len(outs) == 9
    return {k: v.cpu().numpy() for k, v in zip(NAMES, outs)}


def _oracle(scene):
    return IC.reference(dict(scene=scene, feature="aux"))["o"]


@functools.lru_cache(maxsize=None)
def _forward_reference(scene, Cn):
    f, bg = _features(IC.inputs(dict(scene=scene))["P"], Cn)
    return FR.forward_ref(_oracle(scene), f.numpy(), bg.numpy())


# ---- 1. forward against the oracle
FWD = [("A1", c) for c in (1, 3, 5, 32)] + [(s, c) for s in ("A2", "adversarial", "P257-M9") for c in (5, 32)]


@pytest.mark.parametrize("scene,Cn", FWD, ids=[f"{s}-C{c}" for s, c in FWD])
def test_forward_matches_oracle(native_lib, scene, Cn):
    d, o = IC.inputs(dict(scene=scene)), _oracle(scene)
    f, bg = _features(d["P"], Cn)
    res = _native(d, f, bg)
    assert len(res) == 7 and res[-1].shape == (Cn, d["H"], d["W"]) and res[-1].dtype == torch.float32
    n = decode_result(d, res)
    frag, _ = assert_blend_matches(n, o, what=scene)          # (asserts the cap of 2 + W H / 5000 fragile pixels)
    err = float(np.abs(res[-1].cpu().numpy() - _forward_reference(scene, Cn))[:, ~frag].max(initial=0.0))
    print(f"[features] {scene} C={Cn}: max |dF| = {err:.2e} outside {int(frag.sum())} fragile pixels")
    assert err <= 1e-5


# ---- 2. the same contributors as the colour pass: no mask, every pixel
def _same_contributors(d, what):
    """features = [the records' rgb, z_view, 1], background [bg, 0, 0]: the map is the colour, the depth and the alpha planes of the
    same call, on every pixel.  A contributor in one pass and not in the other shows as ~1/255 = 4e-3."""
    plain = decode_result(d, _native(d))
    vis = (plain["radii"].cpu().numpy() > 0)[:, None]
    rgb = np.where(vis, plain["rgb"], 0.0) if d["colors_precomp"] is None else d["colors_precomp"].numpy()
    z = np.where(vis[:, 0], plain["depths"], 0.0).astype(np.float32)
    f = torch.from_numpy(np.concatenate([rgb, z[:, None], np.ones_like(z)[:, None]], 1).astype(np.float32))
    bg = torch.cat([d["bg"].reshape(3), torch.zeros(2)])
    res = _native(d, f, bg, aux=True)
    color, depth, alpha, F = res[1], res[6], res[7], res[8]
    zmax = max(1.0, float(np.abs(z).max(initial=0.0)))
    e_c = float((F[0:3] - color).abs().max())
    e_d = float((F[3:4] - depth).abs().max())
    e_a = float((F[4:5] - alpha).abs().max())
    print(f"[features] {what}: |F - colour| {e_c:.2e}, |F - depth| {e_d:.2e} (max z {zmax:.2f}), |F - alpha| {e_a:.2e}")
    assert e_c <= 1e-5 and e_a <= 1e-5 and e_d <= 1e-5 * zmax, what


def test_same_contributors_as_the_colour_pass(native_lib):
    _same_contributors(IC.inputs(dict(scene="colors")), "colors")


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("em", [0, 1, 2, 3])
def test_same_contributors_in_every_exp_mode(native_lib, em, cull):
    with _options(dict(IC.DEFAULTS, exp_mode=em, cull=cull)):
        _same_contributors(IC.inputs(dict(scene="A1")), f"A1 exp{em} cull{cull}")


# ---- 3. backward
def _upstream(d, Cn, frag_px, rgb=True, aux=False, seed=IC.GRAD_SEED):
    """N(0, 1) gradients (colour, depth, alpha as IC.upstream_gradients; then the feature map's), zero on the fragile pixels"""
    g, gD, gA = IC.upstream_gradients(d["H"], d["W"], frag_px, seed)
    gF = torch.randn(Cn, d["H"], d["W"], generator=torch.Generator().manual_seed(seed + 100 + Cn))
    gF[:, torch.from_numpy(frag_px)] = 0.0
    if not rgb:
        g = torch.zeros_like(g)
    return g, (gD if aux else None), (gA if aux else None), gF


def _check(d, got, ref, bud, frag, what):
    report = []
    worst = check_gradients(d, got, ref, bud, frag, report=report)
    print(f"[features] {what}: worst gradient error / bound {worst:.3f} "
          f"(dL_dfeatures {[r['worst_ratio'] for r in report if r['array'] == 'dL_dfeatures'][0]:.3f})")
    assert worst <= 1.0, report


BWD = ["features-alone", "with-colour", "with-depth-alpha", "antialiasing", "cov3D_precomp"]


@pytest.mark.parametrize("Cn", [1, 5, 32])
@pytest.mark.parametrize("combo", BWD)
def test_backward_matches_reference(native_lib, combo, Cn):
    scene = "cov-M9" if combo == "cov3D_precomp" else "A1"
    aa, aux = combo == "antialiasing", combo == "with-depth-alpha"
    d = IC.inputs(dict(scene=scene))
    f, bg = _features(d["P"], Cn)
    res = _native(d, f, bg, aux=aux, aa=aa)
    n = decode_result(d, res)
    if aa:   # the oracle at the opacities the GPU's records carry (o h in fp32), as tests/test_antialiasing_gpu.py builds it
        d_o = _gpu_opacity_inputs(d, n)
        o = run_oracle(d_o)
    else:
        d_o, o = d, _oracle(scene)
    frag_px, _ = assert_blend_matches(n, o, what=combo)
    g, gD, gA, gF = _upstream(d, Cn, frag_px, rgb=combo != "features-alone", aux=aux)
    ref, bud, frag = FR.backward_ref(d_o, o, n, g.numpy(), f.numpy(), bg.numpy(), gF.numpy(),
                                     gD.numpy()[0] if aux else None, gA.numpy()[0] if aux else None)
    if aa:
        ref, bud = AA.compose_backward(d, ref, bud)
    got = _backward(d, n, g, f, bg, gF, gD, gA, aa=aa)
    _check(d, got, ref, bud, frag, f"{combo} C={Cn}")


@pytest.mark.parametrize("Cn", [1, 5, 32])
def test_backward_with_fused_activations(native_lib, Cn):
    """The raw-attribute form of scene M1.  Its activated form is held to the float64 reference and budget; the raw form blends
    records that differ from the activated run's by the rounding of the activations (IC.RAW_WINDOW), which no budget of the
    activated inputs covers, so it is held to the activated run pushed through the activations' Jacobians at the bars of the
    depth / alpha and anti-aliasing raw tests (tests/test_instances_gpu.py::_run_raw): 1e-4 of an array's scale where the
    activations do not enter, 2e-4 where they do; no upstream gradient on a pixel where the two runs may blend another set."""
    case = dict(scene="M1", feature="aux")
    d, o = IC.inputs(case), _oracle("M1")
    raw = IC.raw_inputs(d)
    f, bg = _features(d["P"], Cn)
    res, res_raw = _native(d, f, bg), _native(raw, f, bg, raw=True)
    n, nr = decode_result(d, res), decode_result(raw, res_raw)
    frag_px, _ = assert_blend_matches(n, o, what="M1")
    np.testing.assert_array_equal(nr["point_list"], n["point_list"])
    differ = n["n_contrib"] != nr["n_contrib"]
    assert int(differ.sum()) <= 2
    differ = differ | IC.raw_fragile_pixels(case) | frag_px
    err = float(np.abs(res_raw[-1].cpu().numpy() - res[-1].cpu().numpy())[:, ~differ].max(initial=0.0))
    print(f"[features] raw / activated forward C={Cn}: {err:.2e}")
    assert err <= 1e-4
    g, _, _, gF = _upstream(d, Cn, differ)
    ref, bud, frag = FR.backward_ref(d, o, n, g.numpy(), f.numpy(), bg.numpy(), gF.numpy())
    a = _backward(d, n, g, f, bg, gF)
    _check(d, a, ref, bud, frag, f"M1 activated C={Cn}")
    b = _backward(raw, nr, g, f, bg, gF, raw=True)
    s = d["opacities"].double().numpy().reshape(-1, 1)
    expect = {"dL_dmeans3D": (a["dL_dmeans3D"], 1e-4), "dL_dmeans2D": (a["dL_dmeans2D"], 1e-4), "dL_dsh": (a["dL_dsh"], 1e-4),
              "dL_dfeatures": (a["dL_dfeatures"], 1e-4), "dL_dopacity": (a["dL_dopacity"] * s * (1.0 - s), 2e-4),
              "dL_dscales": (a["dL_dscales"] * d["scales"].double().numpy(), 2e-4)}
    for k, (e, rel) in expect.items():
        scale = max(1.0, float(np.abs(e).max(initial=0.0)))
        assert np.isfinite(b[k]).all(), k
        err = float(np.abs(e - b[k].reshape(e.shape)).max(initial=0.0))
        print(f"[features] raw / activated {k} C={Cn}: {err:.2e} of scale {scale:.2e}")
        assert err <= rel * scale, (k, err, scale)


# ---- 4. every element written, nothing beyond
def test_every_element_written_and_nothing_beyond(native_lib):
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd import rasterizer as R
    d = IC.inputs(dict(scene="adversarial"))
    Cn = 5
    f, bg = _features(d["P"], Cn)
    res = _native(d, f, bg)
    n = decode_result(d, res)
    H, W = d["H"], d["W"]
    # the map into a buffer with a guard plane of NaN behind channel C - 1
    buf = torch.full((Cn + 1, H, W), float("nan"), dtype=torch.float32, device=DEV)
    args = device_args(d)
    _, P, _, prm, keep = R._marshal_forward(*args, False)
    ctx, stream = _capi.context_and_stream(DEV)
    fd, bd = f.to(DEV), bg.to(DEV)
    ctx.check(ctx.lib.ggd_forward_features(ctx.handle, C.c_void_p(stream), C.byref(prm), C.c_void_p(res[3].data_ptr()),
                                           C.c_void_p(res[4].data_ptr()), C.c_void_p(res[5].data_ptr()), int(res[0]),
                                           C.c_void_p(fd.data_ptr()), Cn, C.c_void_p(bd.data_ptr()), C.c_void_p(buf.data_ptr())))
    torch.cuda.synchronize()
    assert torch.isnan(buf[Cn]).all(), "the guard plane behind the last channel was written"
    assert torch.isfinite(buf[:Cn]).all()
    assert torch.equal(buf[:Cn], res[-1])
    g, gD, gA, gF = _upstream(d, Cn, np.zeros((H, W), bool), aux=True)
    for kw in (dict(), dict(gD=gD, gA=gA)):
        got = _backward(d, n, g, f, bg, gF, **kw)          # (NaN-fills the nine arrays first)
        for k, v in got.items():
            assert np.isfinite(v).all(), k
        culled = n["radii"].cpu().numpy() == 0
        assert culled.any()
        assert (got["dL_dfeatures"][culled] == 0.0).all()
        assert np.abs(got["dL_dfeatures"][~culled]).max() > 0.0


def test_entry_points_refuse_bad_arguments(native_lib):
    """GGD_E_INVALID (-1) with a message, nothing launched: C outside 1 .. 32, a NULL features / out_features"""
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd import rasterizer as R
    d = IC.inputs(dict(scene="P257-M9"))
    f, bg = _features(d["P"], 5)
    res = _native(d, f, bg)
    _, _, _, prm, keep = R._marshal_forward(*device_args(d), False)
    ctx, stream = _capi.context_and_stream(DEV)
    fd, out = f.to(DEV), torch.full((5, d["H"], d["W"]), float("nan"), device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(feat, Cn, dst):
        return ctx.lib.ggd_forward_features(ctx.handle, C.c_void_p(stream), C.byref(prm), p(res[3]), p(res[4]), p(res[5]),
                                            int(res[0]), p(feat), Cn, None, p(dst))
    for feat, Cn, dst, word in ((fd, 0, out, "outside"), (fd, 33, out, "outside"), (None, 5, out, "NULL"), (fd, 5, None, "NULL")):
        assert call(feat, Cn, dst) == -1
        assert word in ctx.lib.ggd_last_error(ctx.handle).decode()
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote its output"
    assert call(fd, 5, out) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# ---- 5. edges
def test_no_points(native_lib):
    d = scene_inputs(P=8, size=32, seed=3)
    for k in ("means3D", "opacities", "shs", "scales", "rotations"):
        d[k] = d[k][:0].contiguous()
    d["P"] = 0
    f, bg = torch.zeros(0, 4), torch.tensor([0.25, 0.5, 0.0, 1.0])
    res = _native(d, f, bg)
    assert res[0] == 0
    assert torch.equal(res[-1], bg.to(DEV)[:, None, None].expand(4, 32, 32))
    n = dict(radii=res[2], geom=res[3], num_rendered=0, binning=res[4], img=res[5])
    got = _backward(d, n, torch.randn(3, 32, 32), f, bg, torch.randn(4, 32, 32))
    assert got["dL_dfeatures"].shape == (0, 4)


def test_all_points_behind_the_camera(native_lib):
    d = scene_inputs(P=300, size=40, width=40, height=24, seed=4)
    cam_pos = torch.inverse(d["viewmatrix"])[3, :3]
    fwd = d["viewmatrix"][:3, 2]
    d = dict(d, means3D=(cam_pos - 1.5 * fwd + 0.1 * d["means3D"]).contiguous())
    f, bg = _features(300, 7)
    res = _native(d, f, bg)
    assert res[0] == 0, "the scene was meant to render nothing"
    assert torch.equal(res[-1], bg.to(DEV)[:, None, None].expand(7, 24, 40)), "R = 0: F must be feature_bg exactly"
    assert torch.equal(_native(d, f, None)[-1], torch.zeros(7, 24, 40, device=DEV))
    n = decode_result(d, res)
    got = _backward(d, n, torch.randn(3, 24, 40), f, bg, torch.randn(7, 24, 40))
    for k, v in got.items():
        assert (v == 0.0).all(), k


def test_one_pixel_image(native_lib):
    d = scene_inputs(P=64, size=1, width=1, height=1, lsm=-3.0, seed=5)
    o = run_oracle(d)
    f, bg = _features(64, 5)
    res = _native(d, f, bg)
    n = decode_result(d, res)
    assert int(n["n_contrib"][0, 0]) > 0, "the scene was meant to cover its pixel"
    if not fragile_pixels(o)[0, 0]:
        np.testing.assert_array_equal(n["n_contrib"], o["n_contrib"])
        err = float(np.abs(res[-1].cpu().numpy() - FR.forward_ref(o, f.numpy(), bg.numpy())).max())
        print(f"[features] 1x1: |dF| = {err:.2e}")
        assert err <= 1e-5
    gF = torch.randn(5, 1, 1, generator=torch.Generator().manual_seed(6))
    g = torch.zeros(3, 1, 1)
    ref, bud, frag = FR.backward_ref(d, o, n, g.numpy(), f.numpy(), bg.numpy(), gF.numpy())
    _check(d, _backward(d, n, g, f, bg, gF), ref, bud, frag, "1x1")


def _stack(k):
    """k identical splats at the look-at point of a 16 x 16 view (equal depths: the list keeps index order)"""
    d = scene_inputs(P=k, size=16, seed=7)
    one = lambda v, n: torch.tensor([v], dtype=torch.float32).repeat(k, n).contiguous()
    q = torch.zeros(k, 4); q[:, 0] = 1.0
    return dict(d, means3D=torch.zeros(k, 3), opacities=one(0.05, 1), scales=one(0.05, 3), rotations=q.contiguous())


def _round():
    from gaussian_gan_decoder_amd import _capi
    return _capi.FEATURES_ROUND


@pytest.mark.parametrize("k", ["1", "r", "r+1"])
def test_stack_of_identical_splats_in_closed_form(native_lib, k):
    """Every pixel sees the k splats with ONE alpha a (its own): F_c = sum_i a (1 - a)^i f_ic + (1 - a)^k b_c and
    dL/df_ic = sum_pixels a (1 - a)^i G_c, evaluated in float64 from the records the GPU blended; k = 1, r, r + 1 puts the list's
    end on, and one behind, the kernels' round of r records.  Which pixels see the stack (alpha >= 1/255) is the colour pass's
    decision, read from n_contrib.  Bars: forward 1e-5 (weights sum to <= 1, features in [0, 1)); dL/df per element
    1e-5 + 2 (k + 8) eps32 sum |terms|: a term carries the i + 1 roundings of its transmittance product, alpha's own few, and the sum
    over the pixels its additions' -- each below (k + 8) eps32 of the term, doubled for the atomics' order."""
    r = _round()
    k = {"1": 1, "r": r, "r+1": r + 1}[k]
    d = _stack(k)
    Cn = 5
    f, bg = _features(k, Cn)
    res = _native(d, f, bg)
    n = decode_result(d, res)
    nc = n["n_contrib"]
    assert set(np.unique(nc)) <= {0, k} and (nc == k).sum() >= 16, np.unique(nc)
    seen = nc == k
    ys, xs = np.mgrid[0:16, 0:16]
    x0, y0 = n["xy"][0].astype(np.float64)
    cA, cB, cC, op = n["conic_opacity"][0].astype(np.float64)
    dx, dy = x0 - xs, y0 - ys
    a = np.where(seen, np.minimum(0.99, op * np.exp(-0.5 * (cA * dx * dx + cC * dy * dy) - cB * dx * dy)), 0.0)
    assert (1.0 - a.max()) ** k > 1e-3, "the stack was meant to stay clear of the T < 1e-4 stop"
    w = np.stack([a * (1.0 - a) ** i for i in range(k)])                       # [k, H, W]
    f64, bg64 = f.double().numpy(), bg.double().numpy()
    F_ref = np.einsum("ihw,ic->chw", w, f64) + ((1.0 - a) ** k)[None] * bg64[:, None, None]
    err = float(np.abs(res[-1].cpu().numpy() - F_ref).max())
    gF = torch.randn(Cn, 16, 16, generator=torch.Generator().manual_seed(8))
    got = _backward(d, n, torch.zeros(3, 16, 16), f, bg, gF)
    df_ref = np.einsum("ihw,chw->ic", w, gF.double().numpy())
    df_mag = np.einsum("ihw,chw->ic", w, np.abs(gF.double().numpy()))
    ratio = float((np.abs(got["dL_dfeatures"] - df_ref) / (1e-5 + 2.0 * (k + 8) * EPS32 * df_mag)).max())
    print(f"[features] stack k={k}: |dF| {err:.2e}, dL_dfeatures error / bound {ratio:.3f}")
    assert err <= 1e-5
    assert ratio <= 1.0


# ---- 6. the default path
def _model(S=96, P=3000, seed=5):
    from gaussian_gan_decoder_amd.synthetic import make_scene
    sc_cpu = make_scene(P, S, "cube", seed=seed, log_scale_mean=-4.6)
    sc = sc_cpu.to(DEV)
    return sc_cpu, sc, sc.gaussian_model(requires_grad=True)


def test_default_path_is_unmoved(native_lib):
    from gaussian_gan_decoder_amd.gaussian_renderer import render, render_simple
    sc_cpu, sc, pc = _model()
    f, bg = _features(3000, 32)
    with torch.no_grad():
        for fn in (lambda **kw: render_simple(sc.cam, pc, bg_color=sc.bg, render_depth_alpha=True, **kw),
                   lambda **kw: render_simple(sc.cam, pc, bg_color=sc.bg, antialiasing=True, fused_activations=True, **kw)):
            a, b = fn(), fn(features=f.to(DEV), feature_bg=bg.to(DEV))
            assert "features" not in a and b["features"].shape == (32, 96, 96)
            for key in ("render", "radii", "depth", "alpha"):
                assert torch.equal(a[key], b[key]), key

        class Pipe:
            debug = False; compute_cov3D_python = False; convert_SHs_python = False
        a = render(sc.cam, pc, Pipe, sc.bg)
        b = render(sc.cam, pc, Pipe, sc.bg, features=f.to(DEV), override_color=torch.rand(3000, 3, device=DEV))
        assert "features" not in a and b["features"].shape == (32, 96, 96)


def test_no_feature_call_without_the_keyword(native_lib, monkeypatch):
    """without `features` a render makes exactly the calls it makes today: neither new entry point is reached"""
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    sc_cpu, sc, pc = _model()
    lib = _capi.load()
    calls = []
    for name in ("ggd_forward_features", "ggd_backward_features"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _r=real: (calls.append(_n), _r(*a))[1])
    out = render_simple(sc.cam, pc, bg_color=sc.bg, render_depth_alpha=True)
    (out["render"].sum() + out["depth"].sum()).backward()
    assert calls == []
    f = torch.rand(3000, 4, device=DEV, requires_grad=True)
    out = render_simple(sc.cam, pc, bg_color=sc.bg, features=f)
    out["features"].sum().backward()
    assert calls == ["ggd_forward_features", "ggd_backward_features"]


# ---- 7. the autograd surface
def test_autograd_end_to_end(native_lib):
    """a loss on out["features"] alone, through render_simple: the leaf gradients are case 3's reference pushed through the
    model's activations (exp, sigmoid, normalize) in float64; bound per element = the reference's own bound through the
    activation's |Jacobian|, plus 16 eps32 of the chained magnitude for the fp32 evaluation of that Jacobian in torch."""
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    from gaussian_gan_decoder_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    S, P, Cn = 96, 3000, 5
    sc_cpu, sc, pc = _model(S, P)
    f0, bg = _features(P, Cn)
    f = f0.to(DEV).requires_grad_(True)
    cpu = lambda t: t.detach().cpu()
    cam = sc_cpu.cam
    d = dict(P=P, W=S, H=S, sh_degree=0, scale_modifier=1.0, tanfovx=math.tan(cam.FoVx * 0.5),
             tanfovy=math.tan(cam.FoVy * 0.5), means3D=sc_cpu.xyz, opacities=cpu(pc.get_opacity),
             viewmatrix=cam.world_view_transform.contiguous(), projmatrix=cam.full_proj_transform.contiguous(),
             campos=cam.camera_center, bg=sc_cpu.bg, shs=sc_cpu.features_dc.contiguous(), colors_precomp=None,
             scales=cpu(pc.get_scaling).contiguous(), rotations=cpu(pc.get_rotation).contiguous(), cov3D_precomp=None)
    o = run_oracle(d)
    n = decode_result(d, _native(d))
    frag_px, _ = assert_blend_matches(n, o, what="autograd scene")
    _, _, _, gF = _upstream(d, Cn, frag_px)
    out = render_simple(sc.cam, pc, bg_color=sc.bg, features=f, feature_bg=bg.to(DEV))
    assert out["features"].shape == (Cn, S, S)
    (out["features"] * gF.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    ref, bud, frag = FR.backward_ref(d, o, n, np.zeros((3, S, S), np.float32), f0.numpy(), bg.numpy(), gF.numpy())
    ok = frag == 0
    tol = {k: ATOL + KAPPA * EPS32 * bud[k] for k in ("dL_dmeans3D", "dL_dscales", "dL_drots", "dL_dopacity", "dL_dfeatures")}
    worst = {}

    def held(name, got, r, t):
        assert got is not None, f"{name}: no gradient"
        ratio = np.abs(cpu(got).double().numpy().reshape(r.shape) - r) / t
        worst[name] = float(ratio[ok].max(initial=0.0))

    held("_xyz", pc._xyz.grad, ref["dL_dmeans3D"], tol["dL_dmeans3D"])
    held("features", f.grad, ref["dL_dfeatures"], tol["dL_dfeatures"])
    s = cpu(pc.get_scaling).double().numpy()
    r = ref["dL_dscales"] * s
    held("_scaling", pc._scaling.grad, r, tol["dL_dscales"] * s + 16 * EPS32 * np.abs(r))
    a = cpu(pc.get_opacity).double().numpy().reshape(-1)
    J = a * (1.0 - a)
    r = ref["dL_dopacity"].reshape(-1) * J
    held("_opacity", pc._opacity.grad, r, tol["dL_dopacity"].reshape(-1) * J + 16 * EPS32 * np.abs(r))
    q_raw = cpu(pc._rotation).double().numpy()
    nq = np.linalg.norm(q_raw, axis=1)[:, None, None]
    q = q_raw / nq[:, :, 0]
    Jq = (np.eye(4)[None] - q[:, :, None] * q[:, None, :]) / nq          # d normalize / d raw, symmetric
    r = np.einsum("pij,pj->pi", Jq, ref["dL_drots"])
    t = np.einsum("pij,pj->pi", np.abs(Jq), tol["dL_drots"] + 16 * EPS32 * np.abs(ref["dL_drots"]))
    held("_rotation", pc._rotation.grad, r, t)
    print(f"[features] autograd: error / bound per leaf {worst}")
    assert max(worst.values()) <= 1.0, worst
    assert float(pc._xyz.grad.abs().max()) > 0 and float(pc._scaling.grad.abs().max()) > 0
    assert float(pc._rotation.grad.abs().max()) > 0 and float(pc._opacity.grad.abs().max()) > 0
    # the tuple order of GaussianRasterizer.forward: colour, radii, depth, alpha, features
    rs = GaussianRasterizationSettings(S, S, d["tanfovx"], d["tanfovy"], sc.bg, 1.0, sc.cam.world_view_transform,
                                       sc.cam.full_proj_transform, 0, sc.cam.camera_center, False, False,
                                       render_depth_alpha=True)
    with torch.no_grad():
        tup = GaussianRasterizer(rs)(pc.get_xyz, torch.zeros_like(pc.get_xyz), pc.get_opacity, shs=pc.get_features,
                                     scales=pc.get_scaling, rotations=pc.get_rotation, features=f, feature_bg=bg.to(DEV))
    assert [tuple(t.shape) for t in tup] == [(3, S, S), (P,), (1, S, S), (1, S, S), (Cn, S, S)]
    assert tup[1].dtype == torch.int32 and torch.equal(tup[4], out["features"].detach())
