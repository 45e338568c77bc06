"""The depth-distortion map without a GPU: the entry points are declared, exported and built without spills; the keyword is off
by default and refused, before any native call, without render_depth_alpha or with absgrad; the trainer's default step makes
the render call it made before; and the reference of tests/_distortion_ref.py stands on its own -- its closed forms equal its
literal double sum, its scenes stay inside the fragile-pixel cap, and its constant K is what its float32 twin measures."""
from __future__ import annotations

import inspect
import os
import re

import numpy as np
import pytest
import torch

import _antialias_ref as AA
import _distortion_ref as DR
from _util import fragile_pixels, run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_and_exported(native_lib):
    from gaussian_gan_decoder_amd import _capi
    header = open(os.path.join(ROOT, "include", "ggd_raster.h")).read()
    for sym in ("ggd_forward_distortion", "ggd_backward_distortion"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
        assert sym in _capi.EXPORTS
        assert hasattr(native_lib, sym)
    assert "ggd_feature_side" in header
    assert [n for n, _ in _capi.FeatureSide._fields_] == ["features", "C", "feature_bg", "dL_dfeatmap", "dL_dfeatures"]
    assert len(native_lib.ggd_backward_distortion.argtypes) == len(native_lib.ggd_backward_aux.argtypes) + 2


def test_distortion_kernels_are_built_without_spills(native_lib):
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    from gaussian_gan_decoder_amd import _capi
    tab = {kr.short(k): v for k, v in kr.kernel_resources(_capi.LIB_PATH).items()}
    fwd = sorted(k for k in tab if k.startswith("distortion_forward_kernel<"))
    bwd = sorted(k for k in tab if k.startswith("distortion_backward_kernel<"))
    assert fwd == [f"distortion_forward_kernel<{em}>" for em in range(3)], fwd
    assert bwd == [f"distortion_backward_kernel<{em}>" for em in range(4)], bwd
    for name in fwd + bwd:
        assert tab[name]["vgpr_spill"] == 0 and tab[name]["scratch"] == 0, (name, tab[name])
        assert tab[name]["lds"] <= 40960, (name, tab[name])       # at least four single-wave workgroups per CU (160 KB of LDS)


def _settings(**kw):
    from gaussian_gan_decoder_amd import rasterizer as R
    return R.GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                           False, False, **kw)


def test_settings_default_is_off():
    from gaussian_gan_decoder_amd import gaussian_renderer as GR
    from gaussian_gan_decoder_amd import rasterizer as R
    from gaussian_gan_decoder_amd import train as T
    rs = _settings()
    assert rs.render_distortion is False and len(rs) == 14 and "render_distortion" not in repr(rs)
    on = _settings(render_depth_alpha=True, render_distortion=True)
    assert on.render_distortion is True and len(on) == 14 and "render_distortion=True" in repr(on)
    assert on._replace(debug=True).render_distortion is True
    assert on._replace(render_distortion=False).render_distortion is False
    assert rs._replace(render_distortion=True).render_distortion is True
    for fn in (R.rasterize_gaussians_native, GR.render, GR.render_simple):
        assert inspect.signature(fn).parameters["render_distortion"].default is False, fn
    assert inspect.signature(R.rasterize_gaussians_native).parameters["render_distortion"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(R.rasterize_gaussians_backward_native).parameters["dL_ddistortion"].default is None
    assert inspect.signature(T.DecoderTrainer.__init__).parameters["distortion_weight"].default == 0.0
    assert "render_distortion" not in inspect.signature(R.FramePipeline.submit).parameters


@pytest.fixture
def no_native(monkeypatch):
    from gaussian_gan_decoder_amd import _capi

    def fail(*a, **k):
        raise AssertionError("the native library was reached")
    for name in ("load", "context_for", "context_and_stream"):
        monkeypatch.setattr(_capi, name, fail)


def _forward_args(P=4, H=8, W=8):
    e = torch.empty(0)
    return (torch.zeros(3), torch.zeros(P, 3), e, torch.ones(P, 1), torch.ones(P, 3), torch.ones(P, 4), 1.0, e, torch.eye(4),
            torch.eye(4), 1.0, 1.0, H, W, torch.zeros(P, 1, 3), 0, torch.zeros(3), False, False)


def _backward_args(H=8, W=8, P=4):
    e = torch.empty(0)
    return (torch.zeros(3), torch.zeros(P, 3), torch.zeros(P, dtype=torch.int32), e, torch.ones(P, 3), torch.ones(P, 4),
            1.0, e, torch.eye(4), torch.eye(4), 1.0, 1.0, torch.zeros(3, H, W), e, 0, torch.zeros(3), torch.empty(0),
            0, torch.empty(0), torch.empty(0), False)


class _Cam:
    FoVx = FoVy = 0.2
    image_height = image_width = 8
    world_view_transform = full_proj_transform = torch.eye(4)
    camera_center = torch.zeros(3)


class _Model:
    active_sh_degree = 0
    get_xyz = torch.zeros(4, 3)
    get_opacity = torch.ones(4, 1)
    get_scaling = torch.ones(4, 3)
    get_rotation = torch.ones(4, 4)
    get_features = torch.zeros(4, 1, 3)


def _rasterize(rs):
    from gaussian_gan_decoder_amd import rasterizer as R
    return R.GaussianRasterizer(rs)(torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(4, 1), shs=torch.zeros(4, 1, 3),
                                    scales=torch.ones(4, 3), rotations=torch.ones(4, 4))


def test_distortion_without_depth_alpha_is_refused(no_native):
    from gaussian_gan_decoder_amd import gaussian_renderer as GR
    from gaussian_gan_decoder_amd import rasterizer as R
    with pytest.raises(ValueError, match="render_depth_alpha"):
        R.rasterize_gaussians_native(*_forward_args(), render_distortion=True)
    with pytest.raises(ValueError, match="render_depth_alpha"):
        _rasterize(_settings(render_distortion=True))
    with pytest.raises(ValueError, match="render_depth_alpha"):
        GR.render_simple(_Cam, _Model, torch.zeros(3), render_distortion=True)


def test_distortion_with_absgrad_is_refused(no_native):
    from gaussian_gan_decoder_amd import gaussian_renderer as GR
    from gaussian_gan_decoder_amd import rasterizer as R
    with pytest.raises(ValueError, match="colour terms"):
        _rasterize(_settings(render_depth_alpha=True, render_distortion=True, absgrad=True))
    with pytest.raises(ValueError, match="colour terms"):
        GR.render_simple(_Cam, _Model, torch.zeros(3), render_depth_alpha=True, render_distortion=True, absgrad=True)
    with pytest.raises(ValueError, match="colour terms"):
        R.rasterize_gaussians_backward_native(*_backward_args(), absgrad=True, dL_ddistortion=torch.zeros(8, 8))


def test_cpu_tensors_raise_as_the_other_inputs_do(no_native):
    from gaussian_gan_decoder_amd import rasterizer as R
    with pytest.raises(RuntimeError, match="CPU"):
        R.rasterize_gaussians_native(*_forward_args(), render_depth_alpha=True, render_distortion=True)


def test_trainer_default_step_renders_as_before():
    """distortion_weight = 0 (the default) leaves render_fn's keywords what they were; a positive weight adds the two keywords
    and nothing else; a negative one is refused"""
    from gaussian_gan_decoder_amd.train import DecoderTrainer

    def fake_render(cam, gs, bg_color, **kw):
        raise RuntimeError("stop")
    mk = lambda **kw: DecoderTrainer("cpu", 1, plane_res=8, plane_channels=4, hidden_dim=8, image_size=8, render_fn=fake_render, **kw)
    assert mk().render_kwargs == {} and mk().distortion_weight == 0.0
    assert mk(distortion_weight=0.0, antialiasing=True).render_kwargs == {"antialiasing": True}
    assert mk(distortion_weight=0.5).render_kwargs == {"render_depth_alpha": True, "render_distortion": True}
    assert mk(distortion_weight=0.5, mask_weight=1.0).render_kwargs == {"render_depth_alpha": True, "render_distortion": True}
    with pytest.raises(ValueError):
        mk(distortion_weight=-1.0)


# ---- the reference by itself
def _frames():
    """(name, oracle forward) of every scene of the GPU tests, the two large ones also anti-aliased (the oracle at float32(o h))"""
    for name in DR.SCENES:
        d = DR.scene(name)
        yield name, run_oracle(d)
        if name in ("shell", "adversarial"):
            op = torch.from_numpy(np.float32(AA.o_eff(d))).reshape(d["opacities"].shape)
            yield name + "+aa", run_oracle(dict(d, opacities=op))


def test_scenes_are_what_the_gpu_tests_need():
    """the fp32 oracle alone keeps every scene inside the fragile-pixel cap (fragile_pixels asserts it) with no Gaussian on the
    alpha floor; the shell's longest list exceeds two 64-entry gather rounds; the hand-built scenes hold the pixels they are for"""
    for name, o in _frames():
        assert int(fragile_pixels(o).sum()) <= max(1, o["W"] * o["H"] // 5000), name
        r = DR.evaluate(o)
        assert int((r["fragile"] > 0).sum()) == 0, name
        longest = int((o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0]).max())
        if name.startswith("shell"):
            assert (o["W"], o["H"]) == (40, 24) and longest > 2 * 64, longest
        if name == "hand":
            assert set(np.unique(r["count"])) == {0, 1, 3}
            assert r["count"][0, 0] == 0 and (r["D"][r["count"] < 2] == 0.0).all()
        if name == "opaque-front":
            assert (o["n_contrib"] == 4).all() and (r["count"] == 4).all() and longest == 36
        if name == "two-layers":
            assert (r["count"] == 2).all()


def test_closed_forms_agree_with_the_literal_double_sum():
    """D from the prefix recurrence against sum_ij w_i w_j |z_i - z_j| written out, both float64: they differ by the rounding
    of at most n_contrib terms each, 1e-12 of the budget; the tie of the hand-built scene contributes nothing, and two constant
    layers give 2 a1 a2 (1 - a1) (z2 - z1)"""
    for name, o in _frames():
        r = DR.evaluate(o)
        err = float((np.abs(r["D"] - r["D_literal"]) / (1e-300 + r["D_budget"]))[r["D_budget"] > 0].max(initial=0.0))
        print(f"[distortion] {name}: recurrence vs literal double sum, error / budget {err:.2e}")
        assert err <= 1e-12, name
        assert (r["D"][r["D_budget"] == 0] == 0.0).all() and (r["D_literal"] >= 0.0).all()
    d = DR.scene("hand")
    o = run_oracle(d)
    r = DR.evaluate(o)
    z = o["depths"].astype(np.float64)
    assert z[0] == z[1] < z[2]
    py, px = np.unravel_index(np.argmax(r["D"]), r["D"].shape)
    a = []
    for i in range(3):
        dx, dy = float(o["xy"][i, 0]) - px, float(o["xy"][i, 1]) - py
        A, B, Cc, op = o["conic_opacity"][i].astype(np.float64)
        a.append(op * np.exp(-0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy))
    w = [a[0], a[1] * (1 - a[0]), a[2] * (1 - a[0]) * (1 - a[1])]
    assert abs(r["D"][py, px] - 2.0 * (w[0] + w[1]) * w[2] * (z[2] - z[0])) <= 1e-14
    o2 = run_oracle(DR.scene("two-layers"))
    r2 = DR.evaluate(o2)
    z1, z2 = o2["depths"].astype(np.float64)
    a1, a2 = 0.6, 0.5
    # (G = 1 - 4e-6 at the edge: alpha is constant to that)
    assert np.abs(r2["D"] - DR.closed_form_two_layers(a1, a2, z1, z2)).max() <= 2e-5 * DR.closed_form_two_layers(a1, a2, z1, z2)


def test_k_is_four_times_the_float32_twins_share():
    worst = 0.0
    for name, o in _frames():
        g = torch.randn(o["H"], o["W"], generator=torch.Generator().manual_seed(1)).numpy()
        share = DR.fp32_share(o, g)
        print(f"[distortion] {name}: float32 twin's share of the budget " + ", ".join(f"{k} {v:.2f}" for k, v in share.items()))
        worst = max(worst, max(share.values()))
    print(f"[distortion] largest share {worst:.2f}; MEASURED_SHARE {DR.MEASURED_SHARE}, K {DR.K}")
    assert worst <= DR.MEASURED_SHARE and abs(worst - DR.MEASURED_SHARE) <= 0.01 * DR.MEASURED_SHARE
    assert 4.0 * DR.MEASURED_SHARE <= DR.K <= 4.0 * DR.MEASURED_SHARE + 2.0


def test_gradients_of_the_reference_match_finite_differences():
    """the reference's accumulator sums against central differences of its own forward in the records (float64): z, opacity and
    the mean of one Gaussian of the hand-built scene that sits in the middle of a pixel's walk"""
    d = DR.scene("hand")
    o = run_oracle(d)
    g = torch.randn(o["H"], o["W"], generator=torch.Generator().manual_seed(2)).numpy().astype(np.float64)
    r = DR.evaluate(o, None, g)
    loss = lambda oo: float((DR.evaluate(oo)["D"] * g).sum())

    def bumped(key, idx, h):
        a = o[key].astype(np.float64).copy()
        a[idx] += h
        return dict(o, **{key: a})
    # (evaluate() reads the records through float32 for depths only; bump by exactly representable steps)
    i = 2
    h = 2.0 ** -10
    fd = lambda key, idx: (loss(bumped(key, idx, h)) - loss(bumped(key, idx, -h))) / (2 * h)
    got = dict(z=r["z"][i], opacity=r["opacity"][i], mx=r["mean2D"][i, 0] / (0.5 * o["W"]), my=r["mean2D"][i, 1] / (0.5 * o["H"]))
    want = dict(z=fd("depths", i), opacity=fd("conic_opacity", (i, 3)), mx=fd("xy", (i, 0)), my=fd("xy", (i, 1)))
    for k in got:
        print(f"[distortion] finite difference {k}: {got[k]:.6e} vs {want[k]:.6e}")
        assert abs(got[k] - want[k]) <= 1e-4 * max(1e-3, abs(want[k])), k
