"""The anti-aliasing option without a GPU: the ABI field sits where the spare word was, the new kernels are in the library
without spills or scratch, every new keyword defaults to off, the fp64 reference helper's h and gradient match finite
differences, and bad calls are refused in Python before any native call."""
from __future__ import annotations

import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import _antialias_ref as AA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    from gaussian_gan_decoder_amd import _capi
    return {kr.short(k): v for k, v in kr.kernel_resources(_capi.LIB_PATH).items()}


def _targs(name):
    m = re.search(r"<(.*)>$", name)
    return [a.strip() for a in m.group(1).split(",")] if m else []


def test_params_field_replaces_the_spare_word():
    from gaussian_gan_decoder_amd import _capi
    names = [f[0] for f in _capi.Params._fields_]
    assert "reserved_" not in names and names[-1] == "antialiasing"
    assert C.sizeof(_capi.Params) == 80
    assert _capi.Params.antialiasing.offset == _capi.Params.raw_attributes.offset + 4 == 76
    assert _capi.Params.antialiasing.size == 4
    text = open(os.path.join(ROOT, "include", "ggd_raster.h")).read()
    assert re.search(r"int32_t raw_attributes;.*?int32_t antialiasing;.*?\} ggd_params;", text, re.S)


def test_antialiasing_kernels_are_built_without_spills(native_lib):
    tab = _resources()
    # AA is the last template argument of preprocess_kernel<SHVEC, FOLD, AA> and the one before AUX in
    # preprocess_backward{,_vec}_kernel<AA, AUX> / preprocess_backward_staged_kernel<SHVEC, AA, AUX>
    fwd = {k: v for k, v in tab.items() if k.startswith("preprocess_kernel<") and _targs(k)[-1] == "true"}
    assert sorted(fwd) == sorted(f"preprocess_kernel<{sv}, {fo}, true>" for sv in ("false", "true")
                                 for fo in ("false", "true")), sorted(tab)          # SHVEC x FOLD
    bwd = {k: v for k, v in tab.items() if k.startswith("preprocess_backward") and _targs(k)[-2] == "true"}
    # the plain / vec / staged forms with the depth term off and on
    assert sorted(bwd) == sorted(["preprocess_backward_kernel<true, false>", "preprocess_backward_kernel<true, true>",
                                  "preprocess_backward_vec_kernel<true, false>", "preprocess_backward_vec_kernel<true, true>",
                                  "preprocess_backward_staged_kernel<false, true, false>",
                                  "preprocess_backward_staged_kernel<false, true, true>"]), sorted(tab)
    for name, r in {**fwd, **bwd}.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
    # the plain instances are the same templates with AA = false
    for name in ("preprocess_kernel<false, false, false>", "preprocess_kernel<true, true, false>",
                 "preprocess_backward_kernel<false, false>", "preprocess_backward_kernel<false, true>",
                 "preprocess_backward_staged_kernel<false, false, false>"):
        assert name in tab, name


def test_settings_and_keywords_default_to_off():
    import inspect
    from gaussian_gan_decoder_amd import rasterizer as R
    from gaussian_gan_decoder_amd import gaussian_renderer as GR
    from gaussian_gan_decoder_amd import train as T
    z3, eye = torch.zeros(3), torch.eye(4)
    rs = R.GaussianRasterizationSettings(8, 8, 1.0, 1.0, z3, 1.0, eye, eye, 0, z3, False, False)
    assert rs.antialiasing is False
    assert "antialiasing" not in R.GaussianRasterizationSettings._fields   # positions of the tuple fields unchanged
    on = R.GaussianRasterizationSettings(8, 8, 1.0, 1.0, z3, 1.0, eye, eye, 0, z3, False, False, antialiasing=True)
    assert on.antialiasing is True and on._replace(debug=True).antialiasing is True
    assert "antialiasing=True" in repr(on)
    keep = []
    dev = torch.device("cpu")
    assert R._params(rs, 4, 1, dev, keep).antialiasing == 0
    assert R._params(on, 4, 1, dev, keep).antialiasing == 1
    for fn in (R.rasterize_gaussians_native, R.rasterize_gaussians_backward_native, R.FramePipeline.submit, GR.render,
               GR.render_simple, T.DecoderTrainer.__init__):
        p = inspect.signature(fn).parameters["antialiasing"]
        assert p.default is False, fn
    for fn in (R.rasterize_gaussians_native, R.rasterize_gaussians_backward_native, R.FramePipeline.submit):
        assert inspect.signature(fn).parameters["antialiasing"].kind is inspect.Parameter.KEYWORD_ONLY, fn


def test_trainer_passes_the_flag_only_when_set():
    from gaussian_gan_decoder_amd.train import DecoderTrainer
    seen = []

    def fake_render(cam, gs, bg_color, **kw):
        seen.append(kw)
        raise RuntimeError("stop")
    for aa in (False, True):
        tr = DecoderTrainer("cpu", 1, plane_res=8, plane_channels=4, hidden_dim=8, image_size=8, render_fn=fake_render,
                            antialiasing=aa)
        assert tr.render_kwargs == ({"antialiasing": True} if aa else {})


def _scene(P=64, seed=0, use_cov=False, mod=1.0):
    """points well inside the frustum: the clamped view-space x / y the kernels treat as constants stay out of the
    finite-difference checks (their true derivative is not the convention's)"""
    from _util import scene_inputs
    d = scene_inputs(P=P, size=64, seed=seed, lsm=-4.5, use_cov=use_cov, scale_modifier=mod)
    d["means3D"] = (0.3 * d["means3D"]).contiguous()
    return d


def test_reference_h_matches_its_definition():
    d = _scene(P=32, seed=3)
    h, _ = AA.h_and_conditioning(d)
    m, _, _, cov6 = AA._inputs(d, False)
    x, z, y = (t.numpy() for t in AA.cov2d(d, m, cov6))
    det0, det1 = x * y - z * z, (x + 0.3) * (y + 0.3) - z * z
    np.testing.assert_allclose(h, np.sqrt(np.maximum(2.5e-5, det0 / det1)), rtol=1e-12)
    assert (det1 > det0).all() and (h <= 1.0).all()
    np.testing.assert_allclose(AA.o_eff(d), d["opacities"].double().numpy().reshape(-1) * h, rtol=1e-12)


def _fd_check(d, g, keys, rel_eps=1e-5, rtol=2e-5):
    """central differences of sum(g o h) w.r.t. every element of d[key] (step rel_eps * max |d[key]|), against AA.vjp"""
    got = AA.vjp(d, g)
    for key, out in keys:
        base = d[key].double().clone()
        eps = rel_eps * float(base.abs().max())
        num = np.zeros(base.numel())
        for j in range(base.numel()):
            vals = []
            for s in (1.0, -1.0):
                pert = base.clone().view(-1)
                pert[j] += s * eps
                dd = dict(d, **{key: pert.view(base.shape)})
                vals.append(float((np.asarray(g) * AA.o_eff(dd)).sum()))
            num[j] = (vals[0] - vals[1]) / (2 * eps)
        a = got[out].reshape(-1)
        scale = max(np.abs(num).max(), 1e-12)
        assert np.abs(a - num).max() <= rtol * scale + 1e-9, (key, np.abs(a - num).max(), scale)


@pytest.mark.parametrize("use_cov", [False, True])
def test_reference_gradient_matches_finite_differences(use_cov):
    d = _scene(P=6, seed=5, use_cov=use_cov, mod=0.8)
    d = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}
    g = np.random.default_rng(1).standard_normal(6)
    keys = [("means3D", "dL_dmeans3D"), ("opacities", "dL_dopacity")]
    keys += [("cov3D_precomp", "dL_dcov3D")] if use_cov else [("scales", "dL_dscales"), ("rotations", "dL_drots")]
    _fd_check(d, g, keys)


def test_reference_gradient_in_clamp_region_and_near_singular():
    """r <= 2.5e-5 (needle thinner than the filter): h is the constant floor, only dL/do = g h remains; a near-singular but
    unclamped covariance still matches its finite differences."""
    d = _scene(P=4, seed=7)
    d = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}
    sc = d["scales"].clone()
    sc[0] = torch.tensor([3e-2, 1e-8, 1e-8], dtype=torch.float64)    # clamped: det0 / det1 far below 2.5e-5
    sc[1] = torch.tensor([3e-2, 3e-2, 1e-8], dtype=torch.float64)    # flat disc: unclamped
    sc[2] = torch.tensor([4e-2, 2e-4, 1e-8], dtype=torch.float64)    # near-singular 2D covariance, r just above the floor
    d["scales"] = sc
    h, cond = AA.h_and_conditioning(d)
    assert h[0] == pytest.approx(math.sqrt(2.5e-5), rel=1e-12) and cond[0] == 1.0
    assert h[2] > math.sqrt(2.5e-5) and cond[2] > 10.0, (h, cond)
    g = np.array([1.0, 0.5, -0.7, 0.0])
    got = AA.vjp(d, g)
    assert np.abs(got["dL_dmeans3D"][0]).max() == 0.0 and np.abs(got["dL_dscales"][0]).max() == 0.0
    assert got["dL_dopacity"][0, 0] == pytest.approx(h[0])
    _fd_check(d, g, [("means3D", "dL_dmeans3D"), ("scales", "dL_dscales"), ("rotations", "dL_drots")], rel_eps=1e-6, rtol=1e-4)


def _bwd_args(H=8, W=8, P=4):
    e = torch.empty(0)
    return (torch.zeros(3), torch.zeros(P, 3), torch.zeros(P, dtype=torch.int32), e, torch.ones(P, 3), torch.ones(P, 4),
            1.0, e, torch.eye(4), torch.eye(4), 1.0, 1.0, torch.zeros(3, H, W), e, 0, torch.zeros(3), torch.empty(0),
            0, torch.empty(0), torch.empty(0), False)


def test_bad_calls_raise_before_any_native_call(monkeypatch):
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd import rasterizer as R

    def no_native(*a, **k):
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_capi, "load", no_native)
    monkeypatch.setattr(_capi, "context_for", no_native)
    monkeypatch.setattr(_capi, "context_and_stream", no_native)
    with pytest.raises(ValueError, match="opacities"):
        R.rasterize_gaussians_backward_native(*_bwd_args(), antialiasing=True)
    with pytest.raises(ValueError, match="opacities"):
        R.rasterize_gaussians_backward_native(*_bwd_args(), False, None, antialiasing=True)
    with pytest.raises(RuntimeError, match="CPU"):
        R.rasterize_gaussians_backward_native(*_bwd_args(), False, torch.ones(4, 1), antialiasing=True)
    e = torch.empty(0)
    with pytest.raises(RuntimeError, match="CPU"):
        R.rasterize_gaussians_native(torch.zeros(3), torch.zeros(4, 3), e, torch.ones(4, 1), torch.ones(4, 3),
                                     torch.ones(4, 4), 1.0, e, torch.eye(4), torch.eye(4), 1.0, 1.0, 8, 8,
                                     torch.zeros(4, 1, 3), 0, torch.zeros(3), False, False, antialiasing=True)
