"""The feature maps without a GPU: the reference construction of tests/_features_ref.py (pseudo-colour triples through the
unchanged oracle) equals a direct float64 C-channel blend, the two entry points are declared and exported, the kernels are in the
library, and the Python layer refuses bad feature inputs before any native call."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest
import torch

import _features_ref as FR
from _util import run_oracle, scene_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_triples_equal_a_direct_float64_blend():
    """One tiny scene, C = 5 (two triples, the second padded with one zero channel), non-zero background.  The oracle blends each
    triple in fp32 with its own exp; the direct blend is float64 with the fp32 run's contributor bounds: per pixel the two differ
    by the fp32 rounding of at most n_contrib weights that sum to <= 1 against features in [0, 1) -- 1e-5, the project's colour bar,
    outside the oracle's own fragile pixels (where float64 may take the other side of a threshold)."""
    from oracle import ggd_oracle as O
    d = scene_inputs(P=120, size=24, width=24, height=20, lsm=-4.0, seed=81)
    o = run_oracle(d)
    gen = torch.Generator().manual_seed(82)
    f = torch.rand(d["P"], 5, generator=gen).numpy()
    bg = np.array([0.3, 0.0, 0.7, 0.2, 0.9], np.float32)
    tr = FR.triples(f, bg)
    assert [ch for _, _, ch in tr] == [[0, 1, 2], [3, 4]]
    np.testing.assert_array_equal(tr[1][0][:, 2], 0.0)
    np.testing.assert_array_equal(tr[1][1], np.array([0.2, 0.9, 0.0], np.float32))
    F = FR.forward_ref(o, f, bg)
    F64 = FR.blend_f64(o, f, bg)
    assert F.shape == (5, d["H"], d["W"]) and int(o["n_contrib"].max()) > 3
    ok = ~O.fragile_pixels(o)
    assert ok.sum() >= ok.size - 2
    err = float(np.abs(F - F64)[:, ok].max())
    print(f"[features] triples vs direct float64 blend: max |dF| = {err:.2e}")
    assert err <= 1e-5
    # the colour itself is the same construction: features = the oracle's rgb, background = its bg
    Fc = FR.forward_ref(o, o["rgb"], o["bg"])
    np.testing.assert_array_equal(Fc, o["color"])


def test_entry_points_are_declared_and_exported(native_lib):
    from gaussian_gan_decoder_amd import _capi
    header = open(os.path.join(ROOT, "include", "ggd_raster.h")).read()
    for sym in ("ggd_forward_features", "ggd_backward_features"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
        assert sym in _capi.EXPORTS
        assert hasattr(native_lib, sym)
    assert int(re.search(r"#define\s+GGD_FEATURES_MAX_CHANNELS\s+(\d+)", header).group(1)) == _capi.FEATURES_MAX_CHANNELS == 32
    assert int(re.search(r"#define\s+GGD_FEATURES_ROUND\s+(\d+)", header).group(1)) == _capi.FEATURES_ROUND


def test_feature_kernels_are_built_without_spills(native_lib):
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    from gaussian_gan_decoder_amd import _capi
    tab = {kr.short(k): v for k, v in kr.kernel_resources(_capi.LIB_PATH).items()}
    fwd = sorted(k for k in tab if k.startswith("features_forward_kernel<"))
    bwd = sorted(k for k in tab if k.startswith("features_backward_kernel<"))
    assert fwd == sorted(f"features_forward_kernel<{em}, {cg}>" for em in range(3) for cg in (4, 8, 16, 32)), fwd
    assert bwd == sorted(f"features_backward_kernel<{em}, {cg}>" for em in range(4) for cg in (4, 8, 16, 32)), bwd
    for name in fwd + bwd:
        assert tab[name]["vgpr_spill"] == 0 and tab[name]["scratch"] == 0, (name, tab[name])
        assert tab[name]["lds"] <= 40960, (name, tab[name])       # at least four single-wave workgroups per CU (160 KB of LDS)


def _forward_args(P=4, H=8, W=8):
    e = torch.empty(0)
    return (torch.zeros(3), torch.zeros(P, 3), e, torch.ones(P, 1), torch.ones(P, 3), torch.ones(P, 4), 1.0, e, torch.eye(4),
            torch.eye(4), 1.0, 1.0, H, W, torch.zeros(P, 1, 3), 0, torch.zeros(3), False, False)


def _backward_args(H=8, W=8, P=4):
    e = torch.empty(0)
    return (torch.zeros(3), torch.zeros(P, 3), torch.zeros(P, dtype=torch.int32), e, torch.ones(P, 3), torch.ones(P, 4),
            1.0, e, torch.eye(4), torch.eye(4), 1.0, 1.0, torch.zeros(3, H, W), e, 0, torch.zeros(3), torch.empty(0),
            0, torch.empty(0), torch.empty(0), False)


BAD = {
    "C > 32": dict(features=torch.zeros(4, 33)),
    "not [P, C]: one row short": dict(features=torch.zeros(3, 5)),
    "not [P, C]: one dimension": dict(features=torch.zeros(20)),
    "not [P, C]: three dimensions": dict(features=torch.zeros(4, 5, 1)),
    "not [P, C]: no channel": dict(features=torch.zeros(4, 0)),
    "feature_bg: C - 1 elements": dict(features=torch.zeros(4, 5), feature_bg=torch.zeros(4)),
    "feature_bg: 3 elements": dict(features=torch.zeros(4, 32), feature_bg=torch.zeros(3)),
}


@pytest.fixture
def no_native(monkeypatch):
    from gaussian_gan_decoder_amd import _capi

    def fail(*a, **k):
        raise AssertionError("the native library was reached")
    for name in ("load", "context_for", "context_and_stream"):
        monkeypatch.setattr(_capi, name, fail)


@pytest.mark.parametrize("what", list(BAD))
def test_bad_feature_inputs_are_refused_before_any_native_call(no_native, what):
    from gaussian_gan_decoder_amd import rasterizer as R
    kw = BAD[what]
    with pytest.raises(ValueError):
        R.rasterize_gaussians_native(*_forward_args(), **kw)
    with pytest.raises(ValueError):
        R.rasterize_gaussians_backward_native(*_backward_args(), **kw)
    rs = R.GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                         False, False)
    with pytest.raises(ValueError):
        R.GaussianRasterizer(rs)(torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(4, 1), shs=torch.zeros(4, 1, 3),
                                 scales=torch.ones(4, 3), rotations=torch.ones(4, 4), **kw)


def test_features_with_absgrad_are_refused(no_native):
    from gaussian_gan_decoder_amd import rasterizer as R
    rs = R.GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                         False, False, absgrad=True)
    with pytest.raises(ValueError, match="colour terms"):
        R.GaussianRasterizer(rs)(torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(4, 1), shs=torch.zeros(4, 1, 3),
                                 scales=torch.ones(4, 3), rotations=torch.ones(4, 4), features=torch.zeros(4, 5))
    with pytest.raises(ValueError, match="colour terms"):
        R.rasterize_gaussians_backward_native(*_backward_args(), absgrad=True, features=torch.zeros(4, 5))


def test_cpu_tensors_raise_as_the_other_inputs_do(no_native):
    from gaussian_gan_decoder_amd import rasterizer as R
    with pytest.raises(RuntimeError, match="CPU"):
        R.rasterize_gaussians_native(*_forward_args(), features=torch.zeros(4, 5), feature_bg=torch.zeros(5))
    with pytest.raises(RuntimeError, match="CPU"):
        R.rasterize_gaussians_backward_native(*_backward_args(), features=torch.zeros(4, 5))


def test_signatures_default_to_no_features():
    import inspect
    from gaussian_gan_decoder_amd import gaussian_renderer as GR
    from gaussian_gan_decoder_amd import rasterizer as R
    for fn in (R.rasterize_gaussians, R.GaussianRasterizer.forward, GR.render, GR.render_simple, R.rasterize_gaussians_native):
        p = inspect.signature(fn).parameters
        assert p["features"].default is None and p["feature_bg"].default is None, fn
    assert "features" not in inspect.signature(R.FramePipeline.submit).parameters
