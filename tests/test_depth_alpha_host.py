"""The depth / alpha extension without a GPU: its kernels are in the library with the resources the design assumes, the
settings default to the plain rasterizer, and bad inputs are refused in Python before any native call."""
from __future__ import annotations

import importlib.util
import os
import re

import pytest
import torch

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


def test_aux_kernels_are_built_without_spills(native_lib):
    tab = _resources()
    # AUX is the last template argument of every kernel that has the extension (false: the plain instance)
    fwd = {k: v for k, v in tab.items() if k.startswith("blend_forward_kernel<") and _targs(k)[-1] == "true"}
    bwd = {k: v for k, v in tab.items() if k.startswith("blend_backward_quarter_kernel<") and _targs(k)[-1] == "true"}
    ppb = {k: v for k, v in tab.items() if k.startswith("preprocess_backward") and _targs(k)[-1:] == ["true"]}
    assert len(fwd) == 6, sorted(tab)          # exp modes 0..2 x cull on / off
    assert len(bwd) == 8, sorted(tab)          # exp modes 0..3 x cull on / off
    assert sorted(fwd) == sorted(f"blend_forward_kernel<{em}, {cu}, false, true>"       # no statistics variant
                                 for em in range(3) for cu in ("false", "true")), sorted(fwd)
    assert sorted(bwd) == sorted(f"blend_backward_quarter_kernel<{em}, {cu}, false, true>"
                                 for em in range(4) for cu in ("false", "true")), sorted(bwd)
    assert {re.sub(r"<.*", "", k) for k in ppb} == {"preprocess_backward_kernel", "preprocess_backward_vec_kernel",
                                                     "preprocess_backward_staged_kernel"}, sorted(ppb)
    # the plain instances are the same templates with AUX = false
    for name in ("blend_forward_kernel<1, true, false, false>", "blend_forward_kernel<1, true, true, false>",
                 "blend_backward_quarter_kernel<3, true, false, false>", "blend_backward_quarter_kernel<3, true, true, false>",
                 "preprocess_backward_kernel<false, false>", "preprocess_backward_vec_kernel<false, false>",
                 "preprocess_backward_staged_kernel<false, false, false>"):
        assert name in tab, name
    for group in (fwd, bwd, ppb):
        for name, r in group.items():
            assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
    for name, r in fwd.items():                # the forward keeps 8 waves per SIMD
        assert r["vgpr"] <= 64 and r["lds"] <= 4096, (name, r)


def test_aux_entry_points_are_exported(native_lib):
    from gaussian_gan_decoder_amd import _capi
    for sym in ("ggd_forward_aux", "ggd_forward_render_aux", "ggd_backward_aux"):
        assert sym in _capi.EXPORTS
        assert hasattr(native_lib, sym)


def test_settings_default_to_plain_rasterizer():
    from gaussian_gan_decoder_amd.rasterizer import GaussianRasterizationSettings
    assert GaussianRasterizationSettings._fields[-1] == "render_depth_alpha"
    assert GaussianRasterizationSettings._fields[-2] == "raw_attributes"
    rs = GaussianRasterizationSettings(8, 8, 1.0, 1.0, None, 1.0, None, None, 0, None, False, False)
    assert rs.render_depth_alpha is False and rs.raw_attributes is False


def _backward_args(H=8, W=8, P=4):
    e = torch.empty(0)
    return (torch.zeros(3), torch.zeros(P, 3), torch.zeros(P, dtype=torch.int32), e, torch.ones(P, 3), torch.ones(P, 4),
            1.0, e, torch.eye(4), torch.eye(4), 1.0, 1.0, torch.zeros(3, H, W), e, 0, torch.zeros(3), torch.empty(0),
            0, torch.empty(0), torch.empty(0), False)


@pytest.mark.parametrize("shape", [(2, 8, 8), (8, 7), (64,), (1, 8, 9)])
def test_backward_rejects_wrong_aux_gradient_shapes(shape):
    from gaussian_gan_decoder_amd import rasterizer as R
    with pytest.raises(ValueError):
        R.rasterize_gaussians_backward_native(*_backward_args(), dL_ddepth=torch.zeros(shape))
    with pytest.raises(ValueError):
        R.rasterize_gaussians_backward_native(*_backward_args(), dL_dalpha=torch.zeros(shape))


def test_cpu_tensors_raise_before_any_native_call(monkeypatch):
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd import rasterizer as R

    def no_native(*a, **k):
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_capi, "load", no_native)
    monkeypatch.setattr(_capi, "context_for", no_native)
    monkeypatch.setattr(_capi, "context_and_stream", no_native)
    with pytest.raises(RuntimeError, match="CPU"):
        R.rasterize_gaussians_backward_native(*_backward_args(), dL_ddepth=torch.zeros(1, 8, 8), dL_dalpha=torch.zeros(8, 8))
    e = torch.empty(0)
    with pytest.raises(RuntimeError, match="CPU"):
        R.rasterize_gaussians_native(torch.zeros(3), torch.zeros(4, 3), e, torch.ones(4, 1), torch.ones(4, 3),
                                     torch.ones(4, 4), 1.0, e, torch.eye(4), torch.eye(4), 1.0, 1.0, 8, 8,
                                     torch.zeros(4, 1, 3), 0, torch.zeros(3), False, False, render_depth_alpha=True)
