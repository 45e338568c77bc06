"""The absgrad extension, parts that need no GPU: the float64 helper the GPU tests hold the kernel to (tests/_absgrad_ref.py)
against the unchanged oracle, the settings keyword, and the densification statistics' refusal."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _absgrad_ref as AG
import _instance_cases as IC

SCENES = ("M1", "P257-M9")


def _oracle(scene):
    r = IC.reference(dict(scene=scene, seed=None, feature="aux"))
    return r["o"], r["frag"]


@pytest.mark.parametrize("scene", SCENES)
def test_helper_signed_sum_is_the_oracles(scene):
    """over the oracle's own forward state the helper's signed sum is backward_ref64's dL_dmeans2D.  1e-12 relative: of the
    element's sum of |terms| (the helper's abs), the scale at which two float64 summation orders of a cancelling sum can agree;
    the absolute sums dominate the signed ones elementwise."""
    from oracle import ggd_oracle as O
    o, frag = _oracle(scene)
    g, _, _ = IC.upstream_gradients(o["H"], o["W"], frag)
    ref, _, _ = O.backward_ref64(o, g.numpy())
    signed, absd = AG.blend_sums(AG.state_of(o), g.numpy())
    vis = (o["radii"] > 0)[:, None]
    want = ref["dL_dmeans2D"][:, :2]
    err = np.abs(signed * vis - want)
    scale = np.maximum(absd * vis, np.abs(want))
    worst = float((err / np.maximum(scale, 1e-300)).max(initial=0.0))
    print(f"[absgrad] {scene}: helper vs backward_ref64, worst error / sum of |terms| {worst:.2e}; "
          f"max |signed| {np.abs(want).max():.3e}, max abs {absd.max():.3e}")
    assert np.abs(want).max() > 0
    assert (err <= 1e-12 * scale).all(), worst
    assert (absd >= np.abs(signed)).all()
    assert (absd * vis > np.abs(want) * (1 + 1e-9)).any(), "no cancellation anywhere: the scene shows nothing"


@pytest.mark.parametrize("scene", SCENES)
def test_helper_with_depth_alpha_channels_is_the_sum_of_the_two_oracle_calls(scene):
    """the five-channel form (colour + the depth / alpha pseudo-colour) against the colour call plus the pseudo-colour call"""
    from oracle import ggd_oracle as O
    from _depth_alpha_ref import pseudo_rgb
    o, frag = _oracle(scene)
    g, gD, gA = IC.upstream_gradients(o["H"], o["W"], frag)
    ref, _, _ = O.backward_ref64(o, g.numpy())
    rgb = pseudo_rgb(o)
    g_aux = np.stack([gD.numpy()[0], gA.numpy()[0], np.zeros((o["H"], o["W"]), np.float32)])
    ref_a, _, _ = O.backward_ref64(dict(o, rgb=rgb, bg=np.zeros(3, np.float32), colors_precomp=rgb), g_aux)
    rgb5, bg5, g5 = AG.aux_channels(o, g.numpy(), gD.numpy()[0], gA.numpy()[0])
    signed, absd = AG.blend_sums(AG.state_of(o, rgb=rgb5, bg=bg5), g5)
    vis = (o["radii"] > 0)[:, None]
    want = (ref["dL_dmeans2D"] + ref_a["dL_dmeans2D"])[:, :2]
    scale = np.maximum(absd * vis, np.abs(want))
    assert (np.abs(signed * vis - want) <= 1e-12 * scale).all()
    assert (absd >= np.abs(signed)).all()


def _settings(**kw):
    from gaussian_gan_decoder_amd.rasterizer import GaussianRasterizationSettings
    z = torch.zeros(3)
    m = torch.eye(4)
    return GaussianRasterizationSettings(8, 8, 0.5, 0.5, z, 1.0, m, m, 0, z, False, False, **kw)


def test_settings_keyword():
    rs = _settings()
    assert rs.absgrad is False and "absgrad=False" in repr(rs)
    on = _settings(absgrad=True)
    assert on.absgrad is True and "absgrad=True" in repr(on) and len(on) == len(rs)
    moved = on._replace(image_width=16)
    assert moved.absgrad is True and moved.image_width == 16 and moved.antialiasing is False
    assert on._replace(absgrad=False).absgrad is False
    both = _settings(absgrad=True, antialiasing=True)._replace(sh_degree=2)
    assert both.absgrad and both.antialiasing and "antialiasing=True, absgrad=True" in repr(both)
    # the drop-in module hands out the same class
    import diff_gaussian_rasterization as shim
    assert shim.GaussianRasterizationSettings(*rs, absgrad=True).absgrad is True


@pytest.mark.parametrize("method", ["add_densification_stats", "update_densification_stats"])
def test_use_absgrad_without_the_attribute_raises(method):
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel
    pc = GaussianModel(0)
    pts = torch.zeros(4, 3, requires_grad=True)
    pts.grad = torch.ones(4, 3)          # a signed gradient alone is not enough
    second = torch.ones(4, dtype=torch.bool) if method.startswith("add") else torch.ones(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="absgrad"):
        getattr(pc, method)(pts, second, use_absgrad=True)
