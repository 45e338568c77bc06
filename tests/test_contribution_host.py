"""Contribution statistics, CPU side: the float64 reference (tests/_contrib_ref.py) against the oracle's own alpha map, the
fragile-row cap it is used under, ContributionStats' decoding, GaussianModel's scores and pruning mask against numpy, and every
refusal that is raised before a device call."""
from __future__ import annotations

import functools
import inspect
import math

import numpy as np
import pytest
import torch

import _contrib_ref as CR
import _instance_cases as IC

SCENES = ("P257-M9", "colors", "adversarial", "A1")


@functools.lru_cache(maxsize=None)
def _oracle(scene):
    return IC.reference(dict(scene=scene, feature="aux"))["o"]


@functools.lru_cache(maxsize=None)
def _reference(scene):
    return CR.of_forward(_oracle(scene))


@pytest.mark.parametrize("scene", SCENES)
def test_reference_conserves_the_oracles_alpha(scene):
    """sum_i sum_i = sum_pixels (1 - final_T): every pair's w leaves the pixel's transmittance"""
    o, ref = _oracle(scene), _reference(scene)
    total, alpha = float(ref["sum"].sum()), float((1.0 - o["final_T"].astype(np.float64)).sum())
    print(f"[contribution host] {scene}: sum of sums {total:.6f}, sum of alpha {alpha:.6f}, |d| = {abs(total - alpha):.2e} "
          f"of {1e-5 * o['W'] * o['H']:.2e}")
    assert abs(total - alpha) <= 1e-5 * o["W"] * o["H"]
    assert (ref["count"] >= 0).all() and ((ref["count"] == 0) == (ref["sum"] == 0.0)).all()
    assert (ref["max"] <= 0.99).all() and (ref["max"][ref["count"] > 0] >= CR.FLOOR * 1e-4).all()
    assert (ref["count"][o["radii"] == 0] == 0).all()
    assert int(ref["count"].sum()) <= int(o["n_contrib"].astype(np.int64).sum())


@pytest.mark.parametrize("scene", SCENES)
def test_fragile_rows_stay_within_the_cap(scene):
    ref = _reference(scene)
    P = ref["sum"].shape[0]
    rows = int((ref["own_fragile"] > 0).sum())
    print(f"[contribution host] {scene}: {rows} rows with a fragile pair, cap {CR.fragile_cap(P)}")
    assert rows <= CR.fragile_cap(P)
    assert (ref["slack"] <= ref["sum"] + 1e-12).all()


def test_reference_on_a_hand_built_pixel():
    """one 1 x 1 image, three records over the pixel: an opaque one, one under the floor, one behind"""
    xy = np.zeros((3, 2))
    co = np.array([[1.0, 0.0, 1.0, 0.5], [1.0, 0.0, 1.0, 0.003], [1.0, 0.0, 1.0, 0.25]])
    ref = CR.contribution_f64(np.array([[3]], np.uint32), np.array([0, 1, 2], np.uint32), np.array([[0, 3]], np.uint32), xy, co)
    np.testing.assert_allclose(ref["sum"], [0.5, 0.0, 0.125], rtol=0, atol=1e-15)
    np.testing.assert_allclose(ref["max"], [0.5, 0.0, 0.125], rtol=0, atol=1e-15)
    assert ref["count"].tolist() == [1, 0, 1]
    assert ref["own_fragile"].tolist() == [1, 1, 1]            # power = 0 exactly: within the window of the power > 0 skip
    np.testing.assert_allclose(ref["slack"], [0.0, 0.0, 0.125], rtol=0, atol=1e-15)
    short = CR.contribution_f64(np.array([[1]], np.uint32), np.array([0, 1, 2], np.uint32), np.array([[0, 3]], np.uint32), xy, co)
    assert short["count"].tolist() == [1, 0, 0]                # n_contrib bounds the walk


# ---- ContributionStats
def test_decoding_of_a_hand_built_raw():
    from gaussian_gan_decoder_amd.contribution import ContributionStats
    import diff_gaussian_rasterization as shim
    assert shim.ContributionStats is ContributionStats
    st = ContributionStats(4)
    assert st.raw.dtype == torch.int64 and tuple(st.raw.shape) == (4, 3) and not st.raw.any() and st.frames == 0 and st.P == 4
    bits = lambda x: int(np.float32(x).view(np.uint32))
    st.raw[0] = torch.tensor([1 << 24, 1, bits(1.0)])
    st.raw[1] = torch.tensor([(1 << 40) + 3, 70_000, bits(0.99)])          # a sum above 2^32
    st.raw[2] = torch.tensor([1, 1, bits(2.0 ** -24)])
    assert st.weight_sum.dtype == torch.float64 and st.weight_sum.tolist() == [1.0, 65536.0 + 3 * 2.0 ** -24, 2.0 ** -24, 0.0]
    assert st.pixel_count.dtype == torch.int64 and st.pixel_count.tolist() == [1, 70_000, 1, 0]
    assert st.weight_max.dtype == torch.float32
    assert st.weight_max.numpy().view(np.uint32).tolist() == [bits(1.0), bits(0.99), bits(2.0 ** -24), 0]
    for kind, want in (("sum", st.weight_sum.float()), ("max", st.weight_max), ("count", st.pixel_count.float())):
        got = st.score(kind)
        assert got.dtype == torch.float32 and torch.equal(got, want)
    with pytest.raises(ValueError, match="kind"):
        st.score("weight")
    st.frames = 3
    st.reset()
    assert not st.raw.any() and st.frames == 0


def _model(P, seed=0):
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel
    gen = torch.Generator().manual_seed(seed)
    pc = GaussianModel(0)
    pc._xyz = torch.randn(P, 3, generator=gen)
    pc._scaling = -4.0 + torch.randn(P, 3, generator=gen)
    pc._opacity = 2.0 * torch.randn(P, 1, generator=gen)
    return pc


def _stats(P, seed=1):
    from gaussian_gan_decoder_amd.contribution import ContributionStats
    gen = torch.Generator().manual_seed(seed)
    st = ContributionStats(P)
    st.raw[:, 1] = torch.randint(0, 40, (P,), generator=gen)
    w = torch.rand(P, generator=gen) * 0.99
    st.raw[:, 2] = torch.where(st.raw[:, 1] > 0, w.view(torch.int32).to(torch.int64), torch.zeros(P, dtype=torch.int64))
    st.raw[:, 0] = torch.where(st.raw[:, 1] > 0, (w.double() * 2.0 ** 24).round().to(torch.int64) * st.raw[:, 1], st.raw[:, 0])
    return st


def test_lightgaussian_score_against_numpy():
    P = 501
    pc, st = _model(P), _stats(P)
    got = pc.importance(st, "lightgaussian")
    assert got.dtype == torch.float32 and tuple(got.shape) == (P,)
    vol = np.exp(pc._scaling.numpy().astype(np.float64)).prod(1)
    op = 1.0 / (1.0 + np.exp(-pc._opacity.numpy().astype(np.float64).reshape(-1)))
    for power in (0.1, 0.5):
        want = st.raw[:, 1].numpy() * op * np.clip(vol / np.quantile(vol, 0.9), 0.0, 1.0) ** power
        got = pc.importance(st, "lightgaussian", volume_power=power).numpy()
        np.testing.assert_allclose(got, want, rtol=2e-5, atol=0)   # float32 exp, product, quantile and power: a few ulps each
    for kind in ("sum", "max", "count"):
        assert torch.equal(pc.importance(st, kind), st.score(kind))
    with pytest.raises(ValueError, match="kind"):
        pc.importance(st, "volume")


def test_prune_mask_and_its_stable_ties_against_numpy():
    P = 200
    pc, st = _model(P), _stats(P)
    st.raw[:, 1] = torch.arange(P) % 7                     # many ties: the count alone ranks
    count = st.raw[:, 1].numpy()
    for frac in (0.0, 0.013, 0.25, 0.5, 1.0):
        keep = min(P, math.ceil(frac * P))
        order = np.argsort(-count, kind="stable")          # descending, lower index first among equals
        want = np.ones(P, bool)
        want[order[:keep]] = False
        got = pc.contribution_prune_mask(st, keep_fraction=frac, kind="count")
        assert got.dtype == torch.bool and np.array_equal(got.numpy(), want), frac
    wmax = st.weight_max.numpy()
    got = pc.contribution_prune_mask(st, min_max_weight=0.3)
    assert np.array_equal(got.numpy(), wmax < np.float32(0.3))
    both = pc.contribution_prune_mask(st, keep_fraction=0.5, min_max_weight=0.3, kind="count")
    order = np.argsort(-count, kind="stable")
    want = wmax < np.float32(0.3)
    want[order[P // 2:]] = True
    assert np.array_equal(both.numpy(), want)


# ---- refusals before any device call
def test_statistics_tensor_refusals():
    from gaussian_gan_decoder_amd.contribution import ContributionStats, check_raw, resolve
    ok = torch.zeros(5, 3, dtype=torch.int64)
    assert check_raw(ok, 5, "cpu") is ok
    bad = {"P": (torch.zeros(4, 3, dtype=torch.int64), "dimensions"), "columns": (torch.zeros(5, 2, dtype=torch.int64), "dimensions"),
           "dtype": (torch.zeros(5, 3, dtype=torch.int32), "int64"), "float": (torch.zeros(5, 3), "int64"),
           "non-contiguous": (torch.zeros(3, 5, dtype=torch.int64).t(), "contiguous"), "no tensor": ([[0, 0, 0]] * 5, "tensor")}
    for what, (raw, match) in bad.items():
        with pytest.raises(ValueError, match=match):
            check_raw(raw, 5, "cpu")
    with pytest.raises(ValueError, match="expected cuda:0"):
        check_raw(ok, 5, torch.device("cuda:0"))
    assert resolve(None, 5, "cpu") is None and resolve(False, 5, "cpu") is None
    fresh = resolve(True, 5, "cpu")
    assert isinstance(fresh, ContributionStats) and fresh.P == 5 and resolve(fresh, 5, "cpu") is fresh
    with pytest.raises(ValueError, match="dimensions"):
        resolve(fresh, 6, "cpu")
    with pytest.raises(ValueError, match="ContributionStats or True"):
        resolve(ok, 5, "cpu")


def test_render_refuses_before_anything_is_built():
    from gaussian_gan_decoder_amd.contribution import ContributionStats
    from gaussian_gan_decoder_amd.gaussian_renderer import render, render_simple
    pc = _model(5)
    wrong = ContributionStats(6)
    with pytest.raises(ValueError, match="dimensions"):
        render_simple(None, pc, None, contribution=wrong)       # (no camera, no background: nothing else is looked at)
    with pytest.raises(ValueError, match="dimensions"):
        render(None, pc, None, None, contribution=wrong)
    sliced = ContributionStats(5)
    sliced.raw = torch.zeros(5, 6, dtype=torch.int64)[:, ::2]
    with pytest.raises(ValueError, match="contiguous"):
        render_simple(None, pc, None, contribution=sliced)
    with pytest.raises(ValueError, match="ContributionStats or True"):
        render_simple(None, pc, None, contribution=torch.zeros(5, 3, dtype=torch.int64))


def test_model_refusals():
    from gaussian_gan_decoder_amd.contribution import ContributionStats
    pc, st = _model(8), _stats(8)
    with pytest.raises(ValueError, match="keep_fraction, min_max_weight"):
        pc.prune_by_contribution(st)
    with pytest.raises(ValueError, match="keep_fraction"):
        pc.prune_by_contribution(st, keep_fraction=1.5)
    with pytest.raises(ValueError, match="rows"):
        pc.prune_by_contribution(ContributionStats(9), keep_fraction=0.5)
    with pytest.raises(ValueError, match="ContributionStats"):
        pc.importance(st.raw)
    with pytest.raises(ValueError, match="kind"):
        pc.prune_by_contribution(st, keep_fraction=0.5, kind="weights")


def test_settings_carry_the_attribute_and_the_pipeline_refuses_it():
    from gaussian_gan_decoder_amd.rasterizer import FramePipeline, GaussianRasterizationSettings, rasterize_gaussians_native
    z = torch.zeros(3)
    fields = (4, 4, 1.0, 1.0, z, 1.0, z, z, 0, z, False, False)
    plain = GaussianRasterizationSettings(*fields)
    assert plain.contribution is None and len(plain) == 14 and "contribution" not in repr(plain)
    raw = torch.zeros(7, 3, dtype=torch.int64)
    rs = GaussianRasterizationSettings(*fields, contribution=raw)
    assert rs.contribution is raw and len(rs) == 14 and rs._fields == plain._fields and tuple(rs)[:4] == tuple(plain)[:4]
    moved = rs._replace(image_height=9)
    assert moved.contribution is raw and moved.image_height == 9 and moved._replace(contribution=None).contribution is None
    assert "contribution" in repr(rs)
    with pytest.raises(TypeError):                         # positional: the tuple's fields stay what they are
        GaussianRasterizationSettings(*fields, False, False, raw)
    assert "contribution" in inspect.signature(rasterize_gaussians_native).parameters
    assert inspect.signature(rasterize_gaussians_native).parameters["contribution"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "contribution" not in inspect.signature(FramePipeline.submit).parameters   # out of scope: a TypeError at the call
    with pytest.raises(ValueError, match="int64"):         # refused before any device call (no device here)
        rasterize_gaussians_native(z, torch.zeros(7, 3), z, z, z, z, 1.0, z, z, z, 1.0, 1.0, 4, 4, z, 0, z, False, False,
                                   contribution=raw.float())
