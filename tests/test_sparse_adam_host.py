"""Sparse Adam without a GPU: the numpy restatement against float64 within a derived rounding bound, the C entry's
declaration / export / NULL-context refusals, the two import paths, and training_setup's optimizer_type switch.

Rounding bound of the float32 restatement (u = 2^-24, one rounding per operation): the two products and the sum of m' cost
at most 2 u (|b1 m| + |(1 - b1) g|); v' is a sum of non-negative terms, 3 u relative, halved by the square root, which adds
its own u, as does the sum with eps: under 3.5 u on the denominator; the product with lr and the division add 2 u.  That is
under 8 u on the update term lr (|b1 m| + |(1 - b1) g|) / (sqrt(v') + eps), plus u |p'| for the last sum:
    |p32 - p64| <= 2^-24 |p64| + 8 * 2^-24 * lr (|b1 m| + |(1 - b1) g|) / (sqrt(v') + eps)
"""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from _sparse_adam_ref import EPS, LRS, VISIBILITY, adam32, adam64, draw_group, visibility

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def training_args(**over):
    a = dict(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
             position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
    a.update(over)
    return SimpleNamespace(**a)


def cpu_model():
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel
    pc = GaussianModel(1)
    P = 5
    for attr, shape in (("_xyz", (P, 3)), ("_features_dc", (P, 1, 3)), ("_features_rest", (P, 3, 3)), ("_opacity", (P, 1)),
                        ("_scaling", (P, 3)), ("_rotation", (P, 4))):
        setattr(pc, attr, torch.nn.Parameter(torch.zeros(shape)))
    pc.spatial_lr_scale = 1.0
    return pc


def test_float32_restatement_within_the_rounding_bound_of_float64():
    u = 2.0 ** -24
    worst = 0.0
    for seed, lr in enumerate(LRS):
        rng = np.random.default_rng(100 + seed)
        N = 4099
        p, g, m, v = draw_group(rng, N, (5, 3), lr)
        for kind in VISIBILITY:
            vis = visibility(kind, N, rng)
            p32, m32, v32 = adam32(p, g, m, v, vis, lr)
            (p64, m64, v64), (mag, den) = adam64(p, g, m, v, vis, lr)
            bound = u * np.abs(p64) + 8 * u * (np.float64(np.float32(lr)) * mag / den)
            err = np.abs(p32.astype(np.float64) - p64)
            assert np.isfinite(err).all()
            assert (err[vis] <= bound[vis]).all(), (lr, kind, float((err[vis] / bound[vis]).max()))
            if vis.any() and lr:
                worst = max(worst, float((err[vis] / bound[vis]).max()))
            # the moments: two products and a sum, all terms of v' non-negative
            assert (np.abs(m32 - m64)[vis] <= 2 * u * mag[vis]).all()
            assert (np.abs(v32 - v64)[vis] <= 3 * u * v64[vis]).all()
            for new, old in ((p32, p), (m32, m), (v32, v)):
                assert np.array_equal(new[~vis].view(np.int32), old[~vis].view(np.int32))
    print(f"float32 restatement: worst error / bound = {worst:.3f}")
    assert worst > 0.01                                  # the bound is of the error's order, not a blanket


def test_restatement_copies_invisible_rows_bit_for_bit():
    rng = np.random.default_rng(3)
    N = 65
    p, g, m, v = draw_group(rng, N, (3,), 0.05)
    vis = visibility("every_other", N, rng)
    g[~vis] = np.nan
    m[~vis] = np.inf
    v[~vis] = np.float32(np.nan)
    out = adam32(p, g, m, v, vis, 0.05)
    for new, old in zip(out, (p, m, v)):
        assert np.array_equal(new[~vis].view(np.int32), old[~vis].view(np.int32))
        assert np.isfinite(new[vis]).all()
    assert not np.array_equal(out[0][vis], p[vis])


def test_entry_is_declared_listed_and_exported(native_lib):
    from gaussian_gan_decoder_amd import _capi, build
    hdr = open(os.path.join(ROOT, "include", "ggd_raster.h")).read()
    assert re.search(r"\bint\s+ggd_adam_sparse\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "ggd_adam_group" in hdr
    assert "ggd_adam_sparse" in _capi.EXPORTS and "ggd_adam.hip" in build.SOURCES
    assert hasattr(native_lib, "ggd_adam_sparse")
    assert C.sizeof(_capi.AdamGroup) == 48 and _capi.AdamGroup.width.offset == 32 and _capi.AdamGroup.eps.offset == 40


def test_null_context_is_refused(native_lib):
    from gaussian_gan_decoder_amd import _capi
    table = (_capi.AdamGroup * 1)()
    dummy = C.c_void_p(4096)                             # never dereferenced: the call returns before anything is launched
    for N, n_groups, tab, visible, radii in ((4, 1, table, dummy, None), (4, 1, table, None, dummy), (0, 1, table, dummy, None),
                                             (-1, 1, table, dummy, None), (4, 0, table, dummy, None), (4, 9, table, dummy, None),
                                             (4, 1, None, dummy, None), (4, 1, table, None, None), (4, 1, table, dummy, dummy)):
        assert native_lib.ggd_adam_sparse(None, None, N, n_groups, tab, visible, radii, 0.9, 0.999) != 0


def test_importable_from_both_module_paths():
    from diff_gaussian_rasterization import SparseGaussianAdam as shim
    from gaussian_gan_decoder_amd.sparse_adam import SparseGaussianAdam
    assert shim is SparseGaussianAdam and issubclass(SparseGaussianAdam, torch.optim.Adam)
    opt = SparseGaussianAdam([{"params": [torch.nn.Parameter(torch.zeros(4, 3))], "lr": 0.01, "name": "xyz"}], lr=0.0, eps=1e-15)
    assert opt.param_groups[0]["lr"] == 0.01 and opt.param_groups[0]["eps"] == 1e-15
    assert tuple(opt.param_groups[0]["betas"]) == (0.9, 0.999) and len(opt.state) == 0


def test_training_setup_refuses_an_unknown_optimizer_type():
    pc = cpu_model()
    with pytest.raises(ValueError, match="optimizer_type"):
        pc.training_setup(training_args(optimizer_type="adamw"))
    assert pc.optimizer is None


def test_training_setup_refuses_decoder_params_under_sparse_adam():
    pc = cpu_model()
    extra = [{"params": [torch.nn.Parameter(torch.zeros(7))], "lr": 0.001, "name": "decoder"}]
    with pytest.raises(ValueError, match="decoder_params"):
        pc.training_setup(training_args(optimizer_type="sparse_adam"), decoder_params=extra)
    assert pc.optimizer is None
    pc.training_setup(training_args(optimizer_type="default"), decoder_params=extra)     # today's path takes them
    assert type(pc.optimizer) is torch.optim.Adam and len(pc.optimizer.param_groups) == 7


def test_sparse_adam_setup_and_cpu_tensors_are_refused():
    from gaussian_gan_decoder_amd.sparse_adam import SparseGaussianAdam
    pc = cpu_model()
    pc.training_setup(training_args(optimizer_type="sparse_adam"))
    assert type(pc.optimizer) is SparseGaussianAdam
    assert [g["name"] for g in pc.optimizer.param_groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    assert all(g["eps"] == EPS for g in pc.optimizer.param_groups)
    assert pc.update_learning_rate(0) == pytest.approx(0.00016)
    for attr in ("_xyz", "_opacity"):
        getattr(pc, attr).grad = torch.ones_like(getattr(pc, attr))
    before = pc._xyz.detach().clone()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.optimizer.step(torch.ones(5, dtype=torch.bool), 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.optimizer.step(torch.ones(5, dtype=torch.int32), 5)
    assert torch.equal(pc._xyz.detach(), before) and len(pc.optimizer.state) == 0
    with pytest.raises(ValueError):
        pc.optimizer.step(torch.ones(5, dtype=torch.bool), -1)


def test_default_optimizer_is_unchanged_without_the_attribute():
    pc = cpu_model()
    args = training_args()
    assert not hasattr(args, "optimizer_type")
    pc.training_setup(args)
    assert type(pc.optimizer) is torch.optim.Adam
    groups = pc.optimizer.param_groups
    assert [g["name"] for g in groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    assert [g["lr"] for g in groups] == [0.00016, 0.0025, 0.0025 / 20.0, 0.05, 0.005, 0.001]
    assert all(g["eps"] == 1e-15 and tuple(g["betas"]) == (0.9, 0.999) and len(g["params"]) == 1 for g in groups)
    assert [g["params"][0] for g in groups] == [pc._xyz, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation]
    assert pc.xyz_gradient_accum.shape == (5, 1) and pc.denom.shape == (5, 1)
