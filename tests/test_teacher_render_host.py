"""Host checks of the teacher renderer (gaussian_gan_decoder_amd/teacher.py) and of tests/_teacher_render_ref.py: camera_rays
bit for bit against the reference's RaySampler, the torch form against every case the reference's own code produced
(tests/golden/teacher_render_fixture.npz), the float64 restatement against the same values -- which is where the *_MEASURED
constants and with them every tolerance come from -- and the refusals."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import _capi, density, teacher
from gaussian_gan_decoder_amd.decoder import planes_channels_last
import _teacher_render_ref as T

OUTPUTS = ("features", "weights", "depth")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _inputs(c):
    return (planes_channels_last(c.planes, c.D or None), density.osg_weights(c.decoder), torch.from_numpy(c.origins),
            torch.from_numpy(c.dirs))


def _noise(c):
    return torch.from_numpy(c.u_coarse), torch.from_numpy(c.u_fine)


@functools.lru_cache(maxsize=None)
def _table(Nc):
    table, delta = teacher.coarse_table(2.25, 3.3, Nc)
    return table.numpy(), delta


@functools.lru_cache(maxsize=None)
def _measured(name):
    """worst deviation of the reference's own fp32 values from the float64 restatement fed the same fp32 inputs, per stage"""
    c = T.case(name)
    imp = T.worst(c.depths_fine, T.importance(c.depths_coarse, c.sigma[:, :c.Nc], c.u_fine)) if c.Ni else 0.0
    r = T.composite(np.concatenate([c.depths_coarse, c.depths_fine], 1), c.sigma, c.rgb, c.white_back, c.scaled)
    comp = {k: T.worst(getattr(c, k), getattr(r, k)) for k in OUTPUTS}
    r, _ = T.end_to_end(c, *_table(c.Nc))
    e2e = {k: T.worst(getattr(c, k), getattr(r, k)) for k in OUTPUTS}
    return imp, comp, e2e


def test_camera_rays_are_bit_equal_to_the_ray_sampler():
    f = T.FIX
    o, d = teacher.camera_rays(torch.from_numpy(f["rays_cam2world"]), torch.from_numpy(f["rays_intrinsics"]), 5)
    assert o.shape == d.shape == (2 * 25, 3) and o.dtype == torch.float32
    assert float(np.abs(f["rays_intrinsics"][:, 0, 1]).min()) > 0           # both cameras are skewed
    assert np.array_equal(_bits(o.numpy()), _bits(f["rays_origins"].reshape(-1, 3)))
    assert np.array_equal(_bits(d.numpy()), _bits(f["rays_dirs"].reshape(-1, 3)))


def test_fixture_holds_the_cases_the_issue_names():
    cs = [T.case(n) for n in T.CASES]
    assert [(c.Nc, c.Ni, c.resolution) for c in cs] == [(48, 48, 6), (8, 5, 5), (48, 0, 4), (64, 64, 4), (33, 64, 0)]
    assert [(c.axes, c.D, c.act, c.crop, c.white_back, c.box_warp) for c in cs] == [
        ("panohead", 3, "sigmoid", 0.1, False, 1.0), ("panohead", 1, "lrelu", 0.05, True, 0.7), ("panohead", 3, "none", 0.1, False, 1.0),
        ("eg3d", 0, "sigmoid", None, False, 1.0), ("panohead", 3, "sigmoid", 0.1, False, 1.0)]
    for c in cs:
        assert c.M == (c.resolution ** 2 or 16)
        fine = T.coordinates(c.origins, c.dirs, c.depths_fine)
        assert not T.near_crop_rays(c, fine).any(), "the fixture needs no ray left out"
    c = cs[4]
    miss = c.weights == 0
    assert int(miss.sum()) >= 4
    assert (c.features[miss] == 0).all() and (c.depth[miss] == max(c.depths_coarse.max(), c.depths_fine.max())).all()


@pytest.mark.parametrize("name", T.CASES)
def test_torch_form_reproduces_the_reference(name):
    """render_teacher_torch on CPU tensors: coarse depths and coordinates bit-equal, everything else inside the tolerances"""
    c = T.case(name)
    cl, w, o, d = _inputs(c)
    out = teacher.render_teacher(cl, w, o, d, noise=_noise(c), return_samples=True, **T.render_kwargs(c))
    s = out.samples
    assert np.array_equal(_bits(s.depths_coarse.numpy()), _bits(c.depths_coarse))
    assert np.array_equal(_bits(s.coords_coarse.numpy()), _bits(T.coordinates(c.origins, c.dirs, c.depths_coarse)))
    assert s.depths_fine.shape == (c.M, c.Ni) and s.rgb_fine.shape == (c.M, c.Ni, 32)
    fine = T.worst(s.depths_fine.numpy(), c.depths_fine)
    got = dict(features=T.as_stored(c, out.features).numpy(), weights=out.weights.numpy(), depth=out.depth.numpy())
    dev = {k: T.worst(got[k], getattr(c, k)) for k in OUTPUTS}
    print(f"\n  {name}: fine depths {fine:.3e} (tolerance {T.TOL_IMPORTANCE:.3e}), outputs {dev}")
    assert fine <= T.TOL_IMPORTANCE
    for k in OUTPUTS:
        assert dev[k] <= getattr(T.TOL_END_TO_END, k), k
    # the coarse samples sit at bit-equal coordinates: the field as tests/test_density_host.py accepts it; cropped ones exact
    assert float(np.abs(s.sigma_coarse.numpy() - c.sigma[:, :c.Nc]).max()) <= 1e-5
    assert float(np.abs(s.rgb_coarse.numpy() - c.rgb[:, :c.Nc]).max()) <= 1e-5
    assert np.array_equal(s.sigma_coarse.numpy() == -1e3, c.sigma[:, :c.Nc] == -1e3)


@pytest.mark.parametrize("name", T.CASES)
def test_float64_restatement_against_the_reference(name):
    """the reference's own fp32 values stand within *_MEASURED of the float64 restatement, stage by stage; the coarse depths of
    the restatement are the reference's bit for bit"""
    c = T.case(name)
    table, delta = _table(c.Nc)
    assert np.array_equal(_bits(T.coarse_depths(table, delta, c.u_coarse)), _bits(c.depths_coarse))
    imp, comp, e2e = _measured(name)
    print(f"\n  {name}: importance {imp:.4e}; composite {comp}; end to end {e2e}")
    assert imp <= T.IMPORTANCE_MEASURED
    for k in OUTPUTS:
        assert comp[k] <= getattr(T.COMPOSITE_MEASURED, k) and e2e[k] <= getattr(T.END_TO_END_MEASURED, k), k


def test_measured_constants_are_what_is_measured_here():
    """neither tighter nor wider: each constant is the worst deviation over the fixture, rounded up in its fourth digit at most"""
    ms = [_measured(n) for n in T.CASES]
    pairs = [("importance", max(m[0] for m in ms), T.IMPORTANCE_MEASURED)]
    for k in OUTPUTS:
        pairs.append(("composite " + k, max(m[1][k] for m in ms), getattr(T.COMPOSITE_MEASURED, k)))
        pairs.append(("end to end " + k, max(m[2][k] for m in ms), getattr(T.END_TO_END_MEASURED, k)))
    for what, measured, recorded in pairs:
        print(f"\n  {what}: measured {measured:.4e}, recorded {recorded:.4e}, tolerance {2 * recorded:.4e}")
        assert measured <= recorded <= 1.01 * measured, what
    assert T.TOL_IMPORTANCE == 2 * T.IMPORTANCE_MEASURED and T.TOL_END_TO_END.depth == 2 * T.END_TO_END_MEASURED.depth


def test_images_follow_synthesis():
    c = T.case(T.CASES[0])
    cl, w, o, d = _inputs(c)
    out = teacher.render_teacher(cl, w, o, d, noise=_noise(c), **T.render_kwargs(c))
    feat, depth, mask = out.images(c.resolution)
    R = c.resolution
    assert feat.shape == (1, 32, R, R) and depth.shape == (1, 1, R, R) and mask.shape == (1, 1, R, R) and out.samples is None
    assert torch.equal(feat[0, :, 2, 3], out.features[2 * R + 3] * 2 - 1)          # the sigmoid case: scaled to (-1, 1)
    assert torch.equal(mask[0, 0, 1, 4], out.weights[R + 4] * (1 + 2 * 0.001) - 0.001)
    assert torch.equal(depth.reshape(-1), out.depth)
    c = T.case(T.CASES[2])                                                         # activation "none": features unscaled
    cl, w, o, d = _inputs(c)
    out = teacher.render_teacher(cl, w, o, d, noise=_noise(c), **T.render_kwargs(c))
    assert torch.equal(out.images(c.resolution)[0].permute(0, 2, 3, 1).reshape(-1, 32), out.features)
    with pytest.raises(ValueError, match="whole number"):
        out.images(5)


def test_noise_is_drawn_with_the_generator():
    c = T.case(T.CASES[1])
    cl, w, o, d = _inputs(c)
    a = teacher.render_teacher(cl, w, o, d, generator=torch.Generator().manual_seed(3), **T.render_kwargs(c))
    b = teacher.render_teacher(cl, w, o, d, generator=torch.Generator().manual_seed(3), **T.render_kwargs(c))
    other = teacher.render_teacher(cl, w, o, d, generator=torch.Generator().manual_seed(4), **T.render_kwargs(c))
    assert torch.equal(a.features, b.features) and torch.equal(a.depth, b.depth) and not torch.equal(a.depth, other.depth)


def test_refusals():
    c = T.case(T.CASES[0])
    cl, w, o, d = _inputs(c)
    kw = T.render_kwargs(c)
    for fn in (teacher.render_teacher, teacher.render_teacher_torch):
        for name in ("disparity_space_sampling", "density_noise", "cull_clouds", "binarize_clouds"):
            with pytest.raises(ValueError, match=name):
                fn(cl, w, o, d, **kw, **{name: 0.5})
            fn(cl, w, o[:2], d[:2], **kw, **{name: 0})                   # a rendering_kwargs' zero / False passes
        with pytest.raises(TypeError, match="unexpected"):
            fn(cl, w, o, d, **kw, clamp_mode="softplus")
        with pytest.raises(ValueError, match="auto"):
            fn(cl, w, o, d, **dict(kw, ray_start="auto", ray_end="auto"))
        with pytest.raises(ValueError, match="ray_start < ray_end"):
            fn(cl, w, o, d, **dict(kw, ray_start=3.3, ray_end=2.25))
        for bad in (3, 65):
            with pytest.raises(ValueError, match="depth_resolution ="):
                fn(cl, w, o, d, **dict(kw, depth_resolution=bad))
        for bad in (-1, 65):
            with pytest.raises(ValueError, match="depth_resolution_importance ="):
                fn(cl, w, o, d, **dict(kw, depth_resolution_importance=bad))
        with pytest.raises(ValueError, match="noise"):
            fn(cl, w, o, d, noise=(torch.zeros(c.M, c.Nc), torch.zeros(c.M, c.Ni + 1)), **kw)
        with pytest.raises(ValueError, match=r"origins \[M, 3\]"):
            fn(cl, w, o, d[:3], **kw)
        with pytest.raises(ValueError, match="channels"):                 # what the field refuses
            fn(torch.zeros(3, 3, 12, 10, 16), w, o, d, **kw)
        with pytest.raises(ValueError, match="EG3D plane axes"):
            fn(planes_channels_last(T.case(T.CASES[3]).planes, None), w, o, d, **dict(kw, triplane_depth=None))
        with pytest.raises(ValueError, match="one device"):
            fn(cl, w, o.to("meta"), d.to("meta"), **kw)


def test_new_entry_point_is_declared_and_bound():
    hdr = open(os.path.join(T.ROOT, "include", "ggd_raster.h")).read()
    assert "ggd_teacher_render" in _capi.EXPORTS and "int ggd_teacher_render(" in hdr
    assert "double ray_start, double ray_end" in hdr and "double crop_limit" in hdr
    from gaussian_gan_decoder_amd import build
    assert "ggd_teacher.hip" in build.SOURCES and "ggd_density_launch.h" in build.HEADERS
