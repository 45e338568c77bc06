"""The teacher renderer's kernels (csrc/ggd_teacher.hip: ggd_teacher_render) on the device, stage by stage against the float64
restatement of tests/_teacher_render_ref.py fed the GPU's own intermediate values, end to end against the values the reference's
own code produced (tests/golden/teacher_render_fixture.npz), and at the edges of the wave, workgroup and sample-count ranges.
Where the tolerances come from: tests/_teacher_render_ref.py; tests/test_teacher_render_host.py measures them on the host."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import _capi, density, teacher
from gaussian_gan_decoder_amd.decoder import planes_channels_last
import _teacher_render_ref as T

DEV = torch.device("cuda:0")
OUTPUTS = ("features", "weights", "depth")
SENTINEL = -7.25
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
AXES = {"eg3d": 0, "panohead": 1}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = T.case(name)
    return (c, planes_channels_last(c.planes, c.D or None).to(DEV), density.osg_weights(c.decoder).to(DEV),
            torch.from_numpy(c.origins).to(DEV), torch.from_numpy(c.dirs).to(DEV),
            (torch.from_numpy(c.u_coarse).to(DEV), torch.from_numpy(c.u_fine).to(DEV)))


@functools.lru_cache(maxsize=None)
def _render(name, white_back=None):
    """one render of a fixture case with its stored noise and every stage's values, shared by the tests (never modified)"""
    c, cl, w, o, d, noise = _inputs(name)
    kw = T.render_kwargs(c)
    if white_back is not None:
        kw["white_back"] = white_back
    return teacher.render_teacher(cl, w, o, d, noise=noise, return_samples=True, **kw)


def _union(s):
    return (np.concatenate([_np(s.depths_coarse), _np(s.depths_fine)], 1), np.concatenate([_np(s.sigma_coarse), _np(s.sigma_fine)], 1),
            np.concatenate([_np(s.rgb_coarse), _np(s.rgb_fine)], 1))


def _all_tensors(out):
    return [out.features, out.depth, out.weights] + list(out.samples)


# ---- 1: exact stages -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", T.CASES)
def test_exact_stages(native_lib, name):
    """coarse depths and coordinates bit-equal to the reference's; sigma (where the crop leaves it) and rgb bit-equal to
    sample_field at the returned coordinates, coarse and fine; cropped samples exactly -1e3; two runs bit-equal in everything"""
    c, cl, w, o, d, noise = _inputs(name)
    out = _render(name)
    s = out.samples
    assert torch.equal(_bits(s.depths_coarse), _bits(torch.from_numpy(c.depths_coarse).to(DEV)))
    assert torch.equal(_bits(s.coords_coarse), _bits(torch.from_numpy(T.coordinates(c.origins, c.dirs, c.depths_coarse)).to(DEV)))
    if c.Ni:
        fine = torch.from_numpy(T.coordinates(c.origins, c.dirs, _np(s.depths_fine))).to(DEV)
        assert torch.equal(_bits(s.coords_fine), _bits(fine))
    lim = T.crop_limit(c)
    n_cropped = 0
    for coords, sigma, rgb in ((s.coords_coarse, s.sigma_coarse, s.rgb_coarse), (s.coords_fine, s.sigma_fine, s.rgb_fine)):
        if coords.numel() == 0:
            continue
        fs, frgb = density.sample_field(cl, w, coords, c.box_warp, c.axes, c.D or None, want_rgb=True)
        assert torch.equal(_bits(rgb.reshape(-1, 32)), _bits(frgb))
        outside = torch.zeros_like(sigma, dtype=torch.bool) if lim is None else \
            ~((coords[..., 0].abs() <= float(lim)) & (coords[..., 2].abs() <= float(lim)))
        want = torch.where(outside, torch.full_like(sigma, -1e3), fs.view_as(sigma))
        assert torch.equal(_bits(sigma), _bits(want))
        n_cropped += int(outside.sum())
    if name == T.CASES[4]:
        assert n_cropped > 0
    again = teacher.render_teacher(cl, w, o, d, noise=noise, return_samples=True, **T.render_kwargs(c))
    for a, b in zip(_all_tensors(out), _all_tensors(again)):
        assert torch.equal(_bits(a), _bits(b)), "two runs differ"
    plain = teacher.render_teacher(cl, w, o, d, noise=noise, **T.render_kwargs(c))          # samples in the workspace
    for a, b in zip(_all_tensors(out)[:3], (plain.features, plain.depth, plain.weights)):
        assert torch.equal(_bits(a), _bits(b)), "the workspace form differs from the return_samples form"


# ---- 2: importance ---------------------------------------------------------------------------------------------------------------
def _check_importance(what, out, u_fine):
    s = out.samples
    want = T.importance(_np(s.depths_coarse), _np(s.sigma_coarse), _np(u_fine))
    dev = T.worst(_np(s.depths_fine), want)
    print(f"\n  {what}: fine depths, worst |gpu - float64| = {dev:.3e} (tolerance {T.TOL_IMPORTANCE:.3e})")
    assert dev <= T.TOL_IMPORTANCE, what


@pytest.mark.parametrize("name", [n for n in T.CASES if T.case(n).Ni])
def test_importance_stage(native_lib, name):
    _check_importance(name, _render(name), _inputs(name)[5][1])


@pytest.mark.parametrize("draw", ["u_fine=0", "u_fine<1", "u_fine constant", "u_coarse=0", "u_coarse<1"])
@pytest.mark.parametrize("name", [T.CASES[1], T.CASES[4]])
def test_importance_stage_edge_draws(native_lib, name, draw):
    c, cl, w, o, d, (uc, uf) = _inputs(name)
    uc, uf = {"u_fine=0": (uc, torch.zeros_like(uf)), "u_fine<1": (uc, torch.full_like(uf, BELOW_ONE)),
              "u_fine constant": (uc, torch.full_like(uf, 0.37)), "u_coarse=0": (torch.zeros_like(uc), uf),
              "u_coarse<1": (torch.full_like(uc, BELOW_ONE), uf)}[draw]
    out = teacher.render_teacher(cl, w, o, d, noise=(uc, uf), return_samples=True, **T.render_kwargs(c))
    _check_importance(f"{name} {draw}", out, uf)
    if draw == "u_fine constant":                     # all fine samples of a ray at one depth: ties in the merge
        assert bool((out.samples.depths_fine == out.samples.depths_fine[:, :1]).all())
    _check_composite(f"{name} {draw}", c, out, c.white_back)


# ---- 3: composite ----------------------------------------------------------------------------------------------------------------
def _check_composite(what, c, out, white_back):
    depths, sigma, rgb = _union(out.samples)
    want = T.composite(depths, sigma, rgb, white_back)
    dev = {k: T.worst(_np(getattr(out, k)), getattr(want, k)) for k in OUTPUTS}
    print(f"\n  {what}: composite, worst |gpu - float64| = {dev} (tolerances {vars(T.TOL_COMPOSITE)})")
    for k in OUTPUTS:
        assert dev[k] <= getattr(T.TOL_COMPOSITE, k), f"{what}: {k}"
    assert float(out.depth.min()) >= want.lo and float(out.depth.max()) <= want.hi
    return want


@pytest.mark.parametrize("name", T.CASES)
def test_composite_stage(native_lib, name):
    c = T.case(name)
    _check_composite(name, c, _render(name), c.white_back)


@pytest.mark.parametrize("white_back", [False, True])
def test_rays_that_miss_have_zero_weight_and_the_largest_depth(native_lib, white_back):
    name = T.CASES[4]
    c = T.case(name)
    out = _render(name, white_back)
    want = _check_composite(f"{name} white_back={white_back}", c, out, white_back)
    miss = torch.from_numpy(c.weights == 0).to(DEV)
    assert int(miss.sum()) >= 4
    assert bool((out.samples.sigma_coarse[miss] == -1e3).all()) and bool((out.samples.sigma_fine[miss] == -1e3).all())
    assert bool((out.weights[miss] == 0).all())
    assert bool((out.features[miss] == (1.0 if white_back else 0.0)).all())
    top = max(float(out.samples.depths_coarse.max()), float(out.samples.depths_fine.max()))
    assert top == want.hi and bool((out.depth[miss] == top).all())
    assert bool((out.weights[~miss] > 0).all())


# ---- 4: end to end ---------------------------------------------------------------------------------------------------------------
def _kept_rays(c, coords_fine):
    near = T.near_crop_rays(c, _np(coords_fine))
    assert int(near.sum()) <= 1, "more than one ray has a fine sample at the crop limit"
    return ~near


@pytest.mark.parametrize("name", T.CASES)
def test_end_to_end_against_the_reference(native_lib, name):
    c = T.case(name)
    out = _render(name)
    keep = _kept_rays(c, out.samples.coords_fine)
    got = dict(features=_np(T.as_stored(c, out.features)), weights=_np(out.weights), depth=_np(out.depth))
    dev = {k: T.worst(got[k], getattr(c, k), keep) for k in OUTPUTS}
    print(f"\n  {name}: end to end, worst |gpu - reference| = {dev} (tolerances {vars(T.TOL_END_TO_END)}), rays left out "
          f"{int((~keep).sum())}")
    for k in OUTPUTS:
        assert dev[k] <= getattr(T.TOL_END_TO_END, k), k


# ---- 5: edges ----------------------------------------------------------------------------------------------------------------
def _direct(c, cl, w, o, d, uc, uf, M, Nc, Ni, features, depth, weights, samples, **over):
    """ggd_teacher_render itself, into the caller's (over-allocated) buffers -> return code"""
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    cx, stream = _capi.context_and_stream(DEV)
    table, _ = teacher.coarse_table(2.25, 3.3, max(Nc, 2))
    a = dict(C=32, act=density.ACTIVATIONS[w.activation], ray_start=2.25, ray_end=3.3, lim=float(c.box_warp / 2 - c.crop), crop=1)
    a.update(over)
    with torch.cuda.device(DEV):
        return cx, cx.lib.ggd_teacher_render(cx.handle, C.c_void_p(stream), vp(cl), a["C"], c.D, cl.shape[-3], cl.shape[-2],
                                             AXES[c.axes], c.box_warp, vp(w.w1), vp(w.b1), vp(w.w2), vp(w.b2), a["act"], vp(o), vp(d), M,
                                             a["ray_start"], a["ray_end"], vp(table), Nc, Ni, vp(uc), vp(uf) if Ni > 0 else None,
                                             a["crop"], a["lim"], 0, vp(features), vp(depth), vp(weights), vp(samples))


def _buffers(M, Nc, Ni, pad=8):
    total = teacher.sample_layout(M, Nc, Ni)[2]
    mk = lambda *shape: torch.full(shape, SENTINEL, device=DEV)
    return mk(M + pad, 32), mk(M + pad), mk(M + pad), mk(total + 64), total


@pytest.mark.parametrize("Nc,Ni", [(4, 1), (64, 64), (48, 0)])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 63, 65])
def test_edges_of_rays_and_samples(native_lib, M, Nc, Ni):
    """ray counts around the four waves of a workgroup, M * Nc on both sides of the field kernel's 128-point workgroup, the
    smallest and largest sample counts and the coarse-only branch: sentinel rows behind every output untouched, the values those
    of the torch form on the device"""
    name = T.CASES[0]
    c, cl, w, o, d, _ = _inputs(name)
    idx = torch.arange(M, device=DEV) % c.M
    o, d = o[idx].contiguous(), d[idx].contiguous()
    g = torch.Generator(device=DEV).manual_seed(100 * M + Nc)
    uc, uf = torch.rand((M, Nc), device=DEV, generator=g), torch.rand((M, Ni), device=DEV, generator=g)
    features, depth, weights, samples, total = _buffers(M, Nc, Ni)
    cx, rc = _direct(c, cl, w, o, d, uc, uf, M, Nc, Ni, features, depth, weights, samples)
    cx.check(rc)
    for buf, used in ((features, M), (depth, M), (weights, M), (samples, total)):
        assert bool((buf[used:] == SENTINEL).all()), "rows behind an output were written"
        assert not bool((buf[:used] == SENTINEL).any()), "an output row was not written"
    kw = dict(T.render_kwargs(c), depth_resolution=Nc, depth_resolution_importance=Ni)
    ref = teacher.render_teacher_torch(cl, w, o, d, noise=(uc, uf), return_samples=True, **kw)
    off, shapes, _ = teacher.sample_layout(M, Nc, Ni)
    part = lambda k: samples[off[k]:off[k] + int(np.prod(shapes[k]))].view(shapes[k])
    assert torch.equal(_bits(part("depths_coarse")), _bits(ref.samples.depths_coarse))
    keep = torch.from_numpy(_kept_rays(c, part("coords_fine")) & _kept_rays(c, ref.samples.coords_fine)).to(DEV)
    got = dict(features=features[:M], weights=weights[:M], depth=depth[:M])
    dev = {k: T.worst(_np(got[k][keep]), _np(getattr(ref, k)[keep])) for k in OUTPUTS}
    print(f"\n  M={M} Nc={Nc} Ni={Ni}: worst |kernels - torch form| = {dev}")
    for k in OUTPUTS:
        assert dev[k] <= getattr(T.TOL_END_TO_END, k), k


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,Nc,Ni,over", [
    ("Nc=3", 3, 4, {}), ("Nc=65", 65, 4, {}), ("Ni=65", 8, 65, {}), ("Ni=-1", 8, -1, {}),
    ("ray_start=ray_end", 8, 4, dict(ray_start=2.25, ray_end=2.25)), ("ray_start>ray_end", 8, 4, dict(ray_start=3.3, ray_end=2.25)),
    ("ray_end=inf", 8, 4, dict(ray_end=float("inf"))), ("ray_start=nan", 8, 4, dict(ray_start=float("nan"))),
    ("crop limit nan", 8, 4, dict(lim=float("nan"))), ("16 channels", 8, 4, dict(C=16)), ("activation 3", 8, 4, dict(act=3))])
def test_refusals_through_the_c_abi_launch_nothing(native_lib, what, Nc, Ni, over):
    name = T.CASES[0]
    c, cl, w, o, d, _ = _inputs(name)
    M = 5
    uc, uf = torch.zeros((M, 64), device=DEV), torch.zeros((M, 64), device=DEV)
    features, depth, weights, samples, _ = _buffers(M, 64, 64)
    cx, rc = _direct(c, cl, w, o[:M].contiguous(), d[:M].contiguous(), uc, uf, M, Nc, Ni, features, depth, weights, samples, **over)
    assert rc != 0, what
    with pytest.raises(_capi.RasterError):
        cx.check(rc)
    torch.cuda.synchronize()
    for buf in (features, depth, weights, samples):
        assert bool((buf == SENTINEL).all()), f"{what}: something was launched"


def test_null_pointers_are_refused(native_lib):
    name = T.CASES[0]
    c, cl, w, o, d, _ = _inputs(name)
    M, Nc, Ni = 5, 8, 4
    uc, uf = torch.zeros((M, Nc), device=DEV), torch.zeros((M, Ni), device=DEV)
    features, depth, weights, samples, _ = _buffers(M, Nc, Ni)
    for drop in ("o", "uc", "uf", "features", "depth", "weights"):
        a = dict(o=o[:M].contiguous(), uc=uc, uf=uf, features=features, depth=depth, weights=weights)
        a[drop] = None
        cx, rc = _direct(c, cl, w, a["o"], d[:M].contiguous(), a["uc"], a["uf"], M, Nc, Ni, a["features"], a["depth"], a["weights"],
                         samples)
        assert rc != 0, drop
    torch.cuda.synchronize()
    for buf in (features, depth, weights, samples):
        assert bool((buf == SENTINEL).all())
