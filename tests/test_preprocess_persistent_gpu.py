"""The per-Gaussian forward kernel as a persistent grid (GGD_OPT_PREPROCESS_WGS): a workgroup strides over
several 256-Gaussian tiles, stores what is keyed by the tile per tile and flushes its sums (the depth sort's histograms, the row
totals and instances, the outside-window count) once.

The reference is the CPU oracle: radii, tiles_touched, point_offsets, depths, xy, conic_opacity and rgb of the visible Gaussians,
the sorted list and the ranges bit for bit, the blend within assert_blend_matches' tolerance outside its fragile-pixel mask; the
native frames of one scene must be identical among themselves in every decoded array, whatever the grid.  A forced grid on a
small input puts many tiles on one workgroup: one workgroup taking every tile, uneven tile counts per workgroup, a ragged last
tile on the last and on a non-last workgroup, and one tile per workgroup."""
import numpy as np
import pytest
import torch

import _antialias_ref as AA
from _util import assert_blend_matches, decode_result, device_args, run_oracle, same_frame, scene_inputs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES = (1, 255, 256, 257, 1000, 2049)
_cache = {}


def _scene(P):
    """inputs and oracle frame of the cube scene with P Gaussians at 128^2, computed once"""
    if P not in _cache:
        d = scene_inputs(P=P, size=128, kind="cube", seed=40 + P % 7)
        _cache[P] = (d, run_oracle(d))
    return _cache[P]


def _ctx():
    from gaussian_gan_decoder_amd import _capi
    ctx = _capi.context_and_stream(DEV)[0]
    ctx.set_option(_capi.OPT_BINNING, 1)
    return ctx


def _assert_oracle(d, o, res, what, opacity_exact=True):
    n = decode_result(d, res)
    vis = o["radii"] > 0
    assert n["num_rendered"] == o["num_rendered"], what
    np.testing.assert_array_equal(n["radii"].cpu().numpy(), o["radii"], err_msg=what)
    np.testing.assert_array_equal(n["tiles_touched"], o["tiles_touched"], err_msg=what)
    np.testing.assert_array_equal(n["point_offsets"], o["point_offsets"], err_msg=what)
    for name in ("depths", "xy", "rgb"):
        np.testing.assert_array_equal(n[name][vis], o[name][vis], err_msg=f"{what}: {name}")
    k = 4 if opacity_exact else 3
    np.testing.assert_array_equal(n["conic_opacity"][vis, :k], o["conic_opacity"][vis, :k], err_msg=f"{what}: conic_opacity")
    np.testing.assert_array_equal(n["point_list"], o["point_list"], err_msg=what)
    np.testing.assert_array_equal(n["ranges"], o["ranges"], err_msg=what)
    assert_blend_matches(n, o, what=what)
    return n


def _frames(d, grid, fold, count, **kw):
    """`count` consecutive frames of one resident scene with `grid` preprocess workgroups; the first may take the two-call form,
    the later ones the single-call path (the next frame's control-block clear and the speculation state are in use)"""
    from gaussian_gan_decoder_amd import _capi, rasterizer as R
    ctx = _ctx()
    args = device_args(d, DEV)
    try:
        ctx.set_option(_capi.OPT_FOLD, fold)
        ctx.set_option(_capi.OPT_PREPROCESS_WGS, grid)
        assert ctx.get_option(_capi.OPT_PREPROCESS_WGS) == grid
        return [R.rasterize_gaussians_native(*args, **kw) for _ in range(count)]
    finally:
        ctx.set_option(_capi.OPT_PREPROCESS_WGS, 0)
        ctx.set_option(_capi.OPT_FOLD, 1)


@pytest.mark.parametrize("grid", [1, 2, 3, "tiles"])
@pytest.mark.parametrize("P", SIZES)
def test_forced_grids(native_lib, P, grid):
    d, o = _scene(P)
    g = (P + 255) // 256 if grid == "tiles" else grid
    folded = _frames(d, g, 1, 3)
    for i, res in enumerate(folded):
        _assert_oracle(d, o, res, f"P = {P}, {g} workgroups, frame {i}")
        assert same_frame(res, folded[0]), f"P = {P}, {g} workgroups: frame {i} differs from the first"
    unfolded = _frames(d, g, 0, 2)
    for i, res in enumerate(unfolded):
        _assert_oracle(d, o, res, f"P = {P}, {g} workgroups, separate histogram launch, frame {i}")
        assert same_frame(res, folded[0]), f"P = {P}, {g} workgroups: the unfolded frame {i} differs"


def _aa_oracle(d, n):
    """the oracle's forward with every opacity replaced by o_eff = o h (tests/test_antialiasing_gpu.py): the helper's value, the
    GPU record's where h is ill-conditioned"""
    oe = AA.o_eff(d)
    _, cond = AA.h_and_conditioning(d)
    vis = n["radii"].cpu().numpy() > 0
    op = np.where(vis & (cond > 1e3), n["conic_opacity"][:, 3], oe).astype(np.float32)
    return run_oracle(dict(d, opacities=torch.from_numpy(op).reshape(d["opacities"].shape).contiguous()))


INSTANCES = {
    "sh3": dict(sh_degree=3),
    "colors_precomp": dict(use_colors=True),
    "cov3D_precomp": dict(use_cov=True),
    "antialiasing": dict(),
}


@pytest.mark.parametrize("name", list(INSTANCES))
def test_instances(native_lib, name):
    """SHVEC, the colour and covariance inputs that replace an array by the view matrix in the request, and AA: 4 tiles on 3
    workgroups against one tile per workgroup and the oracle"""
    d = scene_inputs(P=1000, size=128, kind="cube", seed=50, **INSTANCES[name])
    kw = dict(antialiasing=True) if name == "antialiasing" else {}
    ref = _frames(d, 4, 1, 2, **kw)
    o = _aa_oracle(d, decode_result(d, ref[0])) if kw else run_oracle(d)
    for i, res in enumerate(_frames(d, 3, 1, 3, **kw) + _frames(d, 3, 0, 1, **kw)):
        _assert_oracle(d, o, res, f"{name}: 3 workgroups, frame {i}", opacity_exact=not kw)
        assert same_frame(res, ref[1]), f"{name}: frame {i} on 3 workgroups differs from one tile per workgroup"


def test_automatic_grid_with_more_tiles_than_workgroups(native_lib):
    """700 001 Gaussians are 2735 tiles, more than the automatic grid on any device: frames repeat until the two-launch sort has
    run, which reads the accumulated histogram and the key range -- a wrong one shows as a re-run or as a different list"""
    from gaussian_gan_decoder_amd import _capi, rasterizer as R
    d = scene_inputs(P=700_001, size=256, kind="shell", seed=61)
    o = run_oracle(d)
    ctx = _ctx()
    assert ctx.get_option(_capi.OPT_PREPROCESS_WGS) == 0 and ctx.get_option(_capi.OPT_FOLD) == 1
    ctx.set_option(_capi.OPT_MSD_SORT, 1)      # same value: restarts the speculation state
    args = device_args(d, DEV)
    first = R.rasterize_gaussians_native(*args)
    _assert_oracle(d, o, first, "first frame")
    m0, r0, c0 = ctx.get_option(_capi.STAT_MSD_FRAMES), ctx.get_option(_capi.STAT_SORT_RERUNS), ctx.capacity_retries
    last = first
    for i in range(100):
        last = R.rasterize_gaussians_native(*args)
        assert same_frame(last, first), f"frame {i + 1} differs from the first"
        if ctx.get_option(_capi.STAT_MSD_FRAMES) >= m0 + 2:
            break
    assert ctx.get_option(_capi.STAT_MSD_FRAMES) >= m0 + 2, "the two-launch sort never ran"
    assert ctx.get_option(_capi.STAT_SORT_RERUNS) == r0 and ctx.capacity_retries == c0
    _assert_oracle(d, o, last, "a two-launch-sort frame")


def test_two_scenes_in_alternation(native_lib):
    """two scenes of one shape on one context, 2 workgroups for 4 tiles: each frame clears the control block the other scene's
    next frame accumulates into"""
    from gaussian_gan_decoder_amd import _capi, rasterizer as R
    scenes = [scene_inputs(P=1000, size=128, kind="cube", seed=70 + k) for k in range(2)]
    oracles = [run_oracle(d) for d in scenes]
    args = [device_args(d, DEV) for d in scenes]
    ctx = _ctx()
    try:
        ctx.set_option(_capi.OPT_PREPROCESS_WGS, 2)
        firsts = []
        for i in range(6):
            res = R.rasterize_gaussians_native(*args[i % 2])
            _assert_oracle(scenes[i % 2], oracles[i % 2], res, f"frame {i}")
            if i < 2:
                firsts.append(res)
            assert same_frame(res, firsts[i % 2]), f"frame {i} differs from the scene's first"
    finally:
        ctx.set_option(_capi.OPT_PREPROCESS_WGS, 0)
