"""The teacher renderer's per-ray kernels (csrc/ggd_teacher.hip) at the sample counts and ray counts where their code branches:
the case tables of tests/_teacher_render_cases.py (proven and measured on the CPU by tests/test_teacher_render_cases_host.py) on
the device.  One render per case with return_samples; the exact stages bit for bit, the importance and composite stages against
the float64 restatement of tests/_teacher_render_ref.py fed the GPU's own samples -- every ray, none left out -- at twice the
deviation the torch form on the CPU shows on the same table."""
import ctypes as C
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import _capi, density, teacher
import _teacher_render_cases as K
import _teacher_render_ref as T

DEV = torch.device("cuda:0")
SENTINEL = -7.25
STAGED = K.TABLE_N + K.TABLE_D + K.TABLE_M              # table C runs the same checks in its own test
GUARDED = [c for c in K.TABLE_N if c.nm in K.AROUND_THE_WAVE] + [c for c in K.TABLE_M if c.M == 1025 and c.placement == "front"]
WORKSPACE = [(K.BY_ID["M-4099-8+5-tail"], K.BY_ID["N-pano-33+33"]), (K.BY_ID["M-1025-48+48-front"], K.BY_ID["N-eg3d-64+2"])]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want):
    """a device tensor and a numpy float32 array agree bit for bit"""
    want = np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and np.array_equal(_np(got).view(np.int32), want.view(np.int32))


def _all_tensors(out):
    return [out.features, out.depth, out.weights] + list(out.samples)


@functools.lru_cache(maxsize=None)
def _device_inputs(cid):
    """the case's inputs on the device; table C makes its rays and draws its noise there"""
    case = K.BY_ID[cid]
    b = K.build(case)
    if case.table == "C":
        cams, intr = K.cameras()
        o, d = teacher.camera_rays(cams.to(DEV), intr.to(DEV), K.C_RESOLUTION)
        uc, uf = K.draw(case, case.M, torch.Generator(device=DEV).manual_seed(case.seed))
    else:
        o, d, uc, uf = b.origins.to(DEV), b.dirs.to(DEV), b.u_coarse.to(DEV), b.u_fine.to(DEV)
    return SimpleNamespace(b=b, planes_cl=b.planes_cl.to(DEV), weights=b.weights.to(DEV), origins=o, dirs=d, noise=(uc, uf))


def _call(case, **how):
    i = _device_inputs(case.id)
    return teacher.render_teacher(i.planes_cl, i.weights, i.origins, i.dirs, **dict(i.b.kwargs, **how))


@functools.lru_cache(maxsize=None)
def _render(cid):
    """one render of a case with every stage's values, shared by the tests (never modified)"""
    return _call(K.BY_ID[cid], noise=_device_inputs(cid).noise, return_samples=True)


# ---- the checks, shared with table C ---------------------------------------------------------------------------------------------
def _check_exact_stages(case, out):
    i = _device_inputs(case.id)
    b, s = i.b, out.samples
    o, d, uc = _np(i.origins), _np(i.dirs), _np(i.noise[0])
    table, delta = teacher.coarse_table(K.RAY_START, K.RAY_END, case.Nc)
    assert _same(s.depths_coarse, T.coarse_depths(table.numpy(), delta, uc))
    assert _same(s.coords_coarse, T.coordinates(o, d, _np(s.depths_coarse)))
    assert s.depths_fine.shape == (case.M, case.Ni) and s.rgb_fine.shape == (case.M, case.Ni, 32)
    if case.Ni:
        assert _same(s.coords_fine, T.coordinates(o, d, _np(s.depths_fine)))
    n_cropped = 0
    for coords, sigma, rgb in ((s.coords_coarse, s.sigma_coarse, s.rgb_coarse), (s.coords_fine, s.sigma_fine, s.rgb_fine)):
        if coords.numel() == 0:
            continue
        fs, frgb = density.sample_field(i.planes_cl, i.weights, coords, b.c.box_warp, b.c.axes, b.c.D or None, want_rgb=True)
        assert torch.equal(_bits(rgb.reshape(-1, 32)), _bits(frgb))
        outside = torch.zeros_like(sigma, dtype=torch.bool) if b.lim is None else \
            ~((coords[..., 0].abs() <= float(b.lim)) & (coords[..., 2].abs() <= float(b.lim)))
        want = torch.where(outside, torch.full_like(sigma, -1e3), fs.view_as(sigma))
        assert torch.equal(_bits(sigma), _bits(want))
        assert bool((sigma[outside] == -1e3).all())
        n_cropped += int(outside.sum())
    if case.miss:
        assert n_cropped >= len(case.miss) * (case.Nc + case.Ni)
    again = _call(case, noise=i.noise, return_samples=True)
    for a, g in zip(_all_tensors(out), _all_tensors(again)):
        assert torch.equal(_bits(a), _bits(g)), "two runs differ"


def _check_stages_against_float64(case, out):
    i = _device_inputs(case.id)
    dev, want = K.stage_deviations(out, i.noise[1], i.b.white_back)
    tol = K.TOL[case.table]
    for k in K.STAGES:
        print(f"\n  {case.id}: {k}, worst |gpu - float64| = {dev[k]:.3e}, tolerance {getattr(tol, k):.3e}, ratio "
              f"{dev[k] / getattr(tol, k):.3f} [table {case.table}]", end="")
    for k in K.STAGES:
        assert dev[k] <= getattr(tol, k), f"{case.id}: {k}"
    assert float(out.depth.min()) >= want.lo and float(out.depth.max()) <= want.hi
    return want


# ---- 1, 2: every case of N, D and M ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STAGED, ids=K.ids(STAGED))
def test_exact_stages(native_lib, case):
    """coarse depths and coordinates bit-equal to the fp32 restatement; sigma (where the crop leaves it) and rgb bit-equal to
    sample_field at the returned coordinates; cropped samples exactly -1e3; two runs bit-equal in every tensor"""
    _check_exact_stages(case, _render(case.id))


@pytest.mark.parametrize("case", STAGED, ids=K.ids(STAGED))
def test_importance_and_composite_against_float64(native_lib, case):
    """fine depths, features, weights and depth of every ray within twice the torch form's own deviation on the table; the depth
    inside the call's depth range"""
    _check_stages_against_float64(case, _render(case.id))


# ---- 3: the misses of table M ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.TABLE_M, ids=K.ids(K.TABLE_M))
def test_rays_that_miss_take_the_largest_depth_of_the_call(native_lib, case):
    """weight exactly 0, the white background, depth = the call's largest sample depth bit for bit -- wherever in the clamp
    kernel's stride loop the ray that holds it is reduced"""
    out = _render(case.id)
    s = out.samples
    rows = torch.tensor(case.miss, device=DEV)
    assert bool((s.sigma_coarse[rows] == -1e3).all()) and bool((s.sigma_fine[rows] == -1e3).all())
    assert bool((out.weights[rows] == 0).all())
    assert bool((out.features[rows] == 1.0).all())
    every = torch.cat([s.depths_coarse, s.depths_fine], 1)
    top, low = every.max(), every.min()
    assert int(every.max(1)[0].argmax()) == case.r_hi and int(every.min(1)[0].argmin()) == case.r_lo
    assert torch.equal(_bits(out.depth[rows]), _bits(top.expand(len(case.miss))))
    assert bool((out.depth[out.weights == 0] == top).all())
    live = out.weights > 0
    assert bool((out.depth[live] < top).all()) and bool((out.depth[live] > low).all())


# ---- 4: the workspace form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("large,small", WORKSPACE, ids=[f"{a.id} then {b.id}" for a, b in WORKSPACE])
def test_workspace_form_after_the_scratch_has_grown(native_lib, large, small):
    """samples == NULL puts the sample block and the rays' ranges into the context's scratch: bit-equal to the return_samples form
    at the large ray counts, and for a nine-ray call directly behind one, with the large call's values still in the scratch"""
    want = [_render(case.id) for case in (large, small)]
    got = [_call(case, noise=_device_inputs(case.id).noise) for case in (large, small)]      # back to back
    for case, g, w in zip((large, small), got, want):
        assert g.samples is None
        for k in ("features", "depth", "weights"):
            assert torch.equal(_bits(getattr(g, k)), _bits(getattr(w, k))), f"{case.id}: {k}"


# ---- 5: guards -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GUARDED, ids=K.ids(GUARDED))
def test_nothing_is_written_behind_the_outputs(native_lib, case):
    """ggd_teacher_render itself into over-allocated buffers: sentinel rows behind all four untouched, every output row written,
    the values those of the render above"""
    i = _device_inputs(case.id)
    b, w, cl = i.b, i.weights, i.planes_cl
    M, Nc, Ni = case.M, case.Nc, case.Ni
    offsets, shapes, total = teacher.sample_layout(M, Nc, Ni)
    mk = lambda *shape: torch.full(shape, SENTINEL, device=DEV)
    features, depth, weights, samples = mk(M + 8, 32), mk(M + 8), mk(M + 8), mk(total + 64)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    table, _ = teacher.coarse_table(K.RAY_START, K.RAY_END, Nc)
    lim = None if b.c.crop is None else float(b.c.box_warp) / 2 - float(b.c.crop)
    cx, stream = _capi.context_and_stream(DEV)
    with torch.cuda.device(DEV):
        cx.check(cx.lib.ggd_teacher_render(
            cx.handle, C.c_void_p(stream), *density._plane_args(cl, w, b.c.D, cl.shape[-3], cl.shape[-2], b.c.axes, b.c.box_warp),
            vp(i.origins), vp(i.dirs), M, K.RAY_START, K.RAY_END, vp(table), Nc, Ni, vp(i.noise[0]), vp(i.noise[1]) if Ni else None,
            int(lim is not None), 0.0 if lim is None else lim, int(b.white_back), vp(features), vp(depth), vp(weights), vp(samples)))
    for buf, used in ((features, M), (depth, M), (weights, M), (samples, total)):
        assert bool((buf[used:] == SENTINEL).all()), "rows behind an output were written"
        assert not bool((buf[:used] == SENTINEL).any()), "an output row was not written"
    want = _render(case.id)
    for got, ref in ((features[:M], want.features), (depth[:M], want.depth), (weights[:M], want.weights)):
        assert torch.equal(_bits(got), _bits(ref))
    for name, ref in zip(teacher.TeacherSamples._fields, want.samples):
        part = samples[offsets[name]:offsets[name] + int(np.prod(shapes[name]))]
        assert torch.equal(_bits(part), _bits(ref.reshape(-1))), name


# ---- 6: the public path ----------------------------------------------------------------------------------------------------------
def test_public_path_from_cameras_to_images(native_lib):
    """camera_rays on the device at R = 23, noise drawn with a generator, the stage checks on those rays, images() and geometry()"""
    case = K.TABLE_C[0]
    i, R = _device_inputs(case.id), K.C_RESOLUTION
    assert i.origins.shape == (case.M, 3) and i.origins.is_cuda
    cpu = K.build(case)
    # the same torch ops on the other device: unit vectors after a handful of fp32 roundings each
    assert float((i.dirs.cpu() - cpu.dirs).abs().max()) <= 1e-5 and torch.equal(i.origins.cpu(), cpu.origins)
    out = _render(case.id)
    _check_exact_stages(case, out)
    _check_stages_against_float64(case, out)
    gen = lambda seed: torch.Generator(device=DEV).manual_seed(seed)
    drawn = _call(case, generator=gen(case.seed))                     # the draws of _device_inputs, made by render_teacher itself
    twin = _call(case, generator=gen(case.seed))
    other = _call(case, generator=gen(case.seed + 1))
    for k in ("features", "depth", "weights"):
        assert torch.equal(_bits(getattr(drawn, k)), _bits(getattr(out, k))), k
        assert torch.equal(_bits(getattr(drawn, k)), _bits(getattr(twin, k))), k
    assert not torch.equal(drawn.depth, other.depth)
    feat, depth, mask = drawn.images(R)
    assert feat.shape == (2, 32, R, R) and depth.shape == (2, 1, R, R) and mask.shape == (2, 1, R, R)
    assert drawn.activation == "sigmoid"
    assert torch.equal(feat.permute(0, 2, 3, 1).reshape(-1, 32), drawn.features * 2 - 1)
    assert torch.equal(depth.reshape(-1), drawn.depth)
    assert torch.equal(mask.reshape(-1), drawn.weights * (1 + 2 * 0.001) - 0.001)
    assert torch.equal(feat[1, :, 22, 0], drawn.features[R * R + 22 * R] * 2 - 1)      # row-major pixels, second camera
    g_depth, g_weights = drawn.geometry(R)
    assert g_depth.shape == g_weights.shape == (2, 1, R, R)
    assert torch.equal(g_depth.reshape(-1), drawn.depth) and torch.equal(g_weights.reshape(-1), drawn.weights)
