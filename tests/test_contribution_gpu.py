"""Contribution statistics on the device (ggd_contribution, csrc/ggd_contribution.hip): bit-exact against the colour pass's own
weights (read back through one-hot feature channels), against the float64 reference of tests/_contrib_ref.py on every row,
conservation against the alpha map, accumulation and run-to-run identity, that nothing else of a frame moves, the C entry point's
refusals, and GaussianModel.prune_by_contribution end to end.  Each test prints its measured figures before it asserts."""
from __future__ import annotations

import ctypes as C
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _contrib_ref as CR
import _features_cases as FC
import _instance_cases as IC
from _util import decode_result, device_args, same_frame, scene_inputs
from test_instances_gpu import _options

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SCENES = ("P257-M9", "colors", "adversarial", "A1")
SHAPES = {"P257-M9": (17, 33), "colors": (64, 48), "adversarial": (96, 80), "A1": (104, 72)}
SCALE = np.float32(2.0 ** 24)
SENTINEL = 0x7ADBEEF012345678


def _fresh(P):
    return torch.zeros((P, 3), dtype=torch.int64, device=DEV)


def _native(d, raw=None, f=None, aux=False):
    from gaussian_gan_decoder_amd import rasterizer as R
    kw = {}
    if f is not None:
        kw["features"] = f.to(DEV)
    if raw is not None:
        kw["contribution"] = raw
    return R.rasterize_gaussians_native(*device_args(d), False, render_depth_alpha=aux, **kw)


def _decode(raw):
    """(sum float64, count int64, max float32) on the host, through ContributionStats' own decoding"""
    from gaussian_gan_decoder_amd.contribution import decode_pixel_count, decode_weight_max, decode_weight_sum
    r = raw.cpu()
    return decode_weight_sum(r).numpy(), decode_pixel_count(r).numpy(), decode_weight_max(r).numpy()


def _inputs(scene):
    d = IC.inputs(dict(scene=scene))
    assert (d["W"], d["H"]) == SHAPES[scene]
    return d


@functools.lru_cache(maxsize=None)
def _oracle_reference(scene):
    return CR.of_forward(IC.reference(dict(scene=scene, feature="aux"))["o"])


@functools.lru_cache(maxsize=None)
def _chosen(scene):
    """32 rows, from the oracle alone: every row with a fragile pair (up to 16), the largest counts, seeded random rows"""
    ref = _oracle_reference(scene)
    P = ref["count"].shape[0]
    rows = [int(i) for i in np.flatnonzero(ref["own_fragile"] > 0)[:16]]
    for i in np.argsort(-ref["count"], kind="stable"):
        if len(rows) >= 24:
            break
        if int(i) not in rows:
            rows.append(int(i))
    for i in np.random.RandomState(4100 + P).permutation(P):
        if len(rows) >= 32:
            break
        if int(i) not in rows:
            rows.append(int(i))
    return tuple(rows)


def _one_hot(P, rows):
    f = torch.zeros(P, 32)
    for c, g in enumerate(rows):
        f[g, c] = 1.0
    return f


def _assert_rows_equal_the_map(raw, rows, fmap, what):
    """channel c of a one-hot feature map is w of Gaussian rows[c] at every pixel (fma(1, w, 0), background 0): equality"""
    F = fmap.cpu().numpy()[:len(rows)]
    assert F.dtype == np.float32
    got = raw.cpu().numpy()[list(rows)]
    q = np.rint(F * SCALE).astype(np.int64).reshape(len(rows), -1).sum(1)
    cnt = (F > 0).reshape(len(rows), -1).sum(1)
    mx = F.reshape(len(rows), -1).max(1).view(np.uint32).astype(np.int64)
    print(f"[contribution] {what}: {len(rows)} rows, counts {int(cnt.min())} .. {int(cnt.max())}, "
          f"mismatches sum {int((got[:, 0] != q).sum())} count {int((got[:, 1] != cnt).sum())} max {int((got[:, 2] != mx).sum())}")
    assert np.array_equal(got[:, 0], q), what
    assert np.array_equal(got[:, 1], cnt), what
    assert np.array_equal(got[:, 2], mx), what
    return int(cnt.sum())


# ---- 1. bit-exact against the colour pass's own weights, every pixel
@pytest.mark.parametrize("scene", SCENES)
def test_rows_equal_the_colour_weights(native_lib, scene):
    d, rows = _inputs(scene), _chosen(scene)
    raw = _fresh(d["P"])
    res = _native(d, raw, _one_hot(d["P"], rows))
    assert _assert_rows_equal_the_map(raw, rows, res[-1], scene) > 0


MODES = [(em, cull) for em in (0, 1, 2, 3) for cull in (0, 1)]


@pytest.mark.parametrize("em,cull", MODES, ids=[f"exp{em}-cull{cull}" for em, cull in MODES])
def test_every_instance_equals_the_colour_weights(native_lib, em, cull):
    d, rows = _inputs("A1"), _chosen("A1")
    raw = _fresh(d["P"])
    with _options(dict(IC.DEFAULTS, exp_mode=em, cull=cull)):
        res = _native(d, raw, _one_hot(d["P"], rows))
    assert _assert_rows_equal_the_map(raw, rows, res[-1], f"A1 exp{em} cull{cull}") > 0


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("layout", list(FC.LAYOUTS))
def test_round_shapes_equal_the_colour_weights(native_lib, layout, cull):
    """one 16 x 16 tile, rounds of 0 / 1 / 63 / 64 survivors: ALL splats, one-hot columns in successive calls"""
    d = FC.layout_inputs(layout)
    P = d["P"]
    raw = _fresh(P)
    with _options(dict(IC.DEFAULTS, cull=cull)):
        first = _native(d, raw)
        blended = 0
        for r0 in range(0, P, 32):
            rows = tuple(range(r0, min(r0 + 32, P)))
            res = _native(d, None, _one_hot(P, rows))
            assert same_frame(first, res)
            blended += _assert_rows_equal_the_map(raw, rows, res[-1], f"{layout} cull{cull} rows {r0}..")
    dead = FC.layout_kinds(layout) == "dead"
    assert not raw.cpu().numpy()[dead].any() and blended == int(raw[:, 1].sum())


# ---- 2. against the float64 reference, all rows
@pytest.mark.parametrize("scene", SCENES)
def test_all_rows_against_float64(native_lib, scene):
    d = _inputs(scene)
    raw = _fresh(d["P"])
    ref = CR.of_forward(decode_result(d, _native(d, raw)))
    s, cnt, mx = _decode(raw)
    frag = ref["own_fragile"]
    rows = int((frag > 0).sum())
    dc = np.abs(cnt - ref["count"])
    es, em = np.abs(s - ref["sum"]), np.abs(mx.astype(np.float64) - ref["max"])
    ts, tm = CR.sum_tolerance(ref), CR.max_tolerance(ref)
    print(f"[contribution] {scene}: {rows} fragile rows (cap {CR.fragile_cap(d['P'])}); count differs on {int((dc > 0).sum())} rows; "
          f"worst |dsum| / bound {float((es / np.maximum(ts, 1e-300)).max()):.3f} (|dsum| <= {es.max():.2e}), "
          f"worst |dmax| / bound {float((em / tm).max()):.3f} (|dmax| <= {em.max():.2e})")
    assert rows <= CR.fragile_cap(d["P"])
    assert (dc[frag == 0] == 0).all() and (dc <= frag).all()
    assert (es <= ts).all()
    assert (em <= tm).all()


# ---- 3. conservation
@pytest.mark.parametrize("scene", SCENES)
def test_weights_sum_to_the_alpha_map(native_lib, scene):
    d = _inputs(scene)
    raw = _fresh(d["P"])
    res = _native(d, raw, aux=True)
    s, cnt, _ = _decode(raw)
    alpha = float(res[7].double().sum())
    bound = 1e-5 * d["W"] * d["H"] + 2.0 ** -25 * float(cnt.sum())
    print(f"[contribution] {scene}: sum of weight sums {s.sum():.6f}, sum of the alpha map {alpha:.6f}, |d| = "
          f"{abs(s.sum() - alpha):.2e} of {bound:.2e}")
    assert abs(float(s.sum()) - alpha) <= bound


# ---- 4. accumulation and reproducibility
def _second_camera(d):
    other = scene_inputs(P=3000, size=104, width=104, height=72, kind="shell", lsm=-4.6, seed=61, h=1.2, v=1.8)
    assert torch.equal(other["means3D"], d["means3D"]) and not torch.equal(other["viewmatrix"], d["viewmatrix"])
    return dict(d, **{k: other[k] for k in ("viewmatrix", "projmatrix", "campos", "tanfovx", "tanfovy")})


def test_accumulation_and_run_to_run_identity(native_lib):
    d = _inputs("A1")
    d2 = _second_camera(d)
    P = d["P"]
    a, b, twice, other, both = (_fresh(P) for _ in range(5))
    res = _native(d, a)
    _native(d, b)
    assert torch.equal(a, b) and bool(a.any())
    _native(d, twice); _native(d, twice)
    assert torch.equal(twice[:, :2], 2 * a[:, :2]) and torch.equal(twice[:, 2], a[:, 2])
    _native(d2, other)
    _native(d, both); _native(d2, both)
    assert not torch.equal(other, a)
    assert torch.equal(both[:, :2], a[:, :2] + other[:, :2]) and torch.equal(both[:, 2], torch.maximum(a[:, 2], other[:, 2]))
    culled = res[2] == 0
    assert bool(culled.any()) and not bool(a[culled].any())
    # rows of Gaussians that contribute nowhere are never written
    unused = a[:, 1] == 0
    assert bool(unused[culled].all()) and bool(unused.any())
    marked = _fresh(P)
    marked[unused] = SENTINEL
    _native(d, marked)
    assert bool((marked[unused] == SENTINEL).all()) and torch.equal(marked[~unused], a[~unused])
    print(f"[contribution] A1: {int((~unused).sum())} of {P} rows used, {int(culled.sum())} culled, "
          f"{int((unused & ~culled).sum())} visible but blended nowhere")


# ---- 5. nothing else moves
@pytest.mark.parametrize("scene", ["colors", "A1"])
def test_the_frame_is_unchanged(native_lib, scene):
    d = _inputs(scene)
    f = FC.features(d["P"], 5)[0]
    for kw in (dict(), dict(aux=True), dict(f=f), dict(f=f, aux=True)):
        plain, with_kw = _native(d, None, **kw), _native(d, _fresh(d["P"]), **kw)
        assert len(plain) == len(with_kw) and same_frame(plain, with_kw)
        na, nb = decode_result(d, plain), decode_result(d, with_kw)
        vis = plain[2].cpu().numpy() > 0
        # the records a backward reads (the clamp flags are written for SH colours only: left out)
        for k in ("xy", "conic_opacity", "rgb", "power_threshold", "cull_extent", "depths"):
            assert np.array_equal(na[k][vis].view(np.uint8), nb[k][vis].view(np.uint8)), k
        for x, y in zip(plain[6:], with_kw[6:]):
            assert torch.equal(x, y)


def test_backward_after_a_keyword_render_is_bit_equal(native_lib):
    """A colours-precomp scene whose backward has ONE summation order: the `flush-edges` layout, where every splat's footprint
    lies inside one 8 x 8 quarter, so each accumulator record receives one atomic add per slot and the gradients of two runs are
    comparable bit for bit (on a general scene the backward's float atomics reorder from run to run, keyword or not; there the
    test above holds every buffer the backward reads to equality)."""
    from gaussian_gan_decoder_amd import rasterizer as R
    base = FC.layout_inputs("flush-edges")
    gen = torch.Generator().manual_seed(12)
    d = dict(base, shs=None, colors_precomp=torch.rand(base["P"], 3, generator=gen))
    g = torch.randn(3, d["H"], d["W"], generator=gen).to(DEV)
    t = lambda x: torch.empty(0, device=DEV) if x is None else x.to(DEV)

    def backward(res):
        return R.rasterize_gaussians_backward_native(
            t(d["bg"]), t(d["means3D"]), res[2], t(d["colors_precomp"]), t(d["scales"]), t(d["rotations"]), d["scale_modifier"],
            t(d["cov3D_precomp"]), t(d["viewmatrix"]), t(d["projmatrix"]), d["tanfovx"], d["tanfovy"], g, t(d["shs"]),
            d["sh_degree"], t(d["campos"]), res[3], res[0], res[4], res[5], False)
    raw = _fresh(d["P"])
    plain, with_kw = _native(d), _native(d, raw)
    assert same_frame(plain, with_kw) and bool(raw.any())
    ga, gb = backward(plain), backward(with_kw)
    assert len(ga) == len(gb) == 8
    for name, x, y in zip(("means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rots"), ga, gb):
        assert torch.equal(x, y), name
    assert bool(ga[1].any()) and bool(ga[3].any())


# ---- 6. the C entry point's refusals
def test_c_abi_refusals(native_lib):
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd import rasterizer as R
    d = _inputs("P257-M9")
    P = d["P"]
    want = _fresh(P)
    res = _native(d, want)
    num, geom, binning, img = res[0], res[3], res[4], res[5]
    assert num > 0
    cx, stream = _capi.context_and_stream(DEV)
    lib, h, st = cx.lib, cx.handle, C.c_void_p(stream)
    args = device_args(d)
    rs = R.GaussianRasterizationSettings(d["H"], d["W"], d["tanfovx"], d["tanfovy"], args[0], d["scale_modifier"], args[8], args[9],
                                         d["sh_degree"], args[16], False, False)
    keep = []
    prm = R._params(rs, P, int(d["shs"].shape[1]), DEV, keep)
    prm0 = R._params(rs, 0, 0, DEV, keep)
    raw = torch.full((P + 1, 3), SENTINEL, dtype=torch.int64, device=DEV)
    vp = lambda x, off=0: C.c_void_p(x.data_ptr() + off)

    def call(p=prm, g=vp(geom), b=vp(binning), i=vp(img), r=num, s=vp(raw)):
        return lib.ggd_contribution(h, st, C.byref(p), g, b, i, r, s)
    with torch.cuda.device(DEV):
        bad = {"stats NULL": call(s=None), "stats misaligned": call(s=vp(raw, 4)), "img NULL": call(i=None),
               "geom NULL": call(g=None), "binning NULL": call(b=None), "num_rendered < 0": call(r=-1)}
        assert {k: v for k, v in bad.items() if v != -1} == {}
        assert call(s=vp(raw, 4)) == -1 and b"8-byte aligned" in lib.ggd_last_error(h)
        assert call(s=None) == -1 and b"stats is NULL" in lib.ggd_last_error(h)
        # nothing to add is legal, and changes nothing
        assert call(p=prm0, s=None) == 0 and call(p=prm0) == 0
        assert call(r=0, g=None, b=None) == 0 and call(r=0) == 0
        torch.cuda.synchronize()
        assert bool((raw == SENTINEL).all())                  # nothing was launched
        raw.zero_()
        assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(raw[:P], want) and not bool(raw[P].any())


# ---- 7. end to end: render, accumulate, prune
ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
WALL, HIDDEN, FRONT = 576, 424, 1000
SIZE = 64
VIEWS = ((math.pi / 2, math.pi / 2), (math.pi / 2 - 0.25, math.pi / 2 + 0.1), (math.pi / 2 + 0.25, math.pi / 2 - 0.1))


def _walled_model():
    """2 000 rows: an opaque wall through the origin that faces the cameras (a 24 x 24 grid, spacing 0.052, sigma 0.074: the
    transmittance behind it is under the 1e-4 stop everywhere), 424 rows behind it, 1 000 in front of it with opacities around
    sigmoid(-3), so that a share of the visible rows stays under the 0.01 threshold as well"""
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel
    from gaussian_gan_decoder_amd.synthetic import make_camera
    cams = [make_camera(SIZE, 12.0, hh, vv, device=DEV) for hh, vv in VIEWS]
    n = cams[0].camera_center.detach().cpu().double()
    n = n / n.norm()
    a = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64) if abs(float(n[1])) < 0.9 else torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)
    u = torch.linalg.cross(n, a); u = u / u.norm()
    v = torch.linalg.cross(n, u)
    gen = torch.Generator().manual_seed(77)
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    grid = (torch.arange(24, dtype=torch.float64) - 11.5) * 0.052
    wall = (grid[:, None, None] * u + grid[None, :, None] * v).reshape(-1, 3)
    hidden = -(0.15 + 0.3 * rnd(HIDDEN, 1)) * n + (rnd(HIDDEN, 1) - 0.5) * 0.5 * u + (rnd(HIDDEN, 1) - 0.5) * 0.5 * v
    front = (0.1 + 0.4 * rnd(FRONT, 1)) * n + (rnd(FRONT, 1) - 0.5) * 0.6 * u + (rnd(FRONT, 1) - 0.5) * 0.6 * v
    P = WALL + HIDDEN + FRONT
    xyz = torch.cat([wall, hidden, front]).float()
    scaling = torch.cat([torch.full((WALL, 3), -2.6), -4.5 + 0.4 * torch.randn(HIDDEN + FRONT, 3, generator=gen)])
    opacity = torch.cat([torch.full((WALL, 1), 6.0), 2.0 * torch.randn(HIDDEN, 1, generator=gen),
                         -3.0 + 2.0 * torch.randn(FRONT, 1, generator=gen)])
    rotation = torch.randn(P, 4, generator=gen)
    pc = GaussianModel(0)
    values = dict(_xyz=xyz, _features_dc=torch.randn(P, 1, 3, generator=gen), _features_rest=torch.zeros(P, 0, 3), _opacity=opacity,
                  _scaling=scaling, _rotation=rotation)
    for attr in ATTRS:
        setattr(pc, attr, torch.nn.Parameter(values[attr].contiguous().to(DEV)))
    pc.spatial_lr_scale = 1.0
    pc.training_setup(SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016,
                                      position_lr_delay_mult=0.01, position_lr_max_steps=30_000, feature_lr=0.0025,
                                      opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001))
    for attr in ATTRS:
        getattr(pc, attr).grad = torch.zeros_like(getattr(pc, attr))
    pc.optimizer.step()                                       # zero gradients: the parameters stay, the moments exist
    pc.optimizer.zero_grad(set_to_none=True)
    for attr in ATTRS:
        state = pc.optimizer.state[getattr(pc, attr)]
        state["exp_avg"] = torch.randn(getattr(pc, attr).shape, generator=gen).to(DEV)
        state["exp_avg_sq"] = torch.rand(getattr(pc, attr).shape, generator=gen).to(DEV)
    pc.max_radii2D = torch.arange(P, dtype=torch.float32, device=DEV)      # (a tag: which rows survive)
    pc.xyz_gradient_accum = torch.rand(P, 1, generator=gen).to(DEV)
    pc.denom = torch.rand(P, 1, generator=gen).to(DEV)
    return pc, cams


def _frame_inputs(pc, cam, bg):
    """what render_simple hands the rasterizer for this camera, in the form of _util.scene_inputs"""
    with torch.no_grad():
        return dict(P=pc.get_xyz.shape[0], W=SIZE, H=SIZE, sh_degree=0, scale_modifier=1.0, tanfovx=math.tan(cam.FoVx * 0.5),
                    tanfovy=math.tan(cam.FoVy * 0.5), means3D=pc.get_xyz.detach(), opacities=pc.get_opacity.detach(),
                    viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center, bg=bg,
                    shs=pc.get_features.detach(), colors_precomp=None, scales=pc.get_scaling.detach(),
                    rotations=pc.get_rotation.detach(), cov3D_precomp=None)


def test_prune_by_contribution_end_to_end(native_lib):
    from gaussian_gan_decoder_amd.contribution import ContributionStats
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    pc, cams = _walled_model()
    P = WALL + HIDDEN + FRONT
    bg = torch.zeros(3, device=DEV)
    stats = ContributionStats(P, DEV)
    ref_max, tol = np.zeros(P), np.zeros(P)
    with torch.no_grad():
        for k, cam in enumerate(cams):
            out = render_simple(cam, pc, bg, contribution=stats)
            assert out["contribution"] is stats and stats.frames == k + 1
            d = _frame_inputs(pc, cam, bg)
            res = _native(d)
            assert torch.equal(res[1], out["render"])
            ref = CR.of_forward(decode_result(d, res))
            ref_max, tol = np.maximum(ref_max, ref["max"]), np.maximum(tol, CR.max_tolerance(ref))
    got_max = stats.weight_max.cpu().numpy().astype(np.float64)
    assert (np.abs(got_max - ref_max) <= tol).all()
    before = {}
    for attr in ATTRS:
        p = getattr(pc, attr)
        before[attr] = (p.detach().clone(), pc.optimizer.state[p]["exp_avg"].clone(), pc.optimizer.state[p]["exp_avg_sq"].clone())
    accum, denom = pc.xyz_gradient_accum.clone(), pc.denom.clone()

    kept = pc.prune_by_contribution(stats, min_max_weight=0.01)
    survivors = pc.max_radii2D.long()
    assert kept == survivors.numel() == pc.get_xyz.shape[0]
    dropped = np.ones(P, bool)
    dropped[survivors.cpu().numpy()] = False
    sure = np.abs(ref_max - 0.01) > tol
    hidden = np.arange(P) >= WALL
    hidden &= np.arange(P) < WALL + HIDDEN
    front = np.arange(P) >= WALL + HIDDEN
    print(f"[contribution] end to end: kept {kept} of {P}; dropped {int(dropped[hidden].sum())} of {HIDDEN} hidden and "
          f"{int(dropped[front].sum())} of {FRONT} front rows; {int((~sure).sum())} rows within their tolerance of the threshold")
    assert np.array_equal(dropped[sure], (ref_max < 0.01)[sure])
    assert dropped[hidden].all() and 0 < int(dropped[front].sum()) < FRONT and int((~sure).sum()) <= P // 50
    for attr in ATTRS:
        p = getattr(pc, attr)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad
        state = pc.optimizer.state[p]
        assert torch.equal(p.detach(), before[attr][0][survivors]), attr
        assert torch.equal(state["exp_avg"], before[attr][1][survivors]) and torch.equal(state["exp_avg_sq"], before[attr][2][survivors]), attr
    assert torch.equal(pc.xyz_gradient_accum, accum[survivors]) and torch.equal(pc.denom, denom[survivors])


def test_render_keyword_with_and_without_gradients(native_lib):
    """`contribution=True` makes a fresh object; the statistics of a frame are the same bits under no_grad, with gradients, with
    absgrad and with the other maps, and the backward runs as it does without the keyword"""
    from gaussian_gan_decoder_amd.contribution import ContributionStats
    from gaussian_gan_decoder_amd.gaussian_renderer import render, render_simple
    from gaussian_gan_decoder_amd.synthetic import make_scene
    sc = make_scene(1500, 48, "shell", seed=9, log_scale_mean=-4.5).to(DEV)
    pipe = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    with torch.no_grad():
        out = render_simple(sc.cam, sc.gaussian_model(), sc.bg, contribution=True)
        plain = render_simple(sc.cam, sc.gaussian_model(), sc.bg)
    st = out["contribution"]
    assert isinstance(st, ContributionStats) and st.frames == 1 and st.P == 1500 and bool(st.raw.any())
    assert "contribution" not in plain and torch.equal(plain["render"], out["render"]) and set(out) == set(plain) | {"contribution"}
    for kw in (dict(absgrad=True), dict(render_depth_alpha=True, render_distortion=True), dict(render_normals=True, antialiasing=False)):
        pc = sc.gaussian_model(requires_grad=True)
        got = render_simple(sc.cam, pc, sc.bg, contribution=True, **kw)
        assert torch.equal(got["contribution"].raw, st.raw), kw
        got["render"].sum().backward()
        ref_pc = sc.gaussian_model(requires_grad=True)
        render_simple(sc.cam, ref_pc, sc.bg, **kw)["render"].sum().backward()
        assert pc._xyz.grad is not None and bool(torch.isfinite(pc._xyz.grad).all())
        scale = float(ref_pc._xyz.grad.abs().max())
        assert float((pc._xyz.grad - ref_pc._xyz.grad).abs().max()) <= 1e-5 * max(scale, 1.0)   # float atomics: two runs
    acc = ContributionStats(1500, DEV)
    with torch.no_grad():
        for _ in range(2):
            assert render(sc.cam, sc.gaussian_model(), pipe, sc.bg, contribution=acc)["contribution"] is acc
    assert acc.frames == 2 and torch.equal(acc.raw[:, :2], 2 * st.raw[:, :2]) and torch.equal(acc.raw[:, 2], st.raw[:, 2])
    with pytest.raises(ValueError, match="dimensions"):
        render_simple(sc.cam, sc.gaussian_model(), sc.bg, contribution=ContributionStats(7, DEV))
    with pytest.raises(ValueError, match="expected cuda"):
        render_simple(sc.cam, sc.gaussian_model(), sc.bg, contribution=ContributionStats(1500, "cpu"))
