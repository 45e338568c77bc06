"""The density-field kernel (csrc/ggd_density.hip: ggd_density_points / ggd_density_grid / ggd_density_lattice) on the device,
element by element against the float64 restatement of tests/_density_ref.py:  |gpu - ref64| <= 1e-7 + KAPPA * 2^-24 * budget, no
array-scale term.  The case table, the budgets and where KAPPA comes from: tests/_density_ref.py; tests/test_density_host.py
measures KAPPA on the host and checks that the cases hit the edges they are named for.

Planes are 12 x 10 (an H / W swap shows).  Groups: forms (every depth / axes / activation / lr multiplier, sigma-only, run to run,
the zero-feature rows), the reference's own values, sizes on the wave and workgroup edges with sentinel rows, the softplus
range, the lattice, the grid against points, the chain to the surface sampler, refusals."""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import _capi, density
from gaussian_gan_decoder_amd.decoder import planes_channels_last
from gaussian_gan_decoder_amd.target_sampler import sample_surface_points, sample_target_points
import _density_ref as R

DEV = torch.device("cuda:0")
AXES = {"eg3d": 0, "panohead": 1}
_ids = dict(ids=lambda c: c.name)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _cx():
    return _capi.context_for(DEV), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


@functools.lru_cache(maxsize=None)
def _inputs(c):
    """(channel-last planes, weights, pool of positions) of a case on the device"""
    b = R.build(c)
    return planes_channels_last(b.planes, c.D or None).to(DEV), density.osg_weights(b.decoder).to(DEV), b.pos.to(DEV)


def _field(c, pos, want_rgb=True):
    cl, w, _ = _inputs(c)
    return density.sample_field(cl, w, pos, c.box_warp, c.axes, c.D or None, want_rgb=want_rgb)


def _points_direct(c, N, sigma, rgb, C_=32, act=None):
    """ggd_density_points on the first N rows of the case's pool, into the caller's (over-allocated) outputs"""
    cl, w, pos = _inputs(c)
    cx, stream = _cx()
    with torch.cuda.device(DEV):
        return cx.lib.ggd_density_points(cx.handle, stream, _vp(cl), C_, c.D, R.H, R.W, AXES[c.axes], c.box_warp, _vp(w.w1), _vp(w.b1),
                                         _vp(w.w2), _vp(w.b2), density.ACTIVATIONS[c.act] if act is None else act, _vp(pos), N,
                                         _vp(sigma), _vp(rgb))


def _zero_feature(c):
    """what the kernel gives a point without any tap: W2 softplus(b1) + b2 as IT computes it (a point far outside the box)"""
    far = torch.full((1, 3), 5.0 * c.box_warp, device=DEV)
    sigma, rgb = _field(c, far)
    return sigma[0], rgb[0]


# ---- forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.FORM_CASES, **_ids)
def test_every_form_matches_float64(native_lib, c):
    """D = 0 (EG3D axes), D = 1 and 3 with both axes x the three activations, lr multiplier 1 and 2, over the whole pool (edge
    rows, +-1e30, +-inf, NaN included): sigma and rgb within budget; the sigma of a sigma-only call and of a second run
    bit-equal; rows without any tap (budget 0 on every feature) equal the zero-feature result bit for bit."""
    _, _, pos = _inputs(c)
    ref = R.reference_of(c)
    sigma, rgb = _field(c, pos)
    assert sigma.shape == (R.POOL,) and rgb.shape == (R.POOL, 32)
    R.assert_within(sigma, ref.sigma, ref.sbud, c.name + " sigma")
    R.assert_within(rgb, ref.rgb, ref.rbud, c.name + " rgb")
    only = _field(c, pos, want_rgb=False)
    assert torch.equal(_bits(only), _bits(sigma)), "sigma-only differs from the sigma of the sigma + rgb call"
    again_s, again_rgb = _field(c, pos)
    assert torch.equal(_bits(again_s), _bits(sigma)) and torch.equal(_bits(again_rgb), _bits(rgb)), "two runs differ"
    free = (ref.fbud == 0).all(1).to(DEV)
    nan_rows = torch.isnan(pos).all(1)
    assert bool(free.any()) and bool((nan_rows & free).any())       # an all-NaN row has no tap on any plane
    s0, rgb0 = _zero_feature(c)
    assert torch.equal(_bits(sigma[free]), _bits(s0.expand(int(free.sum()))))
    assert torch.equal(_bits(rgb[free]), _bits(rgb0.expand(int(free.sum()), 32)))


@pytest.mark.parametrize("name", R.FIX_CASES)
def test_kernel_reproduces_the_reference_values(native_lib, name):
    """the reference's own run_model outputs (PanoHead D = 1 / 3, three activations, lr multiplier 1 / 2; EG3D) within the
    budget of the float64 restatement of the same inputs"""
    f = R.fixture_case(name)
    w = density.osg_weights(f.decoder)
    ref = R.reference(f.planes, f.coords, f.box_warp, f.axes, f.D, w.w1, w.b1, w.w2, w.b2, f.act)
    sigma, rgb = density.sample_field(planes_channels_last(f.planes, f.D or None).to(DEV), w.to(DEV), f.coords.to(DEV), f.box_warp,
                                      f.axes, f.D or None, want_rgb=True)
    R.assert_within(sigma, ref.sigma, ref.sbud, name + " sigma")
    R.assert_within(rgb, ref.rgb, ref.rbud, name + " rgb")
    assert float((sigma.cpu() - f.sigma).abs().max()) <= 1e-5 and float((rgb.cpu() - f.rgb).abs().max()) <= 1e-5


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_rgb", [True, False], ids=["rgb", "sigma-only"])
@pytest.mark.parametrize("N", R.SIZES)
@pytest.mark.parametrize("c", R.SIZE_CASES, **_ids)
def test_kernel_stops_at_row_n(native_lib, c, N, want_rgb):
    """N on and next to the points of a gather pass (8), an MFMA tile (32 / 64) and a workgroup (T), and 3 T + 5: rows < N within
    budget, the 64 rows behind them of the over-allocated outputs bit-unchanged."""
    cx, _ = _cx()
    g = torch.Generator().manual_seed(N)
    sigma = torch.randn(N + R.SENTINEL_ROWS, generator=g).to(DEV)
    rgb = torch.randn(N + R.SENTINEL_ROWS, 32, generator=g).to(DEV)
    s_before, rgb_before = sigma.clone(), rgb.clone()
    cx.check(_points_direct(c, N, sigma, rgb if want_rgb else None))
    ref = R.reference_of(c)
    assert torch.equal(_bits(sigma[N:]), _bits(s_before[N:]))
    R.assert_within(sigma[:N], ref.sigma[:N], ref.sbud[:N], f"{c.name} N={N} sigma")
    if want_rgb:
        assert torch.equal(_bits(rgb[N:]), _bits(rgb_before[N:]))
        R.assert_within(rgb[:N], ref.rgb[:N], ref.rbud[:N], f"{c.name} N={N} rgb")
    else:
        assert torch.equal(_bits(rgb), _bits(rgb_before))


# ---- softplus range ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.RANGE_CASES, **_ids)
def test_softplus_from_minus_90_to_plus_90(native_lib, c):
    """W1 scaled so that the pre-activations pass +-25 (the threshold is 20) and +-90 (e^-90 is subnormal): the hidden values
    keep their relative accuracy, so sigma and rgb stay within budget"""
    _, _, pos = _inputs(c)
    ref = R.reference_of(c)
    assert float(ref.z.max()) > 90 and float(ref.z.min()) < -90
    sigma, rgb = _field(c, pos)
    R.assert_within(sigma, ref.sigma, ref.sbud, c.name + " sigma")
    R.assert_within(rgb, ref.rgb, ref.rbud, c.name + " rgb")


# ---- lattice -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lattice", ["reference", "regular"])
@pytest.mark.parametrize("n,cube", R.FIX_LATTICES + [(128, 1.0)])
def test_device_lattice_is_bit_equal_to_the_host_lattice(native_lib, n, cube, lattice):
    got = density.lattice_points(n, cube, lattice, device=DEV)
    want = density.lattice_points(n, cube, lattice)
    assert got.shape == (n ** 3, 3) and torch.equal(_bits(got.cpu()), _bits(want))
    if lattice == "reference" and n < 128:
        assert torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(R.FIX[f"lattice_{n}_{cube}"])))


@functools.lru_cache(maxsize=None)
def _grid_inputs(D, axes):
    """16 x 16 planes for the grid tests, with weights of a table case of the same form"""
    c = R.BY_NAME[{(3, "panohead"): "D3-panohead-none-lr1", (0, "eg3d"): "D0-eg3d-sigmoid-lr1"}[(D, axes)]]
    g = torch.Generator().manual_seed(41 + D)
    planes = torch.randn(3, 32 * max(D, 1), 16, 16, generator=g)
    return c, planes, planes_channels_last(planes, D or None).to(DEV), density.osg_weights(R.build(c).decoder)


@pytest.mark.parametrize("lattice", ["reference", "regular"])
@pytest.mark.parametrize("n", [5, 12, 128])
@pytest.mark.parametrize("D,axes", [(3, "panohead"), (0, "eg3d")])
def test_grid_is_bit_equal_to_the_field_at_the_lattice_points(native_lib, D, axes, n, lattice):
    """coordinates generated in registers against coordinates read from memory (n = 128: 2 097 152 points, 16 384 workgroups);
    at n = 12 also against float64"""
    c, planes, cl, w = _grid_inputs(D, axes)
    cube = 1.6 if n == 5 else c.box_warp
    pts = density.lattice_points(n, cube, lattice, device=DEV)
    kw = dict(box_warp=c.box_warp, plane_axes=axes, triplane_depth=D or None)
    sigma, rgb = density.density_grid(cl, w.to(DEV), n, cube, lattice=lattice, want_rgb=True, **kw)
    assert sigma.shape == (n, n, n) and rgb.shape == (n, n, n, 32)
    s_pts, rgb_pts = density.sample_field(cl, w.to(DEV), pts, want_rgb=True, **kw)
    assert torch.equal(_bits(sigma.view(-1)), _bits(s_pts)) and torch.equal(_bits(rgb.view(-1, 32)), _bits(rgb_pts))
    only = density.density_grid(cl, w.to(DEV), n, cube, lattice=lattice, **kw)
    assert torch.equal(_bits(only), _bits(sigma))
    if n == 12:
        ref = R.reference(planes, pts.cpu(), c.box_warp, axes, D, w.w1, w.b1, w.w2, w.b2, w.activation)
        R.assert_within(sigma.view(-1), ref.sigma, ref.sbud, f"grid n={n} sigma")
        R.assert_within(rgb.view(-1, 32), ref.rgb, ref.rbud, f"grid n={n} rgb")


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_sample_target_points_is_the_two_calls_made_by_hand(native_lib):
    """planes -> sigma grid -> surface points; the sigma bias is shifted so that the grid crosses the level"""
    c, planes, cl, w = _grid_inputs(3, "panohead")
    n, level = 32, 10.0
    kw = dict(box_warp=c.box_warp, plane_axes="panohead", triplane_depth=3)
    base = density.density_grid(cl, w.to(DEV), n, **kw)
    b2 = w.b2.clone()
    b2[0] += level - float(base.median())
    w = density.osg_weights(w.w1, w.b1, w.w2, b2, activation=w.activation).to(DEV)
    sigmas = density.density_grid(cl, w, n, **kw)
    assert float(sigmas.min()) < level < float(sigmas.max())
    pos, nf = sample_target_points(cl, w, n=n, level=level, num_points=4096, surface_thickness=0.1, seed=5, **kw)
    pos2, nf2 = sample_surface_points(sigmas, level, 4096, 0.1, 5)
    assert int(nf) > 0 and int(nf) == int(nf2)
    assert pos.shape == (4096, 3) and torch.equal(_bits(pos), _bits(pos2))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_leave_the_outputs_alone(native_lib):
    c = R.SIZE_CASES[0]
    cl, w, pos = _inputs(c)
    cx, stream = _cx()
    sigma, rgb = torch.randn(16, device=DEV), torch.randn(16, 32, device=DEV)
    before = sigma.clone(), rgb.clone()

    def refused(rc):
        assert rc == -1                              # GGD_E_INVALID
        with pytest.raises(_capi.RasterError):
            cx.check(rc)

    refused(_points_direct(c, 16, sigma, rgb, C_=16))
    refused(_points_direct(c, 16, sigma, rgb, C_=64))
    refused(_points_direct(c, 16, sigma, rgb, act=3))
    refused(_points_direct(c, 16, None, rgb))
    plane_args = [_vp(cl), 32, c.D, R.H, R.W, AXES[c.axes], c.box_warp, _vp(w.w1), _vp(w.b1), _vp(w.w2), _vp(w.b2), 2]
    with torch.cuda.device(DEV):
        for n, cube, lattice in ((1025, 1.0, 0), (1, 1.0, 0), (2, 1.0, 2), (2, 0.0, 0)):
            refused(cx.lib.ggd_density_grid(cx.handle, stream, *plane_args, n, cube, lattice, _vp(sigma), _vp(rgb)))
            refused(cx.lib.ggd_density_lattice(cx.handle, stream, n, cube, lattice, _vp(rgb)))
    torch.cuda.synchronize()
    assert torch.equal(_bits(sigma), _bits(before[0])) and torch.equal(_bits(rgb), _bits(before[1]))
    kw = dict(box_warp=c.box_warp, plane_axes=c.axes, triplane_depth=c.D)
    with pytest.raises(ValueError, match="one device"):      # CPU and CUDA tensors mixed
        density.sample_field(cl, w, pos.cpu(), **kw)
    with pytest.raises(ValueError, match="one device"):
        density.sample_field(cl, w.to("cpu"), pos, **kw)
    with pytest.raises(ValueError, match="one device"):
        density.density_grid(cl.cpu(), w, 5, **kw)
