"""Host checks of the density field (gaussian_gan_decoder_amd/density.py) and of tests/_density_ref.py: the torch form and
osg_weights against the values the reference's own code produced (tests/golden/density_fixture.npz), the lattice bit for bit
against create_samples, the measurement of KAPPA, and the argument checks."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import _capi, density
from gaussian_gan_decoder_amd.decoder import planes_channels_last
import _density_ref as R

FIX, FIX_CASES, LATTICES = R.FIX, R.FIX_CASES, R.FIX_LATTICES


def _torch_form(planes, pos, decoder, D, axes, box_warp):
    w = density.osg_weights(decoder)
    sigma, rgb = density.sample_field(planes_channels_last(planes, D or None), w, pos, box_warp, axes, D or None, want_rgb=True)
    return w, sigma, rgb


@functools.lru_cache(maxsize=None)
def _measure_fixture(name):
    """worst ratios (fixture values, torch form) of a fixture case against the float64 restatement"""
    f = R.fixture_case(name)
    w, sigma, rgb = _torch_form(f.planes, f.coords, f.decoder, f.D, f.axes, f.box_warp)
    assert w.activation == f.act
    ref = R.reference(f.planes, f.coords, f.box_warp, f.axes, f.D, w.w1, w.b1, w.w2, w.b2, f.act)
    fix = max(R.worst_ratio(f.sigma, ref.sigma, ref.sbud), R.worst_ratio(f.rgb, ref.rgb, ref.rbud))
    tor = max(R.worst_ratio(sigma, ref.sigma, ref.sbud), R.worst_ratio(rgb, ref.rgb, ref.rbud))
    return fix, tor


@functools.lru_cache(maxsize=None)
def _measure_case(c):
    """worst ratio of torch's fp32 CPU evaluation of a table case (finite rows) against the float64 restatement"""
    b = R.build(c)
    ref = R.reference_of(c)
    fin = torch.isfinite(b.pos).all(1)
    _, sigma, rgb = _torch_form(b.planes, b.pos[fin], b.decoder, c.D, c.axes, c.box_warp)
    return max(R.worst_ratio(sigma, ref.sigma[fin], ref.sbud[fin]), R.worst_ratio(rgb, ref.rgb[fin], ref.rbud[fin]))


@pytest.mark.parametrize("name", FIX_CASES)
def test_torch_form_and_osg_weights_reproduce_the_reference(name):
    """the reference's run_model output and this package's torch form on the same inputs: both within the budget of the float64
    restatement, and close to each other"""
    fix, tor = _measure_fixture(name)
    print(f"\n  {name}: worst ratio, the reference's values {fix:.3f}, the torch form {tor:.3f}")
    assert fix <= R.KAPPA / 2.0 and tor <= R.KAPPA / 2.0
    f = R.fixture_case(name)
    _, sigma, rgb = _torch_form(f.planes, f.coords, f.decoder, f.D, f.axes, f.box_warp)
    assert float((sigma - f.sigma).abs().max()) <= 1e-5 and float((rgb - f.rgb).abs().max()) <= 1e-5


def test_fixture_covers_the_forms_the_issue_names():
    metas = {(str(FIX[n + ".teacher"]), int(FIX[n + ".meta"][0]), str(FIX[n + ".activation"]), float(FIX[n + ".meta"][1]))
             for n in FIX_CASES}
    assert {m[1] for m in metas if m[0] == "PanoHead"} == {1, 3}
    assert {m[2] for m in metas if m[0] == "PanoHead"} == {"sigmoid", "lrelu", "none"}
    assert {m[3] for m in metas} == {1.0, 2.0} and any(m[0] == "eg3d" for m in metas)


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c.name)
def test_fp32_torch_sits_inside_the_budget(c):
    w = _measure_case(c)
    print(f"\n  {c.name}: worst fp32-torch / (2^-24 * budget) = {w:.3f}")
    assert math.isfinite(w) and w <= R.KAPPA / 2.0


def test_kappa_is_twice_the_measured_ratio_rounded_up():
    w = max([max(_measure_fixture(n)) for n in FIX_CASES] + [_measure_case(c) for c in R.CASES])
    print(f"\n  worst ratio over the fixture and the table: {w:.3f} -> KAPPA = ceil(2 * {w:.3f}) = {math.ceil(2.0 * w)}"
          f" (recorded: {R.KAPPA_MEASURED}, KAPPA = {R.KAPPA})")
    assert w <= R.KAPPA / 2.0
    assert math.ceil(2.0 * w) == R.KAPPA          # neither tighter nor wider than 2 x what is measured here, rounded up
    assert R.KAPPA == math.ceil(2.0 * R.KAPPA_MEASURED)


def test_softplus_range_cases_reach_beyond_25_and_90():
    for c in R.RANGE_CASES:
        z = R.reference_of(c).z
        assert float(z.max()) > 90 and float(z.min()) < -90
        assert bool(((z > 25) & (z < 90)).any()) and bool(((z < -25) & (z > -90)).any()) and bool((z.abs() < 20).any())


def test_pool_carries_every_kind_of_row():
    for c in R.FORM_CASES:
        pos, ref = R.build(c).pos, R.reference_of(c)
        assert pos.shape == (R.POOL, 3)
        assert int(torch.isnan(pos).any(1).sum()) == 4 and int(torch.isinf(pos).any(1).sum()) == 6
        assert int((pos.abs() == float(np.float32(1e30))).any(1).sum()) == 6
        free = (ref.fbud == 0).all(1)              # rows with no tap at all: the zero-feature result
        assert bool(free.any()) and bool((~free).any())


@pytest.mark.parametrize("n,cube", LATTICES)
def test_reference_lattice_is_bit_equal_to_create_samples(n, cube):
    want = torch.from_numpy(FIX[f"lattice_{n}_{cube}"])
    got = density.lattice_points(n, cube, "reference")
    assert got.dtype == torch.float32 and got.shape == (n ** 3, 3)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("n,cube", LATTICES)
def test_regular_lattice_has_integer_indices_and_differs(n, cube):
    reg, ref = density.lattice_points(n, cube, "regular"), density.lattice_points(n, cube, "reference")
    assert not torch.equal(reg, ref)
    idx = (reg.double() + cube / 2.0) / (cube / (n - 1))
    assert float((idx - idx.round()).abs().max()) < 1e-4
    i = torch.arange(n ** 3)
    assert torch.equal(idx.round().long(), torch.stack([i // (n * n), (i // n) % n, i % n], 1))
    assert torch.equal(reg[:, 2], ref[:, 2])       # the z index is an integer in both


def test_density_grid_on_the_cpu_is_the_torch_form_on_the_lattice():
    c = R.BY_NAME["D3-panohead-none-lr1"]
    b = R.build(c)
    cl = planes_channels_last(b.planes, c.D)
    w = density.osg_weights(b.decoder)
    sig, rgb = density.density_grid(cl, w, 5, None, c.box_warp, c.axes, c.D, want_rgb=True)
    s2, r2 = density.sample_field_torch(cl, w, density.lattice_points(5, c.box_warp), c.box_warp, c.axes, c.D, want_rgb=True)
    assert sig.shape == (5, 5, 5) and rgb.shape == (5, 5, 5, 32)
    assert torch.equal(sig.reshape(-1), s2) and torch.equal(rgb.reshape(-1, 32), r2)
    assert torch.equal(density.density_grid(cl, w, 5, None, c.box_warp, c.axes, c.D).reshape(-1),
                       density.sample_field_torch(cl, w, density.lattice_points(5, c.box_warp), c.box_warp, c.axes, c.D))


def test_osg_weights_takes_tensors_and_applies_the_gains_in_fp32():
    c = R.BY_NAME["D1-panohead-lrelu-lr2"]
    dec = R.build(c).decoder
    w = density.osg_weights(dec)
    assert w.activation == "lrelu" and all(t.dtype == torch.float32 for t in w[:4])
    assert torch.equal(w.w1, dec.net[0].weight * float(np.float32(dec.net[0].weight_gain)))
    assert torch.equal(w.b2, dec.net[2].bias * 2.0)
    again = density.osg_weights(w.w1, w.b1, w.w2, w.b2, activation="none")
    assert again.activation == "none" and torch.equal(again.w2, w.w2)
    assert density.osg_weights(w.w1, w.b1, w.w2, w.b2).activation == "sigmoid"
    assert density.osg_weights(w) is w


def test_argument_checks():
    c = R.BY_NAME["D0-eg3d-sigmoid-lr1"]
    b = R.build(c)
    cl = planes_channels_last(b.planes, None)
    w = density.osg_weights(b.decoder)
    pos = b.pos[:9]
    with pytest.raises(ValueError, match="channels"):
        density.sample_field(torch.zeros(3, R.H, R.W, 16), w, pos)
    with pytest.raises(ValueError, match="first layer"):
        density.osg_weights(torch.zeros(128, 32), torch.zeros(128), torch.zeros(33, 128), torch.zeros(33))
    with pytest.raises(ValueError, match="second layer"):
        density.osg_weights(w.w1, w.b1, torch.zeros(4, 64), torch.zeros(4))
    with pytest.raises(ValueError, match="activation"):
        density.osg_weights(w.w1, w.b1, w.w2, w.b2, activation="tanh")
    for bad in (1025, 1):
        with pytest.raises(ValueError, match="n ="):
            density.density_grid(cl, w, bad)
        with pytest.raises(ValueError, match="n ="):
            density.lattice_points(bad)
    with pytest.raises(ValueError, match="lattice"):
        density.lattice_points(5, 1.0, "sheared")
    with pytest.raises(ValueError, match="EG3D plane axes"):
        density.sample_field(cl, w, pos, plane_axes="panohead")
    with pytest.raises(ValueError, match="channel-last"):
        density.sample_field(b.planes, w, pos, triplane_depth=3)
    with pytest.raises(ValueError, match="one device"):
        density.sample_field(cl, w, pos.to("meta"))
    with pytest.raises(ValueError, match="one device"):
        density.density_grid(cl, w.to("meta"), 5)


def test_new_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(R.ROOT, "include", "ggd_raster.h")).read()
    for sym in ("ggd_density_points", "ggd_density_grid", "ggd_density_lattice"):
        assert sym in _capi.EXPORTS and f"int {sym}(" in hdr
    assert "double cube_length" in hdr
