"""The 3-nearest-neighbour kernel (gaussian_gan_decoder_amd.knn, csrc/ggd_knn.hip) on the GPU.  Every comparison with the
numpy fp32 brute force of tests/_knn_ref.py is BIT FOR BIT (the kernel evaluates the same expression in the same order and
its pruning never changes a value); the model constructors built on it are compared with the same torch ops."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _knn_ref as KR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _gpu_mean(p):
    from gaussian_gan_decoder_amd import knn
    return knn.dist_cuda2(torch.from_numpy(np.ascontiguousarray(p)).to(DEV)).cpu().numpy()


def _assert_bit_equal(got, want, what):
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.fixture(scope="module")
def clouds():
    return KR.clouds(20000, seed=0)


@pytest.mark.parametrize("name", ["uniform", "two_far_clusters", "lattice", "duplicates_x4", "sphere"])
def test_bit_exact_against_the_brute_force(clouds, name):
    p = clouds[name]
    got = _gpu_mean(p)
    assert got.shape == (len(p),) and got.dtype == np.float32
    _assert_bit_equal(got, KR.brute_mean_dist2(p), name)
    if name == "duplicates_x4":
        assert (got == 0).all()


def test_small_and_leaf_boundary_sizes():
    from gaussian_gan_decoder_amd import knn
    L = knn.leaf_size()
    g = np.random.default_rng(11)
    for P in (4, 5, 63, 64, 65, L - 1, L, L + 1, 2 * L + 1, 3 * L + 7):
        p = g.normal(size=(P, 3)).astype(np.float32)
        _assert_bit_equal(_gpu_mean(p), KR.brute_mean_dist2(p), f"P={P}")


def test_identical_points_stay_linear():
    """P copies of one point: all zeros, and at most 8 * P * L evaluated candidates.  One leaf makes every third-best 0 and the
    >= rule prunes the rest; a quadratic path evaluates P candidates per query = 1024 L at L = 256 and still 64 L at the largest
    allowed leaf, so the bound tells the two apart."""
    from gaussian_gan_decoder_amd import knn
    P = 262144
    L = knn.leaf_size()
    p = torch.full((P, 3), 0.25, dtype=torch.float32, device=DEV)
    p[:, 1] = -1.5
    d2, idx, examined = knn.knn3(p, return_examined=True)
    assert examined.dtype == torch.int64 and examined.dim() == 0
    n = int(examined.item())
    print(f"identical points: examined / P = {n / P:.1f} (L = {L})")
    assert (d2 == 0).all() and (knn.dist_cuda2(p) == 0).all()
    rows = torch.arange(P, device=DEV, dtype=torch.int32)[:, None]
    assert ((idx != rows).all() and (idx >= 0).all() and (idx < P).all())
    assert 0 < n <= 8 * P * L, (n, P, L)


def test_permutation_invariance_and_determinism(clouds):
    p = clouds["uniform"]
    a = _gpu_mean(p)
    b = _gpu_mean(p)
    assert (_bits(a) == _bits(b)).all()
    perm = np.random.default_rng(3).permutation(len(p))
    c = _gpu_mean(p[perm])
    assert (_bits(c) == _bits(a[perm])).all()
    q = clouds["duplicates_x4"]                     # ties everywhere: the values still do not move
    perm = np.random.default_rng(4).permutation(len(q))
    assert (_bits(_gpu_mean(q[perm])) == _bits(_gpu_mean(q)[perm])).all()


@pytest.mark.parametrize("name", ["uniform", "duplicates_x4", "lattice"])
def test_knn3_outputs(clouds, name):
    from gaussian_gan_decoder_amd import knn
    p = clouds[name]
    t = torch.from_numpy(p).to(DEV)
    d2, idx, examined = knn.knn3(t, return_examined=True)
    d2b, idxb = knn.knn3(t)
    assert d2.shape == (len(p), 3) and d2.dtype == torch.float32 and idx.shape == (len(p), 3) and idx.dtype == torch.int32
    assert not d2.requires_grad
    assert torch.equal(d2, d2b)                     # the counting instance computes the same values
    d, i = d2.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
    assert (d[:, 0] <= d[:, 1]).all() and (d[:, 1] <= d[:, 2]).all()
    rows = np.arange(len(p))
    assert (i >= 0).all() and (i < len(p)).all() and (i != rows[:, None]).all()
    assert (i[:, 0] != i[:, 1]).all() and (i[:, 0] != i[:, 2]).all() and (i[:, 1] != i[:, 2]).all()
    for k in range(3):
        _assert_bit_equal(d[:, k], KR.dist2_of(p, rows, i[:, k]), f"{name} column {k}")
    _assert_bit_equal(d, KR.brute_knn3(p), name)
    _assert_bit_equal(knn.dist_cuda2(t).cpu().numpy(), KR.mean_of(d), name)
    L = knn.leaf_size()
    n = int(examined.item())
    print(f"{name}: examined / P = {n / len(p):.1f} = {n / len(p) / L:.2f} L")
    assert len(p) * 3 <= n <= len(p) * (len(p) - 1)


def test_non_contiguous_input_and_side_stream(clouds):
    from gaussian_gan_decoder_amd import knn
    p = clouds["sphere"]
    want = KR.brute_mean_dist2(p)
    wide = torch.zeros((len(p), 4), dtype=torch.float32, device=DEV)
    wide[:, :3] = torch.from_numpy(p).to(DEV)
    view = wide[:, :3]
    assert not view.is_contiguous()
    _assert_bit_equal(knn.dist_cuda2(view).cpu().numpy(), want, "sliced [P, 4]")
    cols = torch.from_numpy(np.ascontiguousarray(p.T)).to(DEV).t()
    assert not cols.is_contiguous()
    _assert_bit_equal(knn.dist_cuda2(cols).cpu().numpy(), want, "transposed")
    s = torch.cuda.Stream(device=DEV)
    t = torch.from_numpy(p).to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out = knn.dist_cuda2(t)
    s.synchronize()
    _assert_bit_equal(out.cpu().numpy(), want, "side stream")
    g = knn.dist_cuda2(t.clone().requires_grad_(True))
    assert not g.requires_grad


def test_short_input_raises_on_the_device():
    from gaussian_gan_decoder_amd import knn
    with pytest.raises(ValueError):
        knn.dist_cuda2(torch.zeros((3, 3), device=DEV))
    import ctypes as C
    from gaussian_gan_decoder_amd import _capi
    cx, stream = _capi.context_and_stream(DEV)
    tmp = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    pts = torch.zeros((3, 3), device=DEV)
    out = torch.zeros(3, device=DEV)
    rc = cx.lib.ggd_knn3(cx.handle, C.c_void_p(stream), C.c_void_p(pts.data_ptr()), 3, C.c_void_p(out.data_ptr()), None, None,
                         None, C.c_void_p(tmp.data_ptr()), tmp.numel())
    assert rc == -1                                 # GGD_E_INVALID


def _sphere_field(n):
    """density grid of a sphere of radius 0.3 in the sampler's units (index / n - 0.5): level 10 at the surface"""
    ax = (np.arange(n, dtype=np.float32) / np.float32(n)) - np.float32(0.5)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    d = np.float32(0.3) - np.sqrt(x * x + y * y + z * z)
    return (np.float32(10.0) + np.float32(400.0) * d).astype(np.float32)


def _check_subset(points_dev, got_dev, seed, what):
    got = got_dev.cpu().numpy()
    assert np.isfinite(got).all() and (got >= 0).all(), what
    p = points_dev.cpu().numpy()
    rows = np.sort(np.random.default_rng(seed).choice(len(p), 2048, replace=False))
    _assert_bit_equal(got[rows], KR.brute_mean_dist2(p, np.float32, rows), what)


def test_surface_sample_workload():
    from gaussian_gan_decoder_amd import knn
    from gaussian_gan_decoder_amd.target_sampler import sample_surface_points
    sig = torch.from_numpy(_sphere_field(128)).to(DEV)
    pos, _ = sample_surface_points(sig, level=10.0, num_points=500_000, surface_thickness=0.1, seed=7)
    assert pos.shape == (500_000, 3)
    _check_subset(pos, knn.dist_cuda2(pos), 21, "500 000 surface samples")


def test_full_size_uniform():
    from gaussian_gan_decoder_amd import knn
    g = torch.Generator(device="cpu").manual_seed(9)
    p = (torch.rand((1_000_000, 3), generator=g) - 0.5).to(DEV)
    _check_subset(p, knn.dist_cuda2(p), 22, "1 000 000 uniform points")


class _Cloud:
    def __init__(self, points, colors):
        self.points, self.colors = points, colors


@pytest.mark.parametrize("deg", [0, 3])
def test_create_from_pcd_and_pos_col(deg):
    from gaussian_gan_decoder_amd import knn
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel, inverse_sigmoid
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    from gaussian_gan_decoder_amd.sh import SH2RGB
    from gaussian_gan_decoder_amd.synthetic import make_camera
    P = 10000
    g = np.random.default_rng(deg)
    pts = (g.random((P, 3)) * 0.6 - 0.3).astype(np.float32)       # numpy in, as the reference's BasicPointCloud holds
    col = g.random((P, 3)).astype(np.float32)
    dev_pts = torch.from_numpy(pts).to(DEV)
    want_scale = torch.log(torch.sqrt(torch.clamp_min(knn.dist_cuda2(dev_pts), 1e-7)))

    def check_common(m, colours):
        K = (deg + 1) ** 2
        assert m._xyz.shape == (P, 3) and m._features_dc.shape == (P, 1, 3) and m._features_rest.shape == (P, K - 1, 3)
        assert m._scaling.shape == (P, 3) and m._rotation.shape == (P, 4) and m._opacity.shape == (P, 1)
        assert m.max_radii2D.shape == (P,) and (m.max_radii2D == 0).all()
        for name in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"):
            t = getattr(m, name)
            assert isinstance(t, torch.nn.Parameter) and t.requires_grad and t.is_cuda and t.dtype == torch.float32, name
        assert torch.equal(m._xyz.detach(), dev_pts)
        assert (m._features_rest == 0).all()
        # (c - 0.5) / C0 * C0 + 0.5: four fp32 roundings on values below 2 -> 4 * 2^-23 = 4.8e-7
        assert torch.allclose(SH2RGB(m._features_dc.detach()[:, 0, :]), colours, rtol=0, atol=1e-6)

    m = GaussianModel(deg)
    m.create_from_pcd(_Cloud(pts, col), 2.5)
    assert m.spatial_lr_scale == 2.5
    check_common(m, torch.from_numpy(col).to(DEV))
    for k in range(3):
        assert torch.equal(m._scaling.detach()[:, k], want_scale)
    assert torch.equal(m._rotation.detach(), torch.tensor([1.0, 0, 0, 0], device=DEV).expand(P, 4))
    assert torch.equal(m._opacity.detach(), inverse_sigmoid(0.1 * torch.ones((P, 1), device=DEV)))
    cam = make_camera(64, device=DEV)
    out = render_simple(cam, m, bg_color=torch.zeros(3, device=DEV))
    assert out["render"].shape == (3, 64, 64) and torch.isfinite(out["render"]).all()
    out["render"].sum().backward()
    assert m._xyz.grad is not None and torch.isfinite(m._xyz.grad).all()

    # positions alone (device tensor in): grey, default opacity
    m = GaussianModel(deg)
    m.create_from_pos_col(dev_pts)
    assert m.spatial_lr_scale == 1
    check_common(m, torch.full((P, 3), 0.5, device=DEV))
    assert torch.equal(m._scaling.detach(), want_scale[:, None].repeat(1, 3))
    assert torch.equal(m._opacity.detach(), inverse_sigmoid(0.1 * torch.ones((P, 1), device=DEV)))

    # every option: colours clipped to 0..1, opacity floored at 0.1, overrides in the leading rows
    n_s, n_r = 100, 50
    scaling = torch.full((n_s, 3), -3.0, device=DEV)
    rotation = torch.tensor([0.0, 1.0, 0.0, 0.0], device=DEV).expand(n_r, 4).contiguous()
    opacity = g.random((P, 1)).astype(np.float32) * 0.9
    m = GaussianModel(deg)
    m.create_from_pos_col(pts, colors=col * 1.5 - 0.25, opacity=opacity, rotation=rotation, scaling=scaling)
    check_common(m, torch.from_numpy(np.clip(col * 1.5 - 0.25, 0, 1)).to(DEV))
    sc, ro = m._scaling.detach(), m._rotation.detach()
    assert torch.equal(sc[:n_s], scaling) and torch.equal(sc[n_s:], want_scale[n_s:, None].repeat(1, 3))
    assert torch.equal(ro[:n_r], rotation) and torch.equal(ro[n_r:], torch.tensor([1.0, 0, 0, 0], device=DEV).expand(P - n_r, 4))
    assert torch.equal(m.target_scales.detach(), sc) and torch.equal(m.target_rots.detach(), ro)
    assert torch.equal(m._opacity.detach(), inverse_sigmoid(torch.clamp(torch.from_numpy(opacity).to(DEV), min=0.1)))
    out = render_simple(cam, m, bg_color=torch.zeros(3, device=DEV))
    assert torch.isfinite(out["render"]).all()
