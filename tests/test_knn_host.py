"""CPU tests of the 3-nearest-neighbour feature (no GPU): the brute-force oracle against itself in double precision, the new
exports, the search kernels' resources, the simple_knn shim and the argument checks of gaussian_gan_decoder_amd.knn."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import _knn_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def clouds():
    return KR.clouds(20000, seed=0)


@pytest.mark.parametrize("name", ["uniform", "two_far_clusters", "lattice", "duplicates_x4", "sphere"])
def test_fp32_oracle_agrees_with_fp64(clouds, name):
    """Bar 1e-6 relative, derived: at most about 8 fp32 roundings on sums of non-negative terms (3 subtractions feed 3
    squares, 2 sums; then 2 sums and a division) = 8 * 2^-24 = 4.8e-7, doubled.  A neighbour SWAP between the two precisions
    only happens between candidates whose distances agree to that order, so it stays inside the bar."""
    p = clouds[name]
    a = KR.brute_mean_dist2(p, np.float32)
    b = KR.brute_mean_dist2(p, np.float64)
    assert a.dtype == np.float32 and b.dtype == np.float64
    rel = float((np.abs(a.astype(np.float64) - b) / np.maximum(b, np.finfo(np.float64).tiny)).max())
    print(f"{name}: P={len(p)} max rel |fp32 - fp64| = {rel:.3e}")
    assert (np.abs(a.astype(np.float64) - b) <= 1e-6 * b).all(), rel
    if name == "duplicates_x4":
        assert (a == 0).all() and (b == 0).all()


def test_fp32_oracle_is_bit_equal_under_a_row_permutation(clouds):
    p = clouds["uniform"][:6000]
    perm = np.random.default_rng(5).permutation(len(p))
    a = KR.brute_mean_dist2(p)
    b = KR.brute_mean_dist2(p[perm])
    assert (a[perm].view(np.uint32) == b.view(np.uint32)).all()


def test_knn_symbols_are_exported(native_lib):
    from gaussian_gan_decoder_amd import _capi
    for s in ("ggd_knn_tmp_bytes", "ggd_knn_leaf_size", "ggd_knn3"):
        assert s in _capi.EXPORTS
        assert hasattr(native_lib, s), s
    hdr = open(os.path.join(ROOT, "include", "ggd_raster.h")).read()
    for s in ("ggd_knn_tmp_bytes", "ggd_knn_leaf_size", "ggd_knn3"):
        assert re.search(r"\b" + s + r"\(", hdr), s
    L = native_lib.ggd_knn_leaf_size()
    assert 64 <= L <= 4096
    assert native_lib.ggd_knn_max_points() >= 4 * 1024 * 1024
    assert native_lib.ggd_knn_tmp_bytes(3) == 0                       # no three neighbours
    assert native_lib.ggd_knn_tmp_bytes(1 << 20) >= 16 * (1 << 20)     # the gathered float4 points at least


def test_knn_kernels_have_no_spills_and_no_scratch(native_lib):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    from gaussian_gan_decoder_amd import _capi
    tab = {kr.short(k): v for k, v in kr.kernel_resources(_capi.LIB_PATH).items()}
    knn = {k: v for k, v in tab.items() if k.startswith("knn_")}
    assert {re.sub(r"<.*", "", k) for k in knn} >= {"knn_box_kernel", "knn_codes_kernel", "knn_leaves_kernel", "knn_search_kernel"}, sorted(tab)
    assert sum(k.startswith("knn_search_kernel<") for k in knn) == 2      # plain + counting instance
    for name, r in knn.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)


def test_simple_knn_shim_resolves_to_the_kernel_wrapper():
    from simple_knn._C import distCUDA2
    import simple_knn
    from gaussian_gan_decoder_amd import knn
    assert distCUDA2 is knn.dist_cuda2
    assert simple_knn.distCUDA2 is knn.dist_cuda2
    assert os.path.dirname(os.path.abspath(simple_knn.__file__)) == os.path.join(ROOT, "simple_knn")


def test_setup_lists_the_shim_package():
    text = open(os.path.join(ROOT, "setup.py")).read()
    m = re.search(r"packages=\[([^\]]*)\]", text)
    assert m and '"simple_knn"' in m.group(1) and '"diff_gaussian_rasterization"' in m.group(1)


def test_cpu_tensors_raise_before_any_native_call(monkeypatch):
    from gaussian_gan_decoder_amd import _capi, knn

    def no_native(*a, **k):
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_capi, "load", no_native)
    monkeypatch.setattr(_capi, "context_for", no_native)
    monkeypatch.setattr(_capi, "context_and_stream", no_native)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn.dist_cuda2(torch.zeros(8, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn.knn3(torch.zeros(8, 3), return_examined=True)


@pytest.mark.parametrize("fn", ["dist_cuda2", "knn3"])
def test_bad_arguments_raise(monkeypatch, fn):
    from gaussian_gan_decoder_amd import _capi, knn

    def no_native(*a, **k):
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_capi, "load", no_native)
    monkeypatch.setattr(_capi, "context_and_stream", no_native)
    f = getattr(knn, fn)
    for bad in (torch.zeros(8), torch.zeros(8, 4), torch.zeros(2, 8, 3), torch.zeros(3, 8)):
        with pytest.raises(ValueError, match=r"\[P, 3\]"):
            f(bad)
    for bad in (torch.zeros(8, 3, dtype=torch.float64), torch.zeros(8, 3, dtype=torch.float16), torch.zeros(8, 3, dtype=torch.int32)):
        with pytest.raises(TypeError, match="float32"):
            f(bad)
    for P in (0, 1, 3):
        with pytest.raises(ValueError, match="at least 4"):
            f(torch.zeros(P, 3))
    with pytest.raises(TypeError):
        f(np.zeros((8, 3), np.float32))


def test_model_helpers():
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel, inverse_sigmoid
    from gaussian_gan_decoder_amd.sh import RGB2SH, SH2RGB
    x = torch.tensor([0.1, 0.5, 0.9])
    assert torch.allclose(torch.sigmoid(inverse_sigmoid(x)), x, atol=1e-6)
    c = torch.rand(5, 3)
    assert torch.allclose(SH2RGB(RGB2SH(c)), c, atol=1e-6)
    assert callable(GaussianModel.create_from_pcd) and callable(GaussianModel.create_from_pos_col)
