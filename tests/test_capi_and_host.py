"""CPU tests: the C-ABI library builds, loads and exports every symbol include/ggd_raster.h declares (no compute
without a GPU), layout queries are consistent, and the host-side API mirrors the reference's behaviour."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(native_lib):
    hdr = open(os.path.join(ROOT, "include", "ggd_raster.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ggd_[a-z_0-9]+)\s*\(", hdr))
    assert len(declared) >= 20
    from gaussian_gan_decoder_amd import _capi
    assert declared == set(_capi.EXPORTS), declared ^ set(_capi.EXPORTS)
    for sym in declared:
        assert hasattr(native_lib, sym), f"libggd_raster.so does not export {sym}"


def test_option_and_counter_constants_match_the_header():
    """_capi's OPT_* / STAT_* numbers are the enum values of include/ggd_raster.h (the binding passes them as plain ints)."""
    import os
    import re
    from gaussian_gan_decoder_amd import _capi
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ggd_raster.h")).read()
    val = lambda name: int(re.search(r"\b" + name + r"\s*=\s*(\d+)", hdr).group(1))
    assert (_capi.OPT_EXP_MODE, _capi.OPT_BLEND_CULL, _capi.OPT_BINNING, _capi.OPT_BLEND_SPLIT, _capi.OPT_FOLD) == tuple(
        val(n) for n in ("GGD_OPT_EXP_MODE", "GGD_OPT_BLEND_CULL", "GGD_OPT_BINNING", "GGD_OPT_BLEND_SPLIT", "GGD_OPT_FOLD"))
    assert (_capi.STAT_FLAT_STREAK, _capi.STAT_SORT_RERUNS) == (val("GGD_STAT_FLAT_STREAK"), val("GGD_STAT_SORT_RERUNS"))
    # ... and every other one: each GGD_OPT_* / GGD_STAT_* enumerator the header gives a number has its _capi constant
    enum = dict(re.findall(r"^\s*GGD_((?:OPT|STAT)_[A-Z0-9_]+)\s*=\s*(\d+)", hdr, flags=re.M))
    assert len([n for n in enum if n.startswith("OPT_")]) == 8 and len([n for n in enum if n.startswith("STAT_")]) == 5
    for n, v in enum.items():
        assert getattr(_capi, n) == int(v), n


def test_layouts_and_sort_bits(native_lib):
    from gaussian_gan_decoder_amd import _capi
    assert C.sizeof(_capi.Params) == 80
    gv = _capi.geom_view(1000)
    assert gv.splat == 0 and gv.tiles_touched >= 48 * 1000 and gv.total == native_lib.ggd_geom_bytes(1000)
    assert gv.point_offsets - gv.tiles_touched >= 4000 and gv.total - gv.clamped >= 1000
    bv = _capi.binning_view(12345)
    assert bv.list == 0 and bv.list_alt >= 4 * 12345 and bv.keys - bv.list_alt >= 4 * 12345
    assert bv.keys_alt - bv.keys >= 8 * 12345 and bv.total == native_lib.ggd_binning_bytes(12345)
    assert _capi.binning_view(99).list == _capi.binning_view(10 ** 7).list == 0   # independent of the laid-out R
    iv = _capi.img_view(100, 52)
    assert iv.final_T - iv.ranges >= 8 * 7 * 4 and iv.total == native_lib.ggd_img_bytes(100, 52)
    for off in (gv.tiles_touched, gv.point_offsets, gv.clamped, bv.list_alt, bv.keys, bv.keys_alt, iv.final_T, iv.n_contrib):
        assert off % 256 == 0
    assert native_lib.ggd_sort_bits(512, 512) == 43 and native_lib.ggd_sort_bits(1024, 1024) == 45
    assert native_lib.ggd_geom_bytes(0) == 0 and native_lib.ggd_binning_bytes(0) == 0


def test_no_device_is_reported_not_crashed(native_lib):
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    assert not native_lib.ggd_create(0)
    assert b"no HIP device" in native_lib.ggd_last_error(None)


def test_rasterizer_argument_checks():
    from gaussian_gan_decoder_amd.rasterizer import GaussianRasterizer, GaussianRasterizationSettings
    z = torch.zeros
    rs = GaussianRasterizationSettings(16, 16, 0.1, 0.1, z(3), 1.0, torch.eye(4), torch.eye(4), 0, z(3), False, False)
    r = GaussianRasterizer(rs)
    m = z(4, 3)
    with pytest.raises(Exception, match="one of either SHs or precomputed colors"):
        r(m, m, z(4, 1), shs=None, colors_precomp=None, scales=z(4, 3), rotations=z(4, 4))
    with pytest.raises(Exception, match="one of either SHs or precomputed colors"):
        r(m, m, z(4, 1), shs=z(4, 1, 3), colors_precomp=z(4, 3), scales=z(4, 3), rotations=z(4, 4))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(m, m, z(4, 1), shs=z(4, 1, 3), scales=z(4, 3), rotations=z(4, 4), cov3D_precomp=z(4, 6))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(m, m, z(4, 1), shs=z(4, 1, 3))
    # CPU tensors are refused loudly: there is no CPU fallback in the product path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r(m, m, z(4, 1), shs=z(4, 1, 3), scales=z(4, 3), rotations=z(4, 4))


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: no file of the product package (or the drop-in shim) may import, dlopen,
    link or execute anything under oracle/.  Plain grep over code lines (comments stripped)."""
    pat = re.compile(r"(\bimport\b.*\boracle\b|\bfrom\s+oracle\b|CDLL\([^)]*oracle|dlopen\([^)]*oracle|"
                     r"#\s*include\s*[<\"][^>\"]*oracle|libggd_oracle|ggd_oracle|\bggo_[a-z_0-9]+\s*\()")
    offenders = []
    for top in ("gaussian_gan_decoder_amd", "diff_gaussian_rasterization", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if not f.endswith((".py", ".hip", ".h", ".inc", ".c", ".cpp")):
                    continue
                for n, line in enumerate(open(os.path.join(dirpath, f)), 1):
                    code = line.split("//")[0] if not f.endswith(".py") else line.split("#")[0]
                    if pat.search(code):
                        offenders.append(f"{os.path.join(dirpath, f)}:{n}: {line.strip()}")
    assert not offenders, "\n".join(offenders)


def test_gaussian_model_getters_and_sh_helpers():
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel, build_covariance_from_scaling_rotation
    from gaussian_gan_decoder_amd import sh
    from oracle import ggd_oracle as O
    g = torch.Generator().manual_seed(0)
    pc = GaussianModel(0)
    pc._xyz = torch.randn(5, 3, generator=g); pc._scaling = torch.randn(5, 3, generator=g)
    pc._rotation = torch.randn(5, 4, generator=g); pc._opacity = torch.randn(5, 1, generator=g)
    pc._features_dc = torch.randn(5, 1, 3, generator=g)
    assert torch.equal(pc.get_scaling, torch.exp(pc._scaling))
    assert torch.equal(pc.get_opacity, torch.sigmoid(pc._opacity))
    assert torch.allclose(pc.get_rotation.norm(dim=1), torch.ones(5))
    assert pc.get_features.shape == (5, 1, 3) and pc.active_sh_degree == 0
    cov = build_covariance_from_scaling_rotation(pc.get_scaling, 1.3, pc.get_rotation)
    for i in range(5):
        ref = O.cov3d(pc.get_scaling[i].numpy(), 1.3, pc.get_rotation[i].numpy())
        assert torch.allclose(cov[i], torch.from_numpy(ref), rtol=1e-4, atol=1e-8)
    assert abs(sh.SH2RGB(sh.RGB2SH(torch.tensor(0.3))).item() - 0.3) < 1e-6


def test_kernel_register_and_lds_budgets(native_lib):
    """The occupancy figures DESIGN.md builds on, read from the code objects inside the built library (no GPU needed;
    scripts/kernel_resources.py): kernels whose inline asm names FIXED physical registers v[248:255] (gt_lin4 in
    ggd_mlp_gelu.inc) must own a 256-VGPR allocation; the forward blend and the sort's finish kernel must keep the
    register / LDS budgets of 8 waves per SIMD and two workgroups per CU; no hot raster kernel may spill."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec); spec.loader.exec_module(kr)
    from gaussian_gan_decoder_amd import _capi
    tab = {kr.short(k): v for k, v in kr.kernel_resources(_capi.LIB_PATH).items()}
    assert len(tab) > 60, "could not read the kernels' metadata out of the library"
    find = lambda prefix: {k: v for k, v in tab.items() if k.startswith(prefix)}
    for name, r in {**find("decoder_forward_hl_kernel"), **find("decoder_backward_hl_kernel")}.items():
        assert r["vgpr"] == 256, f"{name} uses fixed registers v[248:255] but allocates {r['vgpr']} VGPRs"
        assert r["vgpr_spill"] <= 16, (name, r)
    fwd = find("blend_forward_kernel")
    assert fwd and all(r["vgpr"] <= 64 and r["vgpr_spill"] == 0 and r["lds"] <= 4096 for r in fwd.values()), fwd
    fin = find("sort_msd_finish_kernel")
    assert fin and all(r["vgpr"] <= 64 and r["lds"] <= 80 * 1024 + 512 and r["vgpr_spill"] == 0 for r in fin.values()), fin
    for prefix in ("preprocess_kernel", "sort_msd_partition_kernel", "rb_level1_kernel", "rb_scatter2_kernel", "rb_count2_kernel",
                   "rb_scan2_kernel", "blend_backward_quarter_kernel", "blend_backward_tile_kernel", "preprocess_backward_kernel"):
        ks = find(prefix)
        assert ks, prefix
        assert all(r["vgpr_spill"] == 0 and r["scratch"] == 0 for r in ks.values()), (prefix, ks)
