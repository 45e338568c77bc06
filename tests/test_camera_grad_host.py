"""The camera-gradient extension without a GPU: the settings keyword and its refusal, the float64 reference
(tests/_camera_grad_ref.py) against central differences of the float64 oracle, the entries no kernel reads, and the share of the
budget the reference's float32 twin uses (the K of the GPU tests)."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import _camera_grad_ref as CR
from _util import fragile_pixels, run_oracle, scene_inputs
from oracle import ggd_oracle as O
from gaussian_gan_decoder_amd.synthetic import make_dL_dpix


def _settings(**kw):
    from gaussian_gan_decoder_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                         False, False, **kw)


def test_settings_keyword():
    rs = _settings()
    assert rs.camera_grad is False and "camera_grad" not in repr(rs) and len(rs) == 14
    rs = _settings(camera_grad=True)
    assert rs.camera_grad is True and "camera_grad=True" in repr(rs) and len(rs) == 14
    assert rs._replace(sh_degree=2).camera_grad is True
    assert rs._replace(camera_grad=False).camera_grad is False
    assert _settings(antialiasing=True)._replace(camera_grad=True).antialiasing is True
    with pytest.raises(TypeError):
        _settings(True, camera_grad=True)[14]   # keyword only: not a tuple field


def test_absgrad_is_refused_before_any_device_call():
    from gaussian_gan_decoder_amd import rasterizer as R
    from gaussian_gan_decoder_amd.gaussian_renderer import _settings as renderer_settings
    rs = _settings(camera_grad=True, absgrad=True)
    e = torch.empty(0)
    with pytest.raises(ValueError, match="camera_grad"):
        R.rasterize_gaussians(torch.zeros(4, 3), torch.zeros(4, 3), e, torch.zeros(4, 3), torch.ones(4), torch.ones(4, 3),
                              torch.ones(4, 4), e, rs)
    with pytest.raises(ValueError, match="camera_grad"):
        R.rasterize_gaussians_backward_native(*([None] * 21), absgrad=True, camera_grad=True)

    class Cam: image_height = image_width = 8; FoVx = FoVy = 0.5; world_view_transform = full_proj_transform = torch.eye(4); camera_center = torch.zeros(3)
    class Pc: active_sh_degree = 0
    with pytest.raises(ValueError, match="camera_grad"):
        renderer_settings(Cam, Pc, torch.zeros(3), 1.0, False, absgrad=True, camera_grad=True)
    assert renderer_settings(Cam, Pc, torch.zeros(3), 1.0, False, camera_grad=True).camera_grad is True


def _analytic64(d, g):
    f = run_oracle(d, dtype=np.float64)
    b = O.backward(f, g)
    P = d["P"]
    t, ncl = CR.terms(f, b["dL_dconic"], b["dL_dmeans2D"], b["dL_dcolors"], None)
    return f, t.sum(0), ncl


def test_reference_against_central_differences():
    """d sum(dL_dpix colour) / d (viewmatrix, projmatrix, campos) in float64 through the oracle, SH degree 2, no clamped Gaussian
    (so that the published convention equals the derivative); step, tolerance and discontinuity cap of test_oracle_properties"""
    d = scene_inputs(P=400, size=48, kind="shell", lsm=-4.5, seed=3, sh_degree=2)
    g = make_dL_dpix(48)[:, :d["H"], :d["W"]].double().numpy()
    f, an, ncl = _analytic64(d, g)
    assert ncl == 0 and int((f["radii"] > 0).sum()) > 100
    loss = lambda ff: float((ff["color"] * g).sum())
    rng = np.random.default_rng(0)
    for inp, off, entries in (("viewmatrix", 0, [k for k in range(16) if k not in CR.UNREAD]),
                              ("projmatrix", 16, [k for k in range(16) if 16 + k not in CR.UNREAD]), ("campos", 32, [0, 1, 2])):
        base = d[inp].double().numpy().reshape(-1)
        picks = list(rng.choice(entries, size=min(8, len(entries)), replace=False))
        checked = 0
        for k in picks:
            def central(eps):
                vals = []
                for sgn in (+1, -1):
                    pert = base.copy(); pert[k] += sgn * eps
                    d2 = dict(d); d2[inp] = torch.from_numpy(pert.reshape(tuple(d[inp].shape)))
                    vals.append(loss(run_oracle(d2, dtype=np.float64)))
                return (vals[0] - vals[1]) / (2 * eps)
            fd, fd2 = central(1e-7), central(1e-7 / 4)
            if abs(fd - fd2) > 1e-3 * max(abs(fd), abs(fd2), 1e-6):
                continue   # a jump (alpha / T / radius threshold) sits inside +-eps
            checked += 1
            a = an[off + k]
            print(f"[camera_grad] {inp}[{k}]: finite difference {fd2:.6e}, reference {a:.6e}")
            assert abs(fd2 - a) <= 5e-4 * max(abs(fd2), abs(a)) + 1e-5, f"{inp}[{k}]: finite difference {fd2} vs reference {a}"
        assert checked >= (len(picks) + 1) // 2, f"{inp}: too many finite-difference samples hit a discontinuity"


def test_unread_entries_are_exactly_zero_and_colors_precomp_has_no_campos_gradient():
    for name in ("sh3", "colors"):
        d = CR.SCENES[name]()
        o = run_oracle(d)
        g = make_dL_dpix(max(d["W"], d["H"]))[:, :d["H"], :d["W"]].numpy()
        ref, bud, _ = O.backward_ref64(o, g)
        val, b, car, _ = CR.reference(o, ref, bud)
        assert (val[CR.UNREAD] == 0).all() and (b[CR.UNREAD] == 0).all() and (car[CR.UNREAD] == 0).all()
        assert np.abs(val[:16]).max() > 0 and np.abs(val[16:32]).max() > 0
        assert (np.abs(val[32:]).max() > 0) == (name == "sh3")
        if name == "colors":
            assert (val[32:] == 0).all()


def test_scenes_have_no_gaussian_on_the_alpha_floor_and_measured_share():
    """Every GPU scene: the reference flags no Gaussian on the alpha floor (a sum cannot leave one out); the float32 twin's share of
    the budget is recomputed, printed, and must not exceed MEASURED_SHARE (K = ceil(4 MEASURED_SHARE))."""
    worst = 0.0
    for name, make in CR.SCENES.items():
        d = make()
        o = run_oracle(d)
        frag_px = fragile_pixels(o)
        g = make_dL_dpix(max(d["W"], d["H"]))[:, :d["H"], :d["W"]].clone()
        g[:, torch.from_numpy(frag_px)] = 0.0
        ref, bud, frag = O.backward_ref64(o, g.numpy())
        assert int((frag > 0).sum()) == 0, f"{name}: {int((frag > 0).sum())} Gaussians on the alpha floor"
        sh = CR.share(o, ref, bud)
        print(f"[camera_grad] {name}: visible {int((o['radii'] > 0).sum())}, float32 twin uses {sh:.3f} of the budget")
        worst = max(worst, sh)
    # the instances that read more of the record: the antialiasing h chain (opacity slot) and the depth slot
    import _antialias_ref as AA
    d = CR.SCENES[CR.INSTANCE_SCENE]()
    g = make_dL_dpix(max(d["W"], d["H"]))[:, :d["H"], :d["W"]].clone()
    d_o = dict(d, opacities=torch.from_numpy(AA.o_eff(d).astype(np.float32)).reshape(d["opacities"].shape))
    o = run_oracle(d_o)
    ref, bud, frag = O.backward_ref64(o, g.numpy())
    sh = CR.share(o, ref, bud, aa_opacity=d["opacities"].numpy())
    print(f"[camera_grad] antialiasing: float32 twin uses {sh:.3f} of the budget")
    worst = max(worst, sh)
    o = run_oracle(d)
    ref, bud, frag = O.backward_ref64(o, g.numpy())
    gz, gzb = CR.depth_slot(o, g.numpy()[0], g.numpy()[1])
    sh = CR.share(o, ref, bud, gz, gzb)
    print(f"[camera_grad] depth slot: float32 twin uses {sh:.3f} of the budget")
    worst = max(worst, sh)
    print(f"[camera_grad] largest share {worst:.3f} (MEASURED_SHARE = {CR.MEASURED_SHARE}, K = {CR.K})")
    assert worst <= CR.MEASURED_SHARE and CR.K == math.ceil(4 * CR.MEASURED_SHARE)
