"""Normal consistency, host side (no GPU): the declarations, the reference of tests/_normals_ref.py on its hand-checkable cases, its
closed form and budgets against autograd, the float32 twin's share of the budgets (what K of the GPU tests is four times of), the
package's torch forms against the reference, and the refusals of render / render_simple / DecoderTrainer."""
import inspect
import math
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import normals as N
import _normals_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ggd_gaussian_normals", "ggd_gaussian_normals_backward", "ggd_normal_loss_tmp_bytes", "ggd_normal_loss")


def test_declarations():
    from gaussian_gan_decoder_amd import _capi, build, gaussian_renderer as GR, rasterizer as R, train as T
    header = open(os.path.join(ROOT, "include", "ggd_raster.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b" + sym + r"\(", header), sym
        assert sym in _capi.EXPORTS, sym
    assert "ggd_normals.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ggd_normals.hip"))
    for fn in (GR.render, GR.render_simple):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "render_normals" and params[-1].default is False, fn
    assert inspect.signature(T.DecoderTrainer.__init__).parameters["normal_weight"].default == 0.0
    for fn in (R.rasterize_gaussians, R.GaussianRasterizer.forward, R.rasterize_gaussians_native):
        assert "render_normals" not in inspect.signature(fn).parameters, fn
    assert inspect.signature(N.fused_normal_loss).parameters["alpha_min"].default == 0.5
    assert "untuned placeholder" in " ".join(N.fused_normal_loss.__doc__.split())


# ---- hand-checkable cases, on the reference and on the package's torch forms (CPU tensors take those)

def _view(tz):
    V = torch.eye(4, dtype=torch.float64)
    V[3, 2] = tz
    return V


@pytest.mark.parametrize("fn", (lambda *a: NR.gaussian_normals_ref(*a)[0], N.gaussian_normals, N.gaussian_normals_torch))
def test_normals_by_hand(fn):
    ident = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    mean = torch.zeros(1, 3, dtype=torch.float64)
    s321 = torch.tensor([[3.0, 2.0, 1.0]], dtype=torch.float64)
    # the shortest axis is e_z; the Gaussian in front of the camera (p_v.z = +2) shows it -e_z, behind it (p_v.z = -2) +e_z
    assert torch.equal(fn(ident, s321, mean, _view(2.0), False), torch.tensor([[0.0, 0.0, -1.0]], dtype=torch.float64))
    assert torch.equal(fn(ident, s321, mean, _view(-2.0), False), torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64))
    # equal scales: axis 0; ties in a pair: the lower index
    off = torch.tensor([[1.0, 0.5, 2.0]], dtype=torch.float64)
    for s, axis in (([1, 1, 1], 0), ([2, 1, 1], 1), ([1, 2, 1], 0), ([1, 1, 2], 0), ([2, 2, 1], 2)):
        n = fn(ident, torch.tensor([s], dtype=torch.float64), off, _view(0.0), False)
        want = torch.zeros(1, 3, dtype=torch.float64)
        want[0, axis] = -1.0          # off has positive coordinates: every axis is flipped
        assert torch.equal(n, want), (s, n)
    # raw: the quaternion is normalised, a zero quaternion gives R = I, log-scales have the same argmin
    q = torch.tensor([[3.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    n = fn(q, torch.tensor([[3.0, 2.0, 1.0], [-1.0, -2.0, -3.0]], dtype=torch.float64), mean.expand(2, 3), _view(2.0), True)
    assert torch.equal(n, torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0]], dtype=torch.float64))
    # without raw the quaternion is used as given: column 0 of R(0, 0, 2, 0) is (1 - 2 y^2, 0, 0) = (-7, 0, 0), and it faces the
    # camera as it is (n_v . p_v = -7)
    n = fn(torch.tensor([[0.0, 0.0, 2.0, 0.0]], dtype=torch.float64), torch.tensor([[1.0, 2.0, 3.0]], dtype=torch.float64), off,
           _view(0.0), False)
    assert torch.equal(n, torch.tensor([[-7.0, 0.0, 0.0]], dtype=torch.float64))


@pytest.mark.parametrize("fn", (lambda *a: NR.normal_loss_ref(*a)[:2], N.normal_loss_torch, N.fused_normal_loss))
def test_plane_by_hand(fn):
    depth, alpha, n = NR.plane_case()
    H, W = depth.shape
    zeros = torch.zeros(3, H, W, dtype=torch.float64)
    L, Ns = fn(zeros, depth, alpha, NR.TAN[0], NR.TAN[1], 0.5)
    inner = Ns[:, 1:-1, 1:-1]
    assert float((inner - n[:, None, None]).abs().max()) < 1e-12
    assert float(Ns[:, 0].abs().max()) == 0 and float(Ns[:, :, 0].abs().max()) == 0 and float(Ns[:, -1].abs().max()) == 0
    assert abs(float(L) - 0.75 * (H - 2) * (W - 2) / (H * W)) < 1e-12         # N_r = 0: e = alpha
    L0, _ = fn(alpha[None] * Ns, depth, alpha, NR.TAN[0], NR.TAN[1], 0.5)     # N_r = alpha N_s: e = 0
    assert abs(float(L0)) < 1e-15
    if fn is N.normal_loss_torch:
        assert torch.equal(N.depth_to_normal(depth[None], alpha[None], NR.TAN[0], NR.TAN[1]), Ns)
    # a fronto-parallel plane: (0, 0, -1)
    flat = torch.full((5, 7), 1.5, dtype=torch.float64)
    _, Ns = fn(torch.zeros(3, 5, 7, dtype=torch.float64), flat * 0.75, torch.full_like(flat, 0.75), 0.3, 0.2, 0.5)
    assert float((Ns[:, 1:-1, 1:-1] - torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)[:, None, None]).abs().max()) < 1e-12
    # no alpha above the threshold: nothing at all
    L, Ns = fn(zeros + 1.0, depth, alpha * 0 + 0.5, NR.TAN[0], NR.TAN[1], 0.5)
    assert float(L) == 0.0 and float(Ns.abs().max()) == 0.0


# ---- closed form, budgets and the float32 twin

def test_normal_cases_closed_form_and_twin_share():
    """The fixed seeds leave out at most 1 % of the rows as fragile (float64 alone decides); the closed form the budgets ride on is
    autograd's gradient; the float32 twin stays within TWIN_SHARE_NORMALS of the budget."""
    worst = 0.0
    for P in NR.NORMAL_CASES:
        for raw in (False, True):
            n64, g64, keep, case = NR.normal_reference(P, raw)
            assert int((~keep).sum()) <= P // 100, (P, raw, int((~keep).sum()))
            rot, sc, me, V, g = (t.double() for t in case)
            if P >= 63:
                assert sc[0, 0] == sc[0, 1] < sc[0, 2] and sc[1, 0] == sc[1, 2] < sc[1, 1] and sc[2, 1] == sc[2, 2] < sc[2, 0]
                assert sc[3, 0] == sc[3, 1] == sc[3, 2] and sc[4, 0] == sc[4, 1] > sc[4, 2]
                assert float(rot[7].abs().max()) == 0 and float((me[8:11] @ V[:3, :3] + V[3, :3])[:, 2].max()) < 0
                assert abs(float(rot[5].norm()) - 3.4) < 1e-5
            bn, bg = NR.gaussian_normals_budget(rot, sc, me, V, raw, g)
            assert float((bn.v - n64)[keep].abs().max()) < 1e-12
            assert float(((bg.v - g64)[keep].abs() / (1 + g64[keep].abs())).max()) < 1e-12
            n32, g32, keep32, _ = NR.normal_reference(P, raw, torch.float32)
            s = max(NR.share(n32[keep], n64[keep], bn.b[keep]), NR.share(g32[keep], g64[keep], bg.b[keep]))
            print(f"  P {P} raw {raw}: {int((~keep).sum())} left out, twin share {s:.3f}")
            worst = max(worst, s)
    print(f"  largest twin share {worst:.3f}; K = {NR.K_NORMALS}")
    assert worst <= NR.TWIN_SHARE_NORMALS


def test_loss_cases_closed_form_and_twin_share():
    worst = 0.0
    for tag, (W, H) in NR.LOSS_CASES.items():
        for am in NR.ALPHA_MINS:
            ref, case = NR.loss_reference(tag, am)
            twin, _ = NR.loss_reference(tag, am, torch.float32)
            bud = NR.loss_budgets(tag, am)
            if H < 3 or W < 3:
                assert all(float(ref[k].abs().max()) == 0 for k in ref)
            elif am == 0.0:
                assert float(ref["L"]) > 0 and float(ref["g_depth"].abs().max()) > 0
            alpha = case[2]
            assert bool((alpha > 0.5).any()) or H * W < 4
            assert bool((alpha <= 0.5).any()) or H * W < 4
            shares = {}
            for k in ref:
                assert float((bud[k].v - ref[k]).abs().max()) <= 1e-9 * (1e-30 + float(ref[k].abs().max())), (tag, k)
                shares[k] = NR.share(twin[k].reshape(-1), ref[k].reshape(-1), bud[k].b.reshape(-1))
            print(f"  {tag} alpha_min {am}: L {float(ref['L']):.6f}, twin shares " + " ".join(f"{k} {v:.3f}" for k, v in shares.items()))
            worst = max(worst, *shares.values())
    print(f"  largest twin share {worst:.3f}; K = {NR.K_LOSS}")
    assert worst <= NR.TWIN_SHARE_LOSS


def test_package_torch_forms_are_the_reference():
    for raw in (False, True):
        n64, g64, keep, case = NR.normal_reference(257, raw)
        rot, sc, me, V, g = (t.double() for t in case)
        rot.requires_grad_(True), sc.requires_grad_(True), me.requires_grad_(True), V.requires_grad_(True)
        n = N.gaussian_normals(rot, sc, me, V, raw=raw)
        (n * g).sum().backward()
        assert float((n.detach() - n64).abs().max()) < 1e-12 and float(((rot.grad - g64).abs() / (1 + g64.abs())).max()) < 1e-12
        assert sc.grad is None and me.grad is None and V.grad is None
    for tag in ("3x3", "65x5", "2x2"):
        ref, case = NR.loss_reference(tag, 0.0, scale=1.0)
        Nr, depth, alpha = (t.double().requires_grad_(True) for t in case)
        L, Ns = N.fused_normal_loss(Nr, depth[None], alpha[None], NR.TAN[0], NR.TAN[1], 0.0)
        L.backward()
        assert abs(float(L.detach()) - float(ref["L"])) < 1e-14 and float((Ns - ref["Ns"]).abs().max()) < 1e-14 and not Ns.requires_grad
        for t, k in ((Nr, "g_normals"), (depth, "g_depth"), (alpha, "g_alpha")):
            got = torch.zeros_like(t) if t.grad is None else t.grad
            assert float((got - ref[k]).abs().max()) <= 1e-12 * (1 + float(ref[k].abs().max())), (tag, k)


def test_argument_checks():
    z = torch.zeros
    with pytest.raises(ValueError):
        N.gaussian_normals(z(4, 3), z(4, 3), z(4, 3), z(4, 4))
    with pytest.raises(ValueError):
        N.gaussian_normals(z(4, 4), z(4, 3), z(4, 3), z(3, 4))
    with pytest.raises(TypeError):
        N.gaussian_normals(z(4, 4), z(4, 3).double(), z(4, 3), z(4, 4))
    for fn in (N.fused_normal_loss, N.normal_loss_torch):
        with pytest.raises(ValueError):
            fn(z(3, 4, 5), z(4, 6), z(4, 5), 0.2, 0.2)
        with pytest.raises(ValueError):
            fn(z(2, 4, 5), z(4, 5), z(4, 5), 0.2, 0.2)
        with pytest.raises(ValueError):
            fn(z(3, 4, 5), z(4, 5), z(4, 5), 0.0, 0.2)
        with pytest.raises(ValueError):
            fn(z(3, 4, 5), z(4, 5), z(4, 5), 0.2, 0.2, alpha_min=-0.1)
        with pytest.raises(TypeError):
            fn(z(3, 4, 5), z(4, 5).double(), z(4, 5), 0.2, 0.2)


# ---- refusals, before any device call

@pytest.fixture
def no_native(monkeypatch):
    from gaussian_gan_decoder_amd import _capi

    def refuse(*a, **k):
        raise AssertionError("a refused call must not reach the library")
    monkeypatch.setattr(_capi, "load", refuse)
    monkeypatch.setattr(_capi, "context_for", refuse)
    monkeypatch.setattr(_capi, "context_and_stream", refuse)


def test_render_refusals(no_native):
    """Each refusal is a ValueError raised before the model, the camera or the library is touched (all three are None here)."""
    from types import SimpleNamespace
    from gaussian_gan_decoder_amd import gaussian_renderer as GR
    pipe = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    for call in (lambda **kw: GR.render(None, None, pipe, None, render_normals=True, **kw),
                 lambda **kw: GR.render_simple(None, None, None, render_normals=True, **kw)):
        with pytest.raises(ValueError, match="absgrad"):
            call(absgrad=True)
        with pytest.raises(ValueError, match="camera_grad"):
            call(camera_grad=True)
        with pytest.raises(ValueError, match="at most 32"):
            call(features=torch.zeros(5, 30))
        with pytest.raises(ValueError, match="feature_bg without features"):
            call(feature_bg=torch.zeros(3))
    with pytest.raises(ValueError, match="compute_cov3D_python"):
        GR.render(None, None, SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=False), None,
                  render_normals=True)
    # 29 caller's channels are the most that fit: the refusal is not reached, the (absent) model is
    with pytest.raises(AttributeError):
        GR.render_simple(None, None, None, render_normals=True, features=torch.zeros(5, 29))


def test_trainer_normal_weight():
    """normal_weight = 0 (the default) leaves render_fn's keywords what they were; a positive weight adds the two keywords and
    nothing else; a negative one is refused."""
    from gaussian_gan_decoder_amd.train import DecoderTrainer

    def fake_render(cam, gs, bg_color, **kw):
        raise RuntimeError("stop")
    mk = lambda **kw: DecoderTrainer("cpu", 1, plane_res=8, plane_channels=4, hidden_dim=8, image_size=8, render_fn=fake_render, **kw)
    assert mk().render_kwargs == {} and mk().normal_weight == 0.0
    assert mk(normal_weight=0.0, antialiasing=True).render_kwargs == {"antialiasing": True}
    assert mk(normal_weight=0.1).render_kwargs == {"render_depth_alpha": True, "render_normals": True}
    assert mk(normal_weight=0.1, distortion_weight=0.5).render_kwargs == {"render_depth_alpha": True, "render_distortion": True,
                                                                           "render_normals": True}
    with pytest.raises(ValueError):
        mk(normal_weight=-0.1)
    assert math.isfinite(mk(normal_weight=0.1).normal_weight)
