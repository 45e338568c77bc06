"""Normal consistency on the GPU: normals.gaussian_normals (ggd_gaussian_normals / _backward) and normals.fused_normal_loss
(ggd_normal_loss, two launches) against the float64 reference of tests/_normals_ref.py at the bar 1e-5 + K 2^-24 budget, the exact
zeros, determinism, the raw C entry points, the normals through render_simple's feature pass, and one DecoderTrainer step."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import normals as N
import _normals_ref as NR

DEV = torch.device("cuda:0")


def _held(what, got, ref, budget, K, keep=None):
    err = (got.detach().cpu().double() - ref).abs()
    ratio = err / NR.bound(budget, K)
    if keep is not None:
        ratio = ratio[keep]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"  {what}: worst |err| / bound {worst:.3f} (largest |err| {float(err.max()) if err.numel() else 0.0:.3e})")
    assert worst <= 1.0, (what, worst)


# ---- per-Gaussian normals

@pytest.mark.parametrize("raw", (False, True))
@pytest.mark.parametrize("P", NR.NORMAL_CASES)
def test_normals_match_float64(native_lib, P, raw):
    """Forward and J^T g against float64 autograd on every row but the fragile ones (|n_v . p_v| < 1e-4 |p_v|, at most 1 % by the
    host test); scales, means and the view matrix get no gradient."""
    n64, g64, keep, case = NR.normal_reference(P, raw)
    rot, sc, me, V, g = (t.to(DEV) for t in case)
    for t in (rot, sc, me, V):
        t.requires_grad_(True)
    n = N.gaussian_normals(rot, sc, me, V, raw=raw)
    assert n.shape == (P, 3) and n.dtype == torch.float32
    (n * g).sum().backward()
    assert sc.grad is None and me.grad is None and V.grad is None and rot.grad.shape == (P, 4)
    bn, bg = NR.gaussian_normals_budget(*(t.double() for t in case[:4]), raw, case[4].double())
    _held(f"normals P {P} raw {raw}", n, n64, bn.b, NR.K_NORMALS, keep)
    _held(f"dL/drotations P {P} raw {raw}", rot.grad, g64, bg.b, NR.K_NORMALS, keep)
    p_v = (me.detach() @ V.detach()[:3, :3] + V.detach()[3, :3])
    assert float(((n.detach() * p_v).sum(1))[keep.to(DEV)].max()) <= 0.0, "a normal must face the camera"
    # run to run
    n2 = N.gaussian_normals(rot.detach(), sc.detach(), me.detach(), V.detach(), raw=raw)
    assert torch.equal(n2, n.detach())


def test_normals_c_abi(native_lib):
    from gaussian_gan_decoder_amd import _capi
    cx = _capi.context_for(DEV)
    lib = cx.lib
    P = 300
    rot, sc, me, V, g = (t.to(DEV).contiguous() for t in NR.normal_case(P, False))
    GUARD = 777.0
    out, dq = torch.full((3 * P + 64,), GUARD, device=DEV), torch.full((4 * P + 64,), GUARD, device=DEV)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    good = dict(P=P, rot=rot, sc=sc, me=me, V=V, g=g, out=out, dq=dq)

    def fwd(**kw):
        a = dict(good, **kw)
        return lib.ggd_gaussian_normals(cx.handle, None, a["P"], p(a["rot"]), p(a["sc"]), p(a["me"]), p(a["V"]), 0, p(a["out"]))

    def bwd(**kw):
        a = dict(good, **kw)
        return lib.ggd_gaussian_normals_backward(cx.handle, None, a["P"], p(a["rot"]), p(a["sc"]), p(a["me"]), p(a["V"]), 0,
                                                 p(a["g"]), p(a["dq"]))
    odd = torch.zeros(4 * P + 1, device=DEV)[1:]       # 4 bytes past a 16-byte boundary
    for call, who, bad in ((fwd, "ggd_gaussian_normals", [dict(rot=None), dict(sc=None), dict(me=None), dict(V=None),
                                                          dict(out=None), dict(P=-1), dict(rot=odd)]),
                           (bwd, "ggd_gaussian_normals_backward", [dict(rot=None), dict(sc=None), dict(me=None), dict(V=None),
                                                                   dict(g=None), dict(dq=None), dict(P=-1), dict(rot=odd),
                                                                   dict(dq=odd)])):
        for kw in bad:
            rc = call(**kw)
            assert rc != 0, (who, kw)
            with pytest.raises(_capi.RasterError, match=who):
                cx.check(rc)
        cx.check(call(P=0))
    torch.cuda.synchronize()
    assert bool((out == GUARD).all()) and bool((dq == GUARD).all())
    cx.check(fwd()); cx.check(bwd())
    torch.cuda.synchronize()
    assert bool((out[3 * P:] == GUARD).all()) and bool((dq[4 * P:] == GUARD).all())
    assert bool((out[:3 * P] != GUARD).all()) and bool((dq[:4 * P] != GUARD).all())
    assert torch.equal(out[:3 * P].view(P, 3), N.gaussian_normals(rot, sc, me, V))


# ---- the loss

def _loss_run(tag, alpha_min, scale=None):
    W, H = NR.LOSS_CASES[tag]
    scale = float(H * W) if scale is None else scale
    Nr, depth, alpha = (t.to(DEV).requires_grad_(True) for t in NR.loss_case(tag))
    L, Ns = N.fused_normal_loss(Nr, depth[None], alpha, NR.TAN[0], NR.TAN[1], alpha_min)
    assert not Ns.requires_grad and Ns.shape == (3, H, W) and L.shape == ()
    (scale * L).backward()
    return dict(L=L.detach(), Ns=Ns, g_normals=Nr.grad, g_depth=depth.grad, g_alpha=alpha.grad)


def _loss_check(tag, alpha_min):
    got = _loss_run(tag, alpha_min)
    ref, _ = NR.loss_reference(tag, alpha_min)
    bud = NR.loss_budgets(tag, alpha_min)
    print(f"\n  {tag} alpha_min {alpha_min}: L {float(got['L']):.7f} (float64 {float(ref['L']):.7f})")
    for k in ("L", "Ns", "g_normals", "g_depth", "g_alpha"):
        _held(k, got[k], ref[k], bud[k].b, NR.K_LOSS)
    return got, ref


@pytest.mark.parametrize("alpha_min", NR.ALPHA_MINS)
@pytest.mark.parametrize("tag", NR.LOSS_SMALL)
def test_loss_and_gradients_match_float64(native_lib, tag, alpha_min):
    """Term, surface normals and the three gradient maps under (H W * total).backward() -- the gradients of the pixel sum, so that
    the bar's floor of 1e-5 does not swallow them.  The shapes without an interior pixel give zeros throughout."""
    got, ref = _loss_check(tag, alpha_min)
    W, H = NR.LOSS_CASES[tag]
    if W < 3 or H < 3:
        assert all(float(got[k].abs().max()) == 0.0 for k in got)


def test_loss_and_gradients_match_float64_at_the_workload_shape(native_lib):
    _loss_check("512x512", 0.5)


def test_loss_exact_zeros(native_lib):
    """No alpha above the threshold: the term and every gradient are exactly 0.  With the threshold in force, pixels that are not
    valid get exactly 0 in dL/dN_r and N_s, and pixels whose alpha is at or below it exactly 0 in dL/ddepth and dL/dalpha."""
    W, H = NR.LOSS_CASES["65x5"]
    Nr, depth, alpha = (t.to(DEV) for t in NR.loss_case("65x5"))
    low = (alpha * 0.5).requires_grad_(True)       # all <= 0.5
    Nr.requires_grad_(True), depth.requires_grad_(True)
    L, Ns = N.fused_normal_loss(Nr, depth, low, NR.TAN[0], NR.TAN[1], 0.5)
    L.backward()
    for t in (L.detach(), Ns, Nr.grad, depth.grad, low.grad):
        assert bool((t.view(torch.int32) == 0).all())       # +0.0, bit for bit
    got = _loss_run("65x5", 0.5)
    ok = alpha > 0.5
    valid = torch.zeros_like(ok)
    valid[1:-1, 1:-1] = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1]
    assert bool(valid.any()) and bool((~ok).any())
    assert bool((got["Ns"][:, ~valid] == 0).all()) and bool((got["g_normals"][:, ~valid] == 0).all())
    assert bool((got["Ns"][:, valid].norm(dim=0) > 0.999).all())
    assert bool((got["g_depth"][~ok] == 0).all()) and bool((got["g_alpha"][~ok] == 0).all())


def test_plane_and_matching_normals(native_lib):
    """A planar depth map: N_s is the plane's normal within the bar at every interior pixel, and N_r = alpha N_s gives e = 0 within
    the bar of the term."""
    depth64, alpha64, n = NR.plane_case()
    H, W = depth64.shape
    depth, alpha = depth64.float().to(DEV), alpha64.float().to(DEV)
    bud = NR.normal_loss_budget(torch.zeros(3, H, W, dtype=torch.float64), depth.cpu().double(), alpha.cpu().double(), NR.TAN[0],
                                NR.TAN[1], 0.5)
    Ns = N.depth_to_normal(depth, alpha, NR.TAN[0], NR.TAN[1])
    want = torch.zeros(3, H, W, dtype=torch.float64)
    want[:, 1:-1, 1:-1] = n[:, None, None]
    # (the float32 inputs are the plane's depths rounded: the bar is taken around the float64 normals of those inputs)
    ref = NR.normal_loss_ref(torch.zeros(3, H, W, dtype=torch.float64), depth.cpu().double(), alpha.cpu().double(), NR.TAN[0],
                             NR.TAN[1], 0.5)[1]
    _held("plane N_s", Ns, ref, bud["Ns"].b, NR.K_LOSS)
    assert float((ref - want).abs().max()) < 1e-4 and float((Ns.cpu().double() - want).abs().max()) < 1e-4
    L, _ = N.fused_normal_loss(alpha[None] * Ns, depth, alpha, NR.TAN[0], NR.TAN[1], 0.5)
    bud = NR.normal_loss_budget((alpha[None] * Ns).cpu().double(), depth.cpu().double(), alpha.cpu().double(), NR.TAN[0], NR.TAN[1],
                                0.5)
    assert abs(float(L)) <= float(NR.bound(bud["L"].b, NR.K_LOSS)), float(L)


def test_loss_run_to_run_bit_identical(native_lib):
    for tag in ("130x7", "512x512"):
        a, b = _loss_run(tag, 0.5), _loss_run(tag, 0.5)
        for k in a:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (tag, k)


def test_loss_c_abi(native_lib):
    """ggd_normal_loss_tmp_bytes is positive and monotone; NULL, empty and a short tmp return GGD_E_INVALID with a message and write
    nothing; a valid call writes every element of its maps and not one more; surface_normals may be NULL."""
    from gaussian_gan_decoder_amd import _capi
    cx = _capi.context_for(DEV)
    lib = cx.lib
    sizes = [lib.ggd_normal_loss_tmp_bytes(s, s) for s in (1, 33, 64, 65, 512, 1024)]
    assert all(b > 0 for b in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert lib.ggd_normal_loss_tmp_bytes(0, 8) == 0 and lib.ggd_normal_loss_tmp_bytes(8, -1) == 0
    tag = "65x5"
    W, H = NR.LOSS_CASES[tag]
    Nr, depth, alpha = (t.to(DEV) for t in NR.loss_case(tag))
    nbytes = lib.ggd_normal_loss_tmp_bytes(W, H)
    tmp = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    GUARD, PAD = 12345.0, 256
    gn, sn = (torch.full((3 * H * W + PAD,), GUARD, device=DEV) for _ in range(2))
    gd, ga = (torch.full((H * W + PAD,), GUARD, device=DEV) for _ in range(2))
    term = torch.full((1 + PAD,), GUARD, device=DEV)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    good = dict(W=W, H=H, n=Nr, d=depth, a=alpha, am=0.5, term=term, gn=gn, gd=gd, ga=ga, sn=sn, tmp=tmp, nbytes=nbytes)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ggd_normal_loss(cx.handle, None, a["W"], a["H"], p(a["n"]), p(a["d"]), p(a["a"]), NR.TAN[0], NR.TAN[1], a["am"],
                                   p(a["term"]), p(a["gn"]), p(a["gd"]), p(a["ga"]), p(a["sn"]), p(a["tmp"]), a["nbytes"])
    bad = [dict(n=None), dict(d=None), dict(a=None), dict(term=None), dict(gn=None), dict(gd=None), dict(ga=None), dict(tmp=None),
           dict(W=0), dict(H=0), dict(W=-3), dict(nbytes=nbytes - 1), dict(nbytes=0), dict(am=-0.25), dict(am=float("nan"))]
    for kw in bad:
        rc = call(**kw)
        assert rc != 0, kw
        with pytest.raises(_capi.RasterError, match="ggd_normal_loss"):
            cx.check(rc)
    torch.cuda.synchronize()
    for t in (term, gn, gd, ga, sn):
        assert bool((t == GUARD).all())
    cx.check(call())
    torch.cuda.synchronize()
    for t, n in ((term, 1), (gn, 3 * H * W), (sn, 3 * H * W), (gd, H * W), (ga, H * W)):
        assert bool((t[n:] == GUARD).all()) and bool((t[:n] != GUARD).all())
    first = [t.clone() for t in (term, gn, gd, ga)]
    cx.check(call(sn=None))
    torch.cuda.synchronize()
    for t, f in zip((term, gn, gd, ga), first):
        assert torch.equal(t, f)
    L, Ns = N.fused_normal_loss(Nr, depth, alpha, NR.TAN[0], NR.TAN[1], 0.5)
    assert float(L) == float(term[0]) and torch.equal(Ns.reshape(-1), sn[:3 * H * W])


# ---- through the rasterizer

def _scene(P=2000, S=64):
    from gaussian_gan_decoder_amd.synthetic import make_scene
    return make_scene(P, S, "shell", seed=4, log_scale_mean=-4.0).to(DEV)


@pytest.mark.parametrize("fused", (False, True))
def test_through_the_rasterizer(native_lib, fused):
    """render_simple(render_depth_alpha=True, render_normals=True) on 2000 Gaussians at 64 x 64: colour, radii, depth and alpha are
    those of the call without the keyword and out["normals"] is the feature map of gaussian_normals passed by hand, bit for bit;
    with five caller's channels as well, out["features"] is the map of the call without normals, bit for bit, and under
    fused_normal_loss(...)[0].backward() the loss and the gradients that reach the rasterizer's maps (normals, depth, alpha) are
    those of the hand-composed path, bit for bit.
    The leaf gradients behind them cannot be compared bit for bit: the blend backward adds its per-quarter sums to a Gaussian's
    record with float atomics, whose order changes from run to run.  Measured on this scene, six runs of the hand-composed path
    alone: no two agree in any leaf, max |difference| 6.5e-9 (_rotation, max |g| 1.5e-2), 1.1e-8 (_scaling, 8.3e-3), 4.7e-10
    (_opacity, 2.7e-3), 1.5e-8 (_xyz, 2.1e-1).  So the two paths are held to each other as tightly as the hand-composed path is
    to itself: per leaf, max |a - b| <= 4 x the largest difference among three hand-composed runs (and at least 2^-20 of the
    leaf's largest gradient: reordering a float sum of n terms moves it by at most (n - 1) 2^-24 of their magnitudes, and a
    record collects far fewer than 16 quarters here)."""
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    sc = _scene()
    P, S = 2000, 64
    tan = math.tan(sc.cam.FoVx * 0.5)
    attrs = (lambda pc: (pc._rotation, pc._scaling)) if fused else (lambda pc: (pc.get_rotation, pc.get_scaling))
    by_hand = lambda pc: N.gaussian_normals(*attrs(pc), pc.get_xyz, sc.cam.world_view_transform, raw=fused)
    call = lambda pc, **kw: render_simple(sc.cam, pc, bg_color=sc.bg, fused_activations=fused, render_depth_alpha=True, **kw)
    with torch.no_grad():
        pc = sc.gaussian_model()
        plain, out = call(pc), call(pc, render_normals=True)
        assert "normals" not in plain and "features" not in out and out["normals"].shape == (3, S, S)
        for key in ("render", "radii", "depth", "alpha"):
            assert torch.equal(plain[key], out[key]), key
        assert torch.equal(out["normals"], call(pc, features=by_hand(pc))["features"])
        assert float(out["alpha"].max()) > 0.5 and float(out["normals"].abs().max()) > 0.1
    f = torch.rand(P, 5, generator=torch.Generator().manual_seed(9)).to(DEV)
    fbg = torch.tensor([0.1, 0.2, 0.3, 0.4, 0.5], device=DEV)
    leaves = lambda pc: (pc._rotation, pc._scaling, pc._opacity, pc._xyz)

    def grads(composed):
        pc = sc.gaussian_model(requires_grad=True)
        if composed:
            o = call(pc, features=torch.cat([f, by_hand(pc)], 1), feature_bg=torch.cat([fbg, fbg.new_zeros(3)]))
            feats, normals = o["features"][:5], o["features"][5:]
        else:
            o = call(pc, features=f, feature_bg=fbg, render_normals=True)
            feats, normals = o["features"], o["normals"]
        maps = (normals, o["depth"], o["alpha"])
        for m in maps:
            m.retain_grad()
        total = N.fused_normal_loss(*maps, tan, tan)[0]
        total.backward()
        return feats.detach(), normals.detach(), total.detach(), [m.grad for m in maps], [t.grad for t in leaves(pc)]
    fa, na, la, ua, ga = grads(False)
    fb, nb, lb, ub, gb = grads(True)
    others = [grads(True)[-1] for _ in range(2)]
    with torch.no_grad():
        assert torch.equal(fa, call(sc.gaussian_model(), features=f, feature_bg=fbg)["features"])
    assert torch.equal(fa, fb) and torch.equal(na, nb) and torch.equal(la, lb) and float(la) > 0
    for a, b in zip(ua, ub):
        assert float(a.abs().max()) > 0 and torch.equal(a, b)
    for i, name in enumerate(("_rotation", "_scaling", "_opacity", "_xyz")):
        a, hand = ga[i], [gb[i]] + [o[i] for o in others]
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, name
        own = max(float((x - y).abs().max()) for x in hand for y in hand)
        diff = float((a - hand[0]).abs().max())
        print(f"  fused_activations {fused} {name}: max |a - b| {diff:.3e}; hand-composed runs among themselves {own:.3e}")
        assert diff <= max(4.0 * own, 2.0 ** -20 * float(hand[0].abs().max())), (name, diff, own)


def test_one_orientation(native_lib):
    """All splats share one orientation -- the shortest axis 20 degrees off the viewing direction, so that every splat of the shell
    shows the camera the same side: the normal map is alpha times that one normal within 1e-5."""
    from gaussian_gan_decoder_amd.gaussian_renderer import render_simple
    sc = _scene()
    pc = sc.gaussian_model()
    V = sc.cam.world_view_transform
    k = int(V[:3, 2].abs().argmax())                 # the world axis along the view direction
    q = torch.zeros(4, device=DEV)
    q[0], q[1 + (k + 1) % 3] = math.cos(math.radians(10.0)), math.sin(math.radians(10.0))
    log_s = torch.full((3,), -3.5, device=DEV)
    log_s[k] = -4.5
    pc._rotation, pc._scaling = q.expand(2000, 4).contiguous(), log_s.expand(2000, 3).contiguous()
    with torch.no_grad():
        out = render_simple(sc.cam, pc, bg_color=sc.bg, render_depth_alpha=True, render_normals=True)
        n = N.gaussian_normals(pc.get_rotation, pc.get_scaling, pc.get_xyz, V)
    assert bool((n == n[0]).all()) and abs(float(n[0].norm()) - 1.0) < 1e-6 and float(n[0, 2]) < -0.9
    assert float(out["alpha"].max()) > 0.5
    assert float((out["normals"] - out["alpha"] * n[0][:, None, None]).abs().max()) <= 1e-5


# ---- one trainer step

def test_one_trainer_step(native_lib):
    """DecoderTrainer(normal_weight=0.1): a finite loss that differs from the default step's; normal_weight=0 is the trainer built
    without the argument, bit for bit (under an image loss whose sums have one order: the fused one adds with float atomics)."""
    from gaussian_gan_decoder_amd.train import DecoderTrainer, make_scene_batch
    cfg = dict(n_scenes_total=1, plane_res=32, plane_channels=32, hidden_dim=128, image_size=64, seed=7)
    batch = make_scene_batch([0], 2000, 64, DEV, seed=0)
    ordered = lambda image, target, **_: ((image - target).abs().mean() + (image - target).square().mean(), None)

    def step(**extra):
        tr = DecoderTrainer(DEV, loss_fn=ordered, **cfg, **extra)
        with torch.no_grad():   # splats of about a pixel (the scale head is -softplus(s + 5) - 2.5: a smaller bias is a larger splat),
            tr.decoder.scale_decoder.backbone[-1].bias -= 3.0     # so that alpha > 0.5 on whole neighbourhoods: on the CPU oracle 3590
            tr.decoder.opacity_decoder.backbone[-1].bias += 1.0   # of the 3844 interior pixels are valid (none at the initial bias)
        tr.flat_grad.zero_()
        loss = tr.local_loss(batch)
        loss.backward()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(tr.flat_grad).all())
        return float(loss.detach())
    plain, zero, on = step(), step(normal_weight=0.0), step(normal_weight=0.1)
    print(f"\n  loss: default {plain:.8f}, normal_weight 0 {zero:.8f}, normal_weight 0.1 {on:.8f}")
    assert zero == plain
    assert math.isfinite(on) and abs(on - plain) > 1e-6 * abs(plain)
