"""Every kernel instance with a `raw_attributes` branch against float64, from the case tables of tests/_raw_cases.py
(tests/test_raw_cases_host.py shows that they reach each instance, that the reference alone meets every cap with half of it to
spare, and where the constants of the bars come from).

The kernels take log-scales, unnormalised quaternions and logits.  The reference applies exp, x / max(||x||, 1e-12) and sigmoid in
float64, rounds once to float32, runs the CPU oracle on that, and takes the float64 gradients with respect to the activated
attributes through the three Jacobians in float64 (tests/_raw_ref.py).  Per element, with no array-scale term:

    |gpu - ref2| <= 1e-5 + KAPPA_RAW 2^-24 bud2

Each case renders two frames (the exact two-call path, then the single call: preprocess_kernel unfolded and folded), checks the integer
stages bit for bit, the per-Gaussian records at their own bar, colour (depth, alpha) at 1e-5, and one backward with NaN-poisoned
outputs.  Each test prints its measured figures before it asserts."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _instance_cases as IC
import _normals_ref as NR
import _raw_cases as RC
import _raw_ref as RR
from _util import ATOL, EPS32, assert_blend_matches, check_gradients, decode_result, same_frame
from test_absgrad_gpu import _backward
from test_antialiasing_gpu import _native
from test_instances_gpu import FRAMES, _check_aux_forward, _forget_shape, _options

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _check_integer_stages(n, o, what):
    assert n["num_rendered"] == o["num_rendered"], what
    np.testing.assert_array_equal(n["radii"].cpu().numpy(), o["radii"], err_msg=what)
    np.testing.assert_array_equal(n["point_list"], o["point_list"], err_msg=what)
    np.testing.assert_array_equal(n["ranges"], o["ranges"], err_msg=what)


def _check_records(case, n, what):
    """the per-Gaussian records of a raw forward against the float64-activated oracle's: centre, colour and depth pass no
    activation and are the oracle's bit for bit; the conic and the opacity lie within four times the float32 twins' largest
    deviation (with anti-aliasing the record holds o h: plus 16 cond 2^-24, the bound of the float32 h in
    tests/test_antialiasing_gpu.py::_check_record_opacity)"""
    r = RC.reference(case)
    o = r["o"]
    vis = o["radii"] > 0
    for k in ("xy", "rgb", "depths"):
        np.testing.assert_array_equal(n[k][vis], o[k][vis], err_msg=f"{what}: {k}")
    c, cn = o["conic_opacity"][vis].astype(np.float64), n["conic_opacity"][vis].astype(np.float64)
    dev_c = float((np.abs(cn[:, :3] - c[:, :3]).max(1) / (EPS32 * np.abs(c[:, :3]).max(1))).max(initial=0.0))
    units_o = np.full(c.shape[0], RC.OPACITY_UNITS)
    if RC.has_aa(case):
        import _antialias_ref as AA
        units_o = units_o + 16.0 * AA.h_and_conditioning(r["act"])[1][vis]
    dev_o = float((np.abs(cn[:, 3] - c[:, 3]) / (EPS32 * units_o * np.maximum(c[:, 3], 1e-300))).max(initial=0.0))
    print(f"[raw] {what}: conic off by {dev_c:.1f} units of 2^-24 of the row's largest entry (bar {RC.CONIC_UNITS:.0f}), opacity at "
          f"{dev_o:.3f} of its bar")
    assert dev_c <= RC.CONIC_UNITS, what
    assert dev_o <= 1.0, what


def _forward(case):
    """two frames of a case under its options: (result of the last, decoded, fragile-pixel mask)"""
    r = RC.reference(case)
    raw, o = r["raw"], r["o"]
    aa, aux = RC.has_aa(case), RC.has_aux(case)
    with _options(case["options"]) as ctx:
        _forget_shape(ctx, raw)
        frames = []
        for frame in FRAMES:
            what = f"{case['id']} ({frame})"
            res = _native(raw, aa=aa, raw=True, aux=aux)
            frames.append(res)
            n = decode_result(raw, res)
            _check_integer_stages(n, o, what)
            _check_records(case, n, what)
            frag_px, err = assert_blend_matches(n, o, window=IC.RAW_WINDOW, what=what)
            assert not (frag_px & ~r["frag"]).any()
            print(f"[raw] {what}: max |dRGB| {err:.2e} outside {int(frag_px.sum())} fragile pixels")
            if aux:
                _check_aux_forward(o, res, ~frag_px, what)
                if frame == FRAMES[0]:
                    _forget_shape(ctx, raw)
                assert same_frame(_native(raw, aa=aa, raw=True, aux=False), res[:6]), f"{what}: the depth / alpha maps moved the frame"
        assert same_frame(frames[0][:6], frames[1][:6]), f"{case['id']}: the two paths differ"
        if aux:
            assert torch.equal(frames[0][6], frames[1][6]) and torch.equal(frames[0][7], frames[1][7]), case["id"]
    return res, n, frag_px


def _run(case):
    r = RC.reference(case)
    raw = r["raw"]
    aa, aux, ab = RC.has_aa(case), RC.has_aux(case), case["absgrad"]
    res, n, frag_px = _forward(case)
    g, gD, gA = IC.upstream_gradients(raw["H"], raw["W"], frag_px)
    ref = RR.reference(raw, r["act"], r["o"], case["feature"], g.numpy(), gD.numpy(), gA.numpy(), n=n, absgrad=ab, kappa=RC.KAPPA_RAW)
    with _options(case["options"]):
        got = _backward(raw, n, g, gD if aux else None, gA if aux else None, raw=True, aa=aa, absgrad=ab)   # (NaN-fills first)
    report = []
    worst = check_gradients(raw, got, ref["ref2"], ref["bud2"], ref["frag"], kappa=RC.KAPPA_RAW, report=report)
    print(f"[raw] {case['id']} ({RC.preprocess_backward_instance(case)}): worst error / bound {worst:.3f}; "
          + ", ".join(f"{x['array']} {x['worst_ratio']:.3f}" for x in report))
    assert worst <= 1.0, report
    if ab:
        assert (got["dL_dmeans2D_abs"] >= 0).all() and (got["dL_dmeans2D_abs"][:, 2] == 0).all()
    return got, ref


@pytest.mark.parametrize("case", RC.TABLE_R, ids=[c["id"] for c in RC.TABLE_R])
def test_per_gaussian_kernel_form(native_lib, case):
    _run(case)


@pytest.mark.parametrize("case", RC.TABLE_S, ids=[c["id"] for c in RC.TABLE_S])
def test_absgrad_kernel_form(native_lib, case):
    _run(case)


@pytest.mark.parametrize("case", RC.TABLE_E, ids=[c["id"] for c in RC.TABLE_E])
def test_edge_activations(native_lib, case):
    """the rows set by hand (tests/_raw_cases.py::EDGE_ROWS) are held like every other row -- the zero quaternion and the rows under
    the clamp too, whose bound scales with their budget (dL_drots of the order 1e12 |g|) -- and a row under 1 / 255 has gradients of
    exactly 0"""
    got, ref = _run(case)
    rows = RC.edge_rows(case)
    assert not (ref["frag"][rows] > 0).any(), "a row set by hand must not be left out as fragile"
    P = RC.reference(case)["raw"]["P"]
    for k, v in got.items():
        if v.size:
            assert (v.reshape(P, -1)[rows[list(RC.UNDER_FLOOR_ROWS)]] == 0).all(), k
    for j in RC.UNDER_CLAMP_ROWS:
        a, b = got["dL_drots"].reshape(-1, 4)[rows[j]], ref["ref2"]["dL_drots"][rows[j]]
        print(f"[raw] {case['id']}: row under the clamp: dL_drots {a} against {b}")
    assert got["dL_dopacity"].reshape(-1)[rows[11]] == 0, "1 / (1 + expf(-17)) is 1: the derivative is exactly 0"


@pytest.mark.parametrize("case", RC.TABLE_V, ids=[c["id"] for c in RC.TABLE_V])
def test_camera_gradients(native_lib, case):
    """camera_partial_kernel<AA, AUX> with raw = 1: the 35 values at K_RAW, the entries no kernel reads exactly 0, and the
    translation identity of tests/test_camera_grad_gpu.py on the same call's dL_dmeans3D"""
    import test_camera_grad_gpu as CG
    r = RC.reference(case)
    raw, o = r["raw"], r["o"]
    aa, aux = RC.has_aa(case), RC.has_aux(case)
    what = case["id"]
    res = CG._forward(raw, raw=True, antialiasing=aa, render_depth_alpha=aux)
    n = decode_result(raw, res)
    _check_integer_stages(n, o, what)
    _check_records(case, n, what)
    frag_px, _ = assert_blend_matches(n, o, window=IC.RAW_WINDOW, what=what)
    g, gD, gA = IC.upstream_gradients(raw["H"], raw["W"], frag_px)
    ref = RR.reference(raw, r["act"], o, case["feature"], g.numpy(), gD.numpy(), gA.numpy(), n=n, kappa=RC.KAPPA_RAW)
    assert int((ref["frag"] > 0).sum()) == 0, "a sum cannot leave a Gaussian on the alpha floor out"
    cam = RR.camera_reference(r["act"], o, case["feature"], ref["blend"], gD.numpy(), gA.numpy(), n=n)
    kw = dict(dL_ddepth=gD, dL_dalpha=gA) if aux else {}
    outs = CG._backward(raw, res, g, raw=True, aa=aa, **kw)
    assert len(outs) == 11
    report = []
    worst8 = check_gradients(raw, dict(zip(CG.NAMES, outs)), ref["ref2"], ref["bud2"], ref["frag"], kappa=RC.KAPPA_RAW, report=report)
    v = CG._identity(raw, outs, what)      # (asserts the unread entries exactly 0 and every value written)
    tol = ATOL + cam["car"] + RC.K_RAW * EPS32 * cam["bud"]
    ratio = np.abs(v - cam["val"]) / tol
    k = int(ratio.argmax())
    print(f"[raw] {what} ({RC.camera_instance(case)}): eight gradients error / bound {worst8:.3f}; camera: worst error / bound "
          f"{ratio.max():.4f} at entry {k} (gpu {v[k]:.6e}, ref {cam['val'][k]:.6e}, budget {cam['bud'][k]:.3e})")
    assert worst8 <= 1.0, report
    assert ratio.max() <= 1.0, what
    assert np.abs(cam["val"][:12]).max() > 0 and np.abs(cam["val"][16:28]).max() > 0 and np.abs(cam["val"][32:]).max() > 0


def test_normals_under_the_clamp(native_lib):
    """normals.gaussian_normals(raw=True), forward and backward, on the 64 rows of tests/_normals_ref.py::normal_case with two rows
    under the clamp of the normalisation, against float64 autograd (whose gradient there is g / eps, with no projection) at that
    file's bar"""
    from gaussian_gan_decoder_amd import normals as N
    P = 64
    rot, sc, me, V, g = (t.clone() for t in NR.normal_case(P, True))
    rot[13] = torch.tensor(RC.UNDER)
    rot[14] = torch.tensor([0.0, 0.0, -5e-13, 2e-13])
    r64 = rot.double().requires_grad_(True)
    n64, facing, plen = NR.gaussian_normals_ref(r64, sc.double(), me.double(), V.double(), True)
    (n64 * g.double()).sum().backward()
    keep = (facing.abs() >= NR.FRAGILE * plen).detach()
    assert bool(keep[13]) and bool(keep[14]) and int((~keep).sum()) <= 1
    bn, bg = NR.gaussian_normals_budget(rot.double(), sc.double(), me.double(), V.double(), True, g.double())
    rd = rot.to(DEV).requires_grad_(True)
    n = N.gaussian_normals(rd, sc.to(DEV), me.to(DEV), V.to(DEV), raw=True)
    (n * g.to(DEV)).sum().backward()
    for what, got, ref, bud in (("normals", n.detach(), n64.detach(), bn.b), ("dL/drotations", rd.grad, r64.grad, bg.b)):
        err = (got.double().cpu() - ref).abs()
        assert bool(torch.isfinite(got).all()), what
        ratio = (err / NR.bound(bud, NR.K_NORMALS))[keep]
        i = int(ratio.max(1).values.argmax())
        print(f"[raw] normals under the clamp: {what}: worst error / bound {float(ratio.max()):.4f} (row {int(torch.nonzero(keep)[i])}); "
              f"row 13: gpu {got[13].cpu().numpy()}, float64 {ref[13].numpy()}")
        assert float(ratio.max()) <= 1.0, what
    assert float(r64.grad[13].abs().max()) > 1e9, "a row under the clamp carries g / eps"
