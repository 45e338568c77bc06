"""Every depth / alpha (AUX) and anti-aliasing (AA) kernel instance against the CPU oracle, from the case tables of
tests/_instance_cases.py (tests/test_instance_cases_host.py shows that they reach each instance and that the oracle alone meets
every cap with half of it to spare).  Each case renders two frames -- the first of its shape on the exact two-call path, the
second in a single call -- under its own context options, checks the integer stages bit for bit, colour / final_T / n_contrib,
depth and alpha against the oracle, the frame against the one without the extension, and one backward against the fp64
reference within the suite's budget.  Each test prints its measured figures before it asserts."""
from __future__ import annotations

import contextlib

import numpy as np
import pytest
import torch

import _instance_cases as IC
from _depth_alpha_ref import backward_ref, forward_ref
from _util import assert_blend_matches, check_gradients, decode_result, run_oracle, same_frame
from test_antialiasing_gpu import (_backward, _check_record_opacity, _native, _oracle_opacities, _same_geometry,
                                   composed_reference)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FRAMES = ("exact two-call path", "single-call path")


@contextlib.contextmanager
def _options(opts):
    """the context of the current stream under a case's options; what it held before (and the default binning) afterwards"""
    from gaussian_gan_decoder_amd import _capi
    ctx = _capi.context_for(DEV)
    keys = dict(exp_mode=_capi.OPT_EXP_MODE, cull=_capi.OPT_BLEND_CULL, split=_capi.OPT_BLEND_SPLIT, fold=_capi.OPT_FOLD,
                msd=_capi.OPT_MSD_SORT)
    saved = {k: ctx.get_option(o) for k, o in keys.items()}
    try:
        for k, o in keys.items():
            ctx.set_option(o, opts[k])
        ctx.set_option(_capi.OPT_BINNING, opts["binning"])
        yield ctx
    finally:
        for k, o in keys.items():
            ctx.set_option(o, saved[k])
        ctx.set_option(_capi.OPT_BINNING, 1)


def _forget_shape(ctx, d):
    """the next forward of this shape is the first one: the exact two-call path"""
    ctx.capacity_hint.pop((d["P"], d["W"], d["H"]), None)


def _check_aux_forward(o, res, ok, what):
    """depth and alpha of the forward `res` against the oracle's blend of the pseudo-colour, outside the fragile mask: the
    bars of tests/test_depth_alpha_gpu.py::_check_forward.  Returns (alpha error, depth error / max z)."""
    depth, alpha = res[6].cpu().numpy()[0], res[7].cpu().numpy()[0]
    Dref, Aref = forward_ref(o)
    zmax = float(np.abs(o["depths"][o["radii"] > 0]).max(initial=1.0))
    err_a = float(np.abs(alpha - Aref)[ok].max(initial=0.0))
    err_t = float(np.abs(alpha - (1.0 - o["final_T"]))[ok].max(initial=0.0))
    err_d = float(np.abs(depth - Dref)[ok].max(initial=0.0))
    print(f"[instances] {what}: |dalpha| {err_a:.2e}, |alpha - (1 - T)| {err_t:.2e}, |ddepth| / max z {err_d / zmax:.2e}")
    assert err_a <= 1e-5, what
    assert err_t <= 1e-5, what
    assert err_d <= 1e-5 * zmax, f"{what}: max |ddepth| = {err_d} (max z {zmax})"
    return max(err_a, err_t), err_d / zmax


def _run_activated(case):
    d, ref = IC.inputs(case), IC.reference(case)
    aa, aux = IC.has_aa(case), IC.has_aux(case)
    o = None if aa else ref["o"]
    with _options(case["options"]) as ctx:
        _forget_shape(ctx, d)
        for frame in FRAMES:
            what = f"{case['id']} ({frame})"
            res = _native(d, aa=aa, aux=aux)
            n = decode_result(d, res)
            if aa:   # everything that does not depend on the opacity is the plain render's, the records carry o h
                vis = _same_geometry(n, decode_result(d, _native(d, aa=False)), what, d["shs"] is not None)
                _check_record_opacity(d, n, vis, what)
                if o is None:
                    op = _oracle_opacities(d, n)
                    o = ref["o"] if torch.equal(op, ref["d"]["opacities"]) else run_oracle(dict(d, opacities=op))
            assert n["num_rendered"] == o["num_rendered"], what
            np.testing.assert_array_equal(n["radii"].cpu().numpy(), o["radii"], err_msg=what)
            np.testing.assert_array_equal(n["point_list"], o["point_list"], err_msg=what)
            np.testing.assert_array_equal(n["ranges"], o["ranges"], err_msg=what)
            frag_px, _ = assert_blend_matches(n, o, what=what)
            if aux:
                _check_aux_forward(o, res, ~frag_px, what)
                if frame == FRAMES[0]:
                    _forget_shape(ctx, d)
                assert same_frame(_native(d, aa=aa, aux=False), res[:6]), f"{what}: the depth / alpha maps moved the frame"
        if aa:
            ref_g, bud, frag, g, gD, gA = composed_reference(d, n, seed=IC.GRAD_SEED, aux=aux)
        else:
            g, gD, gA = IC.upstream_gradients(d["H"], d["W"], frag_px)
            ref_g, bud, frag = backward_ref(d, o, n, g.numpy(), gD.numpy()[0], gA.numpy()[0])
        got = _backward(d, n, g, gD if aux else None, gA if aux else None, aa=aa)   # (NaN-fills the outputs first)
    report = []
    worst = check_gradients(d, got, ref_g, bud, frag, report=report)
    print(f"[instances] {case['id']}: worst gradient error / bound {worst:.3f}")
    assert worst <= 1.0, report


def _run_raw(case):
    """the raw-attribute form of an instance against its activated form pushed through the activations' Jacobians, as
    test_backward_with_raw_attributes of the depth / alpha and anti-aliasing tests: 1e-4 of the array's scale where the
    activations do not enter, 2e-4 where they do.  No upstream gradient reaches a pixel whose last contributor differs between
    the two runs, nor one where the activations' rounding can flip a decision in the middle of a list, which n_contrib does
    not show (IC.RAW_WINDOW; table C seed 56 has one: a record at alpha = 1/255 (1 +- 1e-5) under T = 0.33, blended by the
    raw run only -- 0.7 % of that Gaussian's dL_dcolors)."""
    d = IC.inputs(case)
    raw = IC.raw_inputs(d)
    aa, aux = IC.has_aa(case), IC.has_aux(case)
    with _options(case["options"]) as ctx:
        _forget_shape(ctx, d)
        for frame in FRAMES:
            what = f"{case['id']} ({frame})"
            res_raw = _native(raw, aa=aa, raw=True, aux=aux)
            if aux:
                if frame == FRAMES[0]:
                    _forget_shape(ctx, d)
                assert same_frame(_native(raw, aa=aa, raw=True, aux=False), res_raw[:6]), what
        res = _native(d, aa=aa, aux=aux)
        n, nr = decode_result(d, res), decode_result(raw, res_raw)
        np.testing.assert_array_equal(nr["radii"].cpu().numpy(), n["radii"].cpu().numpy())
        np.testing.assert_array_equal(nr["point_list"], n["point_list"])
        # raw-activation rounding can flip a blend decision: no upstream gradient there, in both runs
        differ = n["n_contrib"] != nr["n_contrib"]
        assert int(differ.sum()) <= 2, int(differ.sum())
        differ = differ | IC.raw_fragile_pixels(case)
        for k in (6, 7) if aux else ():
            assert float(np.abs(res_raw[k].cpu().numpy()[0] - res[k].cpu().numpy()[0])[~differ].max(initial=0.0)) <= 1e-4, what
        g, gD, gA = IC.upstream_gradients(d["H"], d["W"], differ)
        a = _backward(d, n, g, gD if aux else None, gA if aux else None, aa=aa)
        b = _backward(raw, nr, g, gD if aux else None, gA if aux else None, raw=True, aa=aa)
    s = d["opacities"].double().numpy().reshape(-1, 1)
    expect = {"dL_dmeans3D": (a["dL_dmeans3D"], 1e-4), "dL_dmeans2D": (a["dL_dmeans2D"], 1e-4), "dL_dcolors": (a["dL_dcolors"], 1e-4),
              "dL_dopacity": (a["dL_dopacity"] * s * (1.0 - s), 2e-4),
              "dL_dscales": (a["dL_dscales"] * d["scales"].double().numpy(), 2e-4)}
    if d["shs"] is not None:
        expect["dL_dsh"] = (a["dL_dsh"], 1e-4)
    if aa:   # (the anti-aliasing test holds every array to 2e-4: the h chain sits before the activations)
        expect = {k: (e, 2e-4) for k, (e, _) in expect.items()}
    worst = 0.0
    for k, (e, rel) in expect.items():
        scale = max(1.0, float(np.abs(e).max(initial=0.0)))
        assert np.isfinite(b[k]).all(), k
        err = float(np.abs(e - b[k].reshape(e.shape)).max(initial=0.0))
        worst = max(worst, err / (rel * scale))
        assert err <= rel * scale, (k, err, scale)
    print(f"[instances] {case['id']}: worst raw / activated difference over its bar {worst:.3f}")


def _run(case):
    """every case against the oracle in its activated form; a raw-attribute case then against that form as well"""
    _run_activated(case)
    if case["raw"]:
        _run_raw(case)


@pytest.mark.parametrize("case", IC.TABLE_A, ids=[c["id"] for c in IC.TABLE_A])
def test_blend_instance(native_lib, case):
    _run(case)


@pytest.mark.parametrize("case", IC.TABLE_B, ids=[c["id"] for c in IC.TABLE_B])
def test_per_gaussian_kernel_form(native_lib, case):
    _run(case)


_C = IC.table_c()


@pytest.mark.parametrize("case", _C, ids=[c["id"] for c in _C])
def test_random_configuration(native_lib, case):
    _run(case)


# ---- exact identities of the depth / alpha frames, once per table A scene and exp mode: no tolerance
IDENTITY = [(scene, em) for scene in ("A1", "A2") for em in (0, 1, 2, 3)]
IDENTITY_IDS = [f"{scene}-exp{em}" for scene, em in IDENTITY]


def _aux_frames(d, ctx):
    _forget_shape(ctx, d)
    return [_native(d, aa=False, aux=True) for _ in FRAMES]


def _assert_identical(a, b, what):
    for frame, x, y in zip(FRAMES, a, b):
        assert same_frame(x[:6], y[:6]), f"{what}: colour, final_T, n_contrib or the lists differ ({frame})"
        assert torch.equal(x[6], y[6]), f"{what}: depth differs ({frame})"
        assert torch.equal(x[7], y[7]), f"{what}: alpha differs ({frame})"


@pytest.mark.parametrize("scene,em", IDENTITY, ids=IDENTITY_IDS)
def test_culling_does_not_change_a_depth_alpha_frame(native_lib, scene, em):
    d = IC.inputs(dict(scene=scene))
    frames = []
    for cull in (0, 1):
        with _options(dict(IC.DEFAULTS, exp_mode=em, cull=cull)) as ctx:
            frames.append(_aux_frames(d, ctx))
    _assert_identical(*frames, "cull 0 / 1")


@pytest.mark.parametrize("scene,em", IDENTITY, ids=IDENTITY_IDS)
def test_binning_path_does_not_change_a_depth_alpha_frame(native_lib, scene, em):
    d = IC.inputs(dict(scene=scene))
    frames = []
    for binning in (0, 3):
        with _options(dict(IC.DEFAULTS, exp_mode=em, binning=binning)) as ctx:
            frames.append(_aux_frames(d, ctx))
    _assert_identical(*frames, "binning 0 / 3")


@pytest.mark.parametrize("scene,em", IDENTITY, ids=IDENTITY_IDS)
def test_blend_statistics_do_not_change_a_depth_alpha_frame(native_lib, scene, em):
    """a depth / alpha frame has no statistics instance (ggd_launch_blend): with the counters on it is the same frame"""
    d = IC.inputs(dict(scene=scene))
    with _options(dict(IC.DEFAULTS, exp_mode=em)) as ctx:
        off = _aux_frames(d, ctx)
        ctx.blend_stats(1)
        try:
            on = _aux_frames(d, ctx)
        finally:
            ctx.blend_stats(0)
    _assert_identical(off, on, "blend statistics off / on")
