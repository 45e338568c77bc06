"""Every feature-map kernel instance (EXP_MODE x channel group, pre-cull on and off) and every shape of stage_round's compaction
against float64, from the case tables of tests/_features_cases.py (tests/test_features_cases_host.py shows that they reach each
instance, that the oracle alone meets every cap with half of it to spare, and that the one-tile layouts stage what they name).
References and helpers are those of tests/test_features_gpu.py; features, backgrounds are signed.  Each test prints its measured
figures before it asserts."""
from __future__ import annotations

import functools
import itertools

import numpy as np
import pytest
import torch

import _features_cases as FC
import _features_ref as FR
import _instance_cases as IC
from _util import assert_blend_matches, check_gradients, decode_result
from test_features_gpu import _backward, _native
from test_instances_gpu import _options

pytestmark = pytest.mark.gpu

DIRECTIONS = ("forward", "backward")


def _np(t):
    return None if t is None else t.numpy()


@functools.lru_cache(maxsize=None)
def _forward_reference(scene, layout, Cn, bg):
    case = dict(table="Q" if layout else "F", scene=scene, layout=layout, C=Cn, bg=bg)
    f, b = FC.case_features(case)
    return FR.forward_ref(FC.reference(case)["o"], f.numpy(), _np(b))


@functools.lru_cache(maxsize=None)
def _forward_f64(layout, Cn, bg):
    case = dict(table="Q", scene=None, layout=layout, C=Cn, bg=bg)
    f, b = FC.case_features(case)
    return FR.blend_f64(FC.reference(case)["o"], f.numpy(), _np(b))


def _forward(case, d, o, f, bg):
    """the native forward of a case under the options in force, held to the oracle's blend outside its fragile mask: (res, n,
    fragile pixels, max |dF|)"""
    res = _native(d, f, bg)
    assert res[-1].shape == (case["C"], d["H"], d["W"]) and res[-1].dtype == torch.float32
    n = decode_result(d, res)
    frag_px, _ = assert_blend_matches(n, o, what=case["id"])
    ref = _forward_reference(case["scene"], case["layout"], case["C"], case["bg"])
    err = float(np.abs(res[-1].cpu().numpy() - ref)[:, ~frag_px].max(initial=0.0))
    return res, n, frag_px, err


def _backward_ratio(case, d, o, n, f, bg, frag_px):
    """one backward with colour and feature upstream gradients (NaN-poisoned outputs) over the float64 reference's bound: (worst
    ratio, dL_dfeatures' ratio, got, budget, check_gradients' report)"""
    g, gF = FC.upstream(case, frag_px)
    ref, bud, frag = FR.backward_ref(d, o, n, g.numpy(), f.numpy(), _np(bg), gF.numpy())
    got = _backward(d, n, g, f, bg, gF)
    report = []
    worst = check_gradients(d, got, ref, bud, frag, report=report)
    return worst, [r["worst_ratio"] for r in report if r["array"] == "dL_dfeatures"][0], got, bud, report


# ---- table F
@pytest.mark.parametrize("case", FC.TABLE_F, ids=[c["id"] for c in FC.TABLE_F])
def test_general_scene(native_lib, case):
    d, o = FC.inputs(case), FC.reference(case)["o"]
    f, bg = FC.case_features(case)
    with _options(case["options"]):
        res, n, frag_px, err = _forward(case, d, o, f, bg)
        print(f"[features instances] {case['id']}: {FC.forward_instance(case)} max |dF| = {err:.2e} outside "
              f"{int(frag_px.sum())} fragile pixels")
        assert err <= 1e-5   # the weights sum to <= 1 and |f| < 1
        worst, worst_f, _, _, report = _backward_ratio(case, d, o, n, f, bg, frag_px)
    print(f"[features instances] {case['id']}: {FC.backward_instance(case)} worst gradient error / bound {worst:.3f} "
          f"(dL_dfeatures {worst_f:.3f})")
    assert worst <= 1.0, report


# ---- table Q
def _staged(n, cull):
    """[direction][quarter] -> survivors per round, from the library's own records of a one-tile frame"""
    out = {}
    for direction in DIRECTIONS:
        c = FC.staged_counts(n, n["point_list"], n["ranges"], n["n_contrib"], cull, direction)
        assert sorted(c) == [(0, s) for s in range(4)]
        out[direction] = [c[(0, s)] for s in range(4)]
    return out


@pytest.mark.parametrize("case", FC.TABLE_Q, ids=[c["id"] for c in FC.TABLE_Q])
def test_one_tile_layout(native_lib, case):
    from gaussian_gan_decoder_amd import _capi
    assert _capi.FEATURES_ROUND == FC.ROUND
    name, Cn = case["layout"], case["C"]
    d, o = FC.inputs(case), FC.reference(case)["o"]
    f, bg = FC.case_features(case)
    quarters, kinds = FC.layout_quarters(name), FC.layout_kinds(name)
    with _options(case["options"]):
        res, n, frag_px, err = _forward(case, d, o, f, bg)
        # what the rounds stage, from the records the kernels read: with the cull on the box test keeps a quarter's own splats and
        # no others, which gives the layout's survivor counts; with it off every entry of a round
        np.testing.assert_array_equal(n["point_list"], np.arange(d["P"]))
        on, off = _staged(n, 1), _staged(n, 0)
        print(f"[features instances] {case['id']}: staged with the cull on {on}, off {off}")
        assert on == FC.Q_STAGED[name], "the library's records do not stage the layout"
        for direction in DIRECTIONS:
            for s in range(4):
                assert sum(off[direction][s]) == FC.quarter_maxn(n["n_contrib"], s)
        if name == "empty-rounds":
            assert any(FC.empty_round_between(c) for c in on["forward"]) and any(FC.empty_round_between(c) for c in on["backward"])
        # forward: both references
        err64 = float(np.abs(res[-1].cpu().numpy() - _forward_f64(name, Cn, case["bg"]))[:, ~frag_px].max(initial=0.0))
        print(f"[features instances] {case['id']}: {FC.forward_instance(case)} max |dF| = {err:.2e} (oracle), {err64:.2e} (float64) "
              f"outside {int(frag_px.sum())} fragile pixels")
        assert err <= 1e-5 and err64 <= 1e-5
        # a pixel without a contributor returns feature_bg (or 0) exactly: whole quarters here
        F = res[-1].cpu()
        nothing = torch.from_numpy(n["n_contrib"] == 0)
        want = (torch.zeros(Cn) if bg is None else bg)[:, None].expand(Cn, int(nothing.sum()))
        assert torch.equal(F[:, nothing], want)
        for s in range(4):
            if not ((quarters == s) & (kinds != "dead")).any():
                qx0, qy0 = FC.quarter_origin(s)
                assert nothing[qy0:qy0 + 8, qx0:qx0 + 8].all()
        # the cull is exact: only the staging differs, the map is the same bits
        with _options(dict(case["options"], cull=1 - case["options"]["cull"])):
            flipped = _native(d, f, bg)
        assert torch.equal(flipped[-1], res[-1]), "the map differs between cull on and off"
        worst, worst_f, got, bud, report = _backward_ratio(case, d, o, n, f, bg, frag_px)
    print(f"[features instances] {case['id']}: {FC.backward_instance(case)} worst gradient error / bound {worst:.3f} "
          f"(dL_dfeatures {worst_f:.3f})")
    assert worst <= 1.0, report
    unseen = (bud["dL_dfeatures"] == 0.0).all(axis=1)      # no (pixel, splat) pair: the reference's sum has no term
    assert unseen[kinds == "dead"].all() and not unseen[kinds != "dead"].any()
    assert (got["dL_dfeatures"][unseen] == 0.0).all(), "a splat no pixel blends has a feature gradient"


def test_layouts_reach_the_survivor_counts(native_lib):
    """over the three layouts, from the library's records, in EACH direction with the cull on: rounds of 0, 1, 31, 32, 33 and 63 or
    64 survivors, a quarter of three or more rounds, and an empty round between two others"""
    seen = {direction: set() for direction in DIRECTIONS}
    rounds = {direction: 0 for direction in DIRECTIONS}
    between = {direction: False for direction in DIRECTIONS}
    for name in FC.LAYOUTS:
        case = dict(table="Q", scene=None, layout=name, C=1, bg=True)
        d = FC.inputs(case)
        n = decode_result(d, _native(d, *FC.case_features(case)))
        st = _staged(n, 1)
        for direction in DIRECTIONS:
            seen[direction] |= set(itertools.chain.from_iterable(st[direction]))
            rounds[direction] = max(rounds[direction], max(len(c) for c in st[direction]))
            between[direction] |= name == "empty-rounds" and any(FC.empty_round_between(c) for c in st[direction])
    print(f"[features instances] survivor counts reached: { {k: sorted(v) for k, v in seen.items()} }, most rounds {rounds}")
    for direction in DIRECTIONS:
        assert {0, 1, FC.FLUSH - 1, FC.FLUSH, FC.FLUSH + 1} <= seen[direction], direction
        assert seen[direction] & {FC.ROUND - 1, FC.ROUND}, direction
        assert rounds[direction] >= 3 and between[direction], direction


# ---- a partial image: 17 x 33, tiles whose right quarters and bottom rows lie outside
@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("Cn", [9, 17])
def test_partial_image_backward(native_lib, Cn, cull):
    case = dict(id=f"P257-M9-C{Cn}-cull{cull}", table="F", scene="P257-M9", layout=None, C=Cn, bg=cull == 1,
                options=dict(IC.DEFAULTS, cull=cull))
    d, o = FC.inputs(case), FC.reference(case)["o"]
    assert (d["W"], d["H"]) == (17, 33)
    f, bg = FC.case_features(case)
    with _options(case["options"]):
        res, n, frag_px, err = _forward(case, d, o, f, bg)
        print(f"[features instances] {case['id']}: max |dF| = {err:.2e} outside {int(frag_px.sum())} fragile pixels")
        assert err <= 1e-5
        worst, worst_f, _, _, report = _backward_ratio(case, d, o, n, f, bg, frag_px)
    print(f"[features instances] {case['id']}: {FC.backward_instance(case)} worst gradient error / bound {worst:.3f} "
          f"(dL_dfeatures {worst_f:.3f})")
    assert worst <= 1.0, report
