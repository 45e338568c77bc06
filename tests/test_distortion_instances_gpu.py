"""Every depth-distortion kernel instance (forward EXP_MODE 0 .. 2, backward 0 .. 3, pre-cull on and off) at every shape of a
round and of the backward's flush chunk against float64, from the case table of tests/_distortion_cases.py
(tests/test_distortion_cases_host.py shows that the table names each instance, that the oracle alone meets every cap with half of
it to spare, that the one-tile layouts stage what they name at the table's depth step, and that a record missing at a round or
chunk edge would move the reference by ten bars).  Reference and helpers are those of tests/test_distortion_gpu.py, at the
table's own bar K_Q (four times the float32 twin's share on these layouts) instead of the general K.  Each test prints its measured
figures before it asserts."""
from __future__ import annotations

import itertools

import numpy as np
import pytest
import torch

import _distortion_cases as DC
import _distortion_ref as DR
import _instance_cases as IC
from _util import assert_blend_matches, decode_result
from test_distortion_gpu import _backward, _check_backward, _check_forward, _native, _reference
from test_instances_gpu import _options

pytestmark = pytest.mark.gpu


def _staged(n, cull):
    """[direction][quarter] -> survivors per round, from the library's own records of a one-tile frame"""
    out = {}
    for direction in DC.DIRECTIONS:
        c = DC.staged_counts(n, n["point_list"], n["ranges"], n["n_contrib"], cull, direction)
        assert sorted(c) == [(0, s) for s in range(4)]
        out[direction] = [c[(0, s)] for s in range(4)]
    return out


def _quarter(a, sub):
    qx0, qy0 = DC.quarter_origin(sub)
    return a[..., qy0:qy0 + 8, qx0:qx0 + 8]


def _forward(case, d, o):
    """the native forward of a layout under the options in force: (res, n, fragile pixels)"""
    res = _native(d)
    assert len(res) == 9 and res[8].shape == (1, d["H"], d["W"]) and res[8].dtype == torch.float32
    n = decode_result(d, res)
    frag_px, _ = assert_blend_matches(n, o, what=case["id"])
    np.testing.assert_array_equal(n["point_list"], np.arange(d["P"]))
    return res, n, frag_px


def _rows_are_zero(got, rows, what):
    for k, v in got.items():
        if v.size:
            assert (v.reshape(len(rows), -1)[rows] == 0.0).all(), f"{k}: {what}"


def _unseen(r):
    """[P]: no (pixel, record) pair of the reference's walk carries an upstream gradient to the Gaussian"""
    return (r["S_opacity"] == 0.0) & (r["S_z"] == 0.0) & (r["S_mean2D"] == 0.0).all(axis=1) & (r["S_conic"] == 0.0).all(axis=1)


@pytest.mark.parametrize("case", DC.TABLE_D, ids=[c["id"] for c in DC.TABLE_D])
def test_one_tile_layout(native_lib, case):
    from gaussian_gan_decoder_amd import _capi
    assert _capi.FEATURES_ROUND == DC.ROUND
    name = case["layout"]
    d, o = DC.inputs(case), DC.reference(case)["o"]
    quarters, kinds = DC.layout_quarters(name), DC.layout_kinds(name)
    with _options(case["options"]):
        res, n, frag_px = _forward(case, d, o)
        # what the rounds stage, from the records the kernels read
        on, off = _staged(n, 1), _staged(n, 0)
        print(f"[distortion instances] {case['id']}: staged with the cull on {on}, off {off}")
        assert on == DC.Q_STAGED[name], "the library's records do not stage the layout"
        for direction in DC.DIRECTIONS:
            for s in range(4):
                assert sum(off[direction][s]) == DC.quarter_maxn(n["n_contrib"], s)
        if name == "empty-rounds":
            assert all(any(DC.empty_round_between(c) for c in on[direction]) for direction in DC.DIRECTIONS)
        # forward against float64 over the native lists; exactly 0 where fewer than two contributors are seen
        g = DC.upstream(case, frag_px)
        ref, bud, frag, r = _reference(("cases", name), d, o, n, g)
        D = res[8][0].cpu().numpy()
        _check_forward(D, r, frag_px, f"{case['id']} {DC.forward_instance(case)}", kappa=DC.K_Q)
        for s in range(4):
            if not ((quarters == s) & (kinds != "dead")).any():
                assert (_quarter(r["count"], s) == 0).all() and (_quarter(D, s) == 0.0).all()
        if name == "ragged":    # lanes that see nothing, or one record, beside lanes past the second round
            few = (_quarter(r["count"], 2) < 2) & ~_quarter(frag_px, 2)
            assert int(few.sum()) >= 8 and (_quarter(D, 2)[few] == 0.0).all() and int(_quarter(n["n_contrib"], 2).max()) > 2 * DC.ROUND
        # the cull is exact: only the staging differs, the map is the same bits
        with _options(dict(case["options"], cull=1 - case["options"]["cull"])):
            flipped = _native(d)
        assert torch.equal(flipped[8], res[8]), "the map differs between cull on and off"
        # backward with dL/dD alone into NaN-poisoned outputs
        got = _backward(d, n, g)
    _check_backward(d, got, ref, bud, frag, f"{case['id']} {DC.backward_instance(case)}", kappa=DC.K_Q)
    unseen = _unseen(r)
    assert unseen[kinds == "dead"].all()
    _rows_are_zero(got, unseen, "a splat no pixel blends has a gradient")


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("name", list(DC.LAYOUTS))
def test_silent_quarter(native_lib, name, cull):
    """dL/dD zero on all 64 pixels of one walking quarter, N(0, 1) on the others: that quarter's workgroup leaves before its
    pre-pass, its splats (confined to it) get exactly 0.0 in every array, the other quarters' still meet the bar -- each walking
    quarter in turn (in "ragged" the only one: nothing is left)"""
    case = dict(id=f"{name}-silent-cull{cull}", layout=name, options=dict(IC.DEFAULTS, cull=cull))
    d, o = DC.inputs(case), DC.reference(case)["o"]
    quarters, kinds = DC.layout_quarters(name), DC.layout_kinds(name)
    with _options(case["options"]):
        res, n, frag_px = _forward(case, d, o)
        walking = [s for s in range(4) if DC.quarter_maxn(n["n_contrib"], s) > 0]
        assert walking == sorted({int(q) for q, k in zip(quarters, kinds) if k != "dead"})
        for s in walking:
            g = DC.upstream(case, frag_px).clone()
            _quarter(g, s)[...] = 0.0
            assert int((_quarter(g, s) == 0.0).sum()) == 64
            ref, bud, frag, r = _reference(("silent", name, s), d, o, n, g)
            got = _backward(d, n, g)
            confined = quarters == s
            assert _unseen(r)[confined].all()
            _rows_are_zero(got, confined, f"a splat of the silent quarter {s} has a gradient")
            _check_backward(d, got, ref, bud, frag, f"{case['id']} quarter {s} silent", kappa=DC.K_Q)
            loud = (kinds != "dead") & ~confined
            if loud.any():
                rows = np.abs(got["dL_dmeans3D"].reshape(d["P"], -1)).max(axis=1)
                assert (rows[loud] > 0.0).all(), "a splat of a quarter with an upstream gradient received none"


@pytest.mark.parametrize("cull", [0, 1])
def test_partial_image(native_lib, cull):
    """17 x 33: tiles whose right quarters lie outside the image, quarters one pixel wide or one row high -- lanes with
    g.in == false inside a walking wave.  A general scene, so the general bar DR.K applies."""
    scene = dict(scene="P257-M9", feature="aux")
    d, o = IC.inputs(scene), IC.reference(scene)["o"]
    assert (d["W"], d["H"]) == (17, 33)
    what = f"P257-M9 cull{cull}"
    with _options(dict(IC.DEFAULTS, cull=cull)):
        res = _native(d)
        assert len(res) == 9 and res[8].shape == (1, d["H"], d["W"])
        n = decode_result(d, res)
        frag_px, _ = assert_blend_matches(n, o, what=what)
        g = torch.randn(1, d["H"], d["W"], generator=torch.Generator().manual_seed(IC.GRAD_SEED + 201))
        g[:, torch.from_numpy(frag_px)] = 0.0
        ref, bud, frag, r = _reference(("partial", "P257-M9"), d, o, n, g)
        _check_forward(res[8][0].cpu().numpy(), r, frag_px, what)
        assert int(r["count"].max()) >= 2 and int(r["count"][:, 16].max()) >= 2 and int(r["count"][32, :].max()) >= 2
        got = _backward(d, n, g)
    _check_backward(d, got, ref, bud, frag, what)


def test_layouts_reach_the_survivor_counts(native_lib):
    """over the three layouts, from the library's records of a render_distortion forward, in EACH direction with the cull on:
    rounds of 0, 1, 31, 32, 33 and 63 or 64 survivors, a quarter of three or more rounds, and an empty round between two others"""
    seen = {direction: set() for direction in DC.DIRECTIONS}
    rounds = {direction: 0 for direction in DC.DIRECTIONS}
    between = {direction: False for direction in DC.DIRECTIONS}
    for name in DC.LAYOUTS:
        d = DC.layout_inputs(name)
        res = _native(d)
        assert len(res) == 9
        st = _staged(decode_result(d, res), 1)
        for direction in DC.DIRECTIONS:
            seen[direction] |= set(itertools.chain.from_iterable(st[direction]))
            rounds[direction] = max(rounds[direction], max(len(c) for c in st[direction]))
            between[direction] |= name == "empty-rounds" and any(DC.empty_round_between(c) for c in st[direction])
    print(f"[distortion instances] survivor counts reached: { {k: sorted(v) for k, v in seen.items()} }, most rounds {rounds}")
    for direction in DC.DIRECTIONS:
        assert {0, 1, DC.FLUSH - 1, DC.FLUSH, DC.FLUSH + 1} <= seen[direction], direction
        assert seen[direction] & {DC.ROUND - 1, DC.ROUND}, direction
        assert rounds[direction] >= 3 and between[direction], direction
