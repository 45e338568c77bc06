"""The case tables of tests/_features_cases.py are sound, without a GPU: together they reach every feature-map kernel instance
the built library holds, each with the pre-cull on and off; the CPU oracle alone meets every cap the GPU tests' helpers assert
with half of it to spare; the hand-built one-tile layouts have the properties they are there for; and the two references of the
forward agree on them."""
from __future__ import annotations

import importlib.util
import itertools
import os

import numpy as np
import pytest

import _features_cases as FC
import _features_ref as FR
import _instance_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = FC.TABLE_F + FC.TABLE_Q
MODES, GROUPS = (0, 1, 2, 3), (4, 8, 16, 32)


def _kernel_names():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    from gaussian_gan_decoder_amd import _capi
    return {kr.short(k) for k in kr.kernel_resources(_capi.LIB_PATH)}


# ---- instance coverage
def test_channel_group_rule():
    assert [FC.channel_group(c) for c in (1, 4, 5, 8, 9, 16, 17, 31, 32)] == [4, 4, 8, 8, 16, 16, 32, 32, 32]
    assert sorted({FC.channel_group(c) for c in range(1, 33)}) == list(GROUPS)


def test_tables_reach_every_instance_with_the_cull_on_and_off(native_lib):
    names = _kernel_names()
    fwd = {n for n in names if n.startswith("features_forward_kernel<")}
    bwd = {n for n in names if n.startswith("features_backward_kernel<")}
    assert fwd == {f"features_forward_kernel<{e}, {g}>" for e in (0, 1, 2) for g in GROUPS}, sorted(fwd)
    assert bwd == {f"features_backward_kernel<{e}, {g}>" for e in MODES for g in GROUPS}, sorted(bwd)
    for rule, want in ((FC.forward_instance, fwd), (FC.backward_instance, bwd)):
        got = {(rule(c), c["options"]["cull"]) for c in ALL}
        assert got == set(itertools.product(want, (0, 1))), sorted(set(itertools.product(want, (0, 1))) - got)
    # table F alone reaches every instance, and both cull values of every backward instance of the two wide groups
    assert {FC.forward_instance(c) for c in FC.TABLE_F} == fwd and {FC.backward_instance(c) for c in FC.TABLE_F} == bwd
    wide = {(FC.backward_instance(c), c["options"]["cull"]) for c in FC.TABLE_F if c["C"] > 8}
    assert len(wide) == 4 * 2 * 2


def test_table_shapes():
    assert len(FC.TABLE_F) == 24 and len({c["id"] for c in ALL}) == len(ALL)
    assert {(c["options"]["exp_mode"], c["C"]) for c in FC.TABLE_F} == set(itertools.product(MODES, FC.F_CHANNELS))
    for key, values in (("scene", {"A1", "A2"}), ("bg", {True, False})):
        assert {c[key] for c in FC.TABLE_F} == values
        for em in MODES:   # every mode sees both
            assert {c[key] for c in FC.TABLE_F if c["options"]["exp_mode"] == em} == values
    assert {(c["options"]["cull"], c["bg"]) for c in FC.TABLE_F} == set(itertools.product((0, 1), (True, False)))
    # table Q: every layout at the default mode over C on, behind and before every group edge, with both cull values; the
    # other modes at one C per group
    for name in FC.LAYOUTS:
        q = [c for c in FC.TABLE_Q if c["layout"] == name]
        assert {(c["C"], c["options"]["cull"]) for c in q if c["options"]["exp_mode"] == 3} == \
            set(itertools.product((1, 4, 5, 8, 9, 16, 17, 32), (0, 1)))
        for em in (0, 1, 2):
            got = {(FC.channel_group(c["C"]), c["options"]["cull"]) for c in q if c["options"]["exp_mode"] == em}
            assert got == set(itertools.product(GROUPS, (0, 1)))
        assert {c["bg"] for c in q} == {True, False}
    # channels beyond half a group, which the second half of the backward's flush lanes owns (CH = CG / 2)
    for g in GROUPS:
        assert any(FC.channel_group(c["C"]) == g and c["C"] > g // 2 for c in ALL)


def test_features_are_signed_and_seeded():
    f, bg = FC.features(194, 9)
    assert f.shape == (194, 9) and bg.shape == (9,)
    assert float(f.min()) < -0.9 and float(f.max()) > 0.9 and float(f.abs().max()) < 1.0 and float(bg.abs().max()) < 1.0
    assert not np.array_equal(f.numpy()[:, :4], FC.features(194, 4)[0].numpy())
    assert FC.features(194, 9, False)[1] is None and FC.features(194, 9, False)[0].equal(f)


# ---- the caps, from the oracle alone
@pytest.mark.parametrize("case", ALL, ids=[c["id"] for c in ALL])
def test_caps_are_met_by_the_reference_alone(case):
    px, gaussians = FC.fragile_counts(case)
    cap_px, cap_gaussians = FC.caps(case)
    if case["table"] == "Q":
        assert (cap_px, cap_gaussians) == (1, 2)
    assert px <= cap_px, f"{px} fragile pixels"
    assert gaussians <= cap_gaussians, f"{gaussians} Gaussians sit on the alpha floor"


# ---- the layouts of table Q
def _quarter(a, sub):
    qx0, qy0 = FC.quarter_origin(sub)
    return a[qy0:qy0 + 8, qx0:qx0 + 8]


@pytest.mark.parametrize("name", list(FC.LAYOUTS))
def test_layout_geometry(name):
    d, o = FC.layout_inputs(name), FC.reference(dict(table="Q", layout=name))["o"]
    k = d["P"]
    assert (d["W"], d["H"]) == (16, 16) and k <= 200
    quarters, kinds = FC.layout_quarters(name), FC.layout_kinds(name)
    assert kinds[-1] == "dead" and (kinds[:-1] != "dead").all()
    # one tile whose list is the index order, every splat in it
    assert o["num_rendered"] == k and (o["radii"] > 0).all()
    np.testing.assert_array_equal(o["ranges"], [[0, k]])
    np.testing.assert_array_equal(o["point_list"], np.arange(k))
    assert (np.diff(o["depths"]) > 0).all()
    # isotropic records; each centre within 1 px of its quarter's centre (the stacked opaque ones: on a pixel, half a pixel off)
    co = o["conic_opacity"].astype(np.float64)
    assert np.abs(co[:, 1]).max() <= 0.01 * co[:, 0].min() and np.abs(co[:, 0] / co[:, 2] - 1.0).max() <= 0.01
    x, y = o["xy"][:, 0].astype(np.float64), o["xy"][:, 1].astype(np.float64)
    q0 = np.array([FC.quarter_origin(q) for q in quarters], np.float64)
    assert np.abs(x - q0[:, 0] - 3.5).max() <= 1.0 + 1e-4 and np.abs(y - q0[:, 1] - 3.5).max() <= 1.0 + 1e-4
    # footprints: none within 1.5 px of another quarter's pixel rectangle, each inside its own
    r = FC.footprint_radius(co)
    live = kinds != "dead"
    assert (r[live] > 0.5).all() and r[~live].max(initial=0.0) == 0.0 and r.max() <= 1.95
    for sub in range(4):
        other = (quarters != sub) & live
        dist = FC.rect_distance(x[other], y[other], r[other], sub)
        assert dist.min(initial=np.inf) >= 1.5, (sub, float(dist.min()))
        own = (quarters == sub) & live
        qx0, qy0 = FC.quarter_origin(sub)
        inside = np.minimum.reduce([x[own] - r[own] - qx0, qx0 + 7.0 - x[own] - r[own], y[own] - r[own] - qy0,
                                    qy0 + 7.0 - y[own] - r[own]]) if own.any() else np.array([1.0])
        assert inside.min() >= 0.5, (sub, float(inside.min()))
    # so a quarter's box test keeps exactly its own splats (with the footprint radius as the half extent)
    rec = FC.oracle_records(o)
    for sub in range(4):
        qx0, qy0 = (np.float32(v) for v in FC.quarter_origin(sub))
        keep = FC._box_hits(rec["xy"][:, 0], rec["xy"][:, 1], rec["cull_extent"][:, 0], rec["cull_extent"][:, 1], qx0,
                            qx0 + np.float32(7), qy0, qy0 + np.float32(7))
        np.testing.assert_array_equal(keep, (quarters == sub) & live)
    # quarters without a splat of their own blend nothing
    for sub in range(4):
        if not ((quarters == sub) & live).any():
            assert _quarter(o["n_contrib"], sub).max() == 0 and (_quarter(o["final_T"], sub) == 1.0).all()


def _counts(name, direction, cull=1):
    o = FC.reference(dict(table="Q", layout=name))["o"]
    return FC.staged_counts(FC.oracle_records(o), o["point_list"], o["ranges"], o["n_contrib"], cull, direction)


def test_block_layouts_stay_clear_of_the_stop_and_stage_what_they_name():
    for name in ("empty-rounds", "flush-edges"):
        o = FC.reference(dict(table="Q", layout=name))["o"]
        assert float(o["final_T"].min()) >= 0.05
    fwd, bwd = _counts("empty-rounds", "forward"), _counts("empty-rounds", "backward")
    assert fwd == {(0, 0): [64, 0, 64], (0, 1): [], (0, 2): [], (0, 3): [0, 64, 0, 1]}
    assert bwd == {(0, 0): [64, 0, 64], (0, 1): [], (0, 2): [], (0, 3): [1, 63, 1, 0]}   # offset by one entry
    assert FC.empty_round_between(fwd[(0, 3)]) and FC.empty_round_between(bwd[(0, 0)]) and not FC.empty_round_between(bwd[(0, 3)])
    assert _counts("empty-rounds", "forward", cull=0) == {(0, 0): [64, 64, 64], (0, 1): [], (0, 2): [], (0, 3): [64, 64, 64, 1]}
    fwd, bwd = _counts("flush-edges", "forward"), _counts("flush-edges", "backward")
    assert fwd == {(0, 0): [], (0, 1): [33, 32, 1], (0, 2): [31, 32], (0, 3): []}
    assert bwd == {(0, 0): [], (0, 1): [32, 33, 1], (0, 2): [32, 31], (0, 3): []}
    for name in FC.LAYOUTS:   # the table the GPU tests hold the library's own records to
        for direction in ("forward", "backward"):
            assert [_counts(name, direction)[(0, s)] for s in range(4)] == FC.Q_STAGED[name][direction], (name, direction)
    # over the layouts, in each direction: no survivor, one, the counts around the flush chunk, a full round or one short of it,
    # and a quarter of three or more rounds
    for direction in ("forward", "backward"):
        per_quarter = [c for name in FC.LAYOUTS for c in _counts(name, direction).values()]
        seen = set(itertools.chain.from_iterable(per_quarter))
        assert {0, 1, FC.FLUSH - 1, FC.FLUSH, FC.FLUSH + 1} <= seen and seen & {FC.ROUND - 1, FC.ROUND}, sorted(seen)
        assert max(len(c) for c in per_quarter) >= 3


def test_round_bounds():
    assert FC.round_bounds(0, "forward") == [] and FC.round_bounds(0, "backward") == []
    assert FC.round_bounds(193, "forward") == [(0, 64), (64, 128), (128, 192), (192, 193)]
    assert FC.round_bounds(193, "backward") == [(129, 193), (65, 129), (1, 65), (0, 1)]
    assert FC.round_bounds(128, "backward") == [(64, 128), (0, 64)] and FC.round_bounds(64, "backward") == [(0, 64)]


def test_ragged_layout_spreads_the_lanes_of_one_quarter():
    o = FC.reference(dict(table="Q", layout="ragged"))["o"]
    sub = 2
    nc, fT = _quarter(o["n_contrib"], sub), _quarter(o["final_T"], sub)
    # a pixel that the T < 1e-4 test ends within the first round: the next of the stack would take it under the stop
    stopped = (fT < 1e-3) & (nc > 0)
    assert int(stopped.sum()) == 1 and int(nc[stopped][0]) < FC.ROUND
    y, x = (int(v[0]) for v in np.nonzero(stopped))
    g = int(o["point_list"][int(nc[y, x])])           # the record behind its last contributor
    assert FC.layout_kinds("ragged")[g] == "opaque"
    qx0, qy0 = FC.quarter_origin(sub)
    dx, dy = float(o["xy"][g, 0]) - (qx0 + x), float(o["xy"][g, 1]) - (qy0 + y)
    a, b, c, op = (float(v) for v in o["conic_opacity"][g])
    alpha = min(0.99, op * np.exp(-0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy))
    assert alpha >= 1.0 / 255.0 and float(fT[y, x]) * (1.0 - alpha) < 0.5e-4 and float(fT[y, x]) > 1.2e-4
    # every other pixel stays clear of the stop; some walk past two rounds, some see nothing
    assert float(fT[~stopped].min()) >= 1e-3
    assert int((nc >= 2 * FC.ROUND + 1).sum()) >= 8 and int((nc == 0).sum()) >= 8
    assert _counts("ragged", "forward")[(0, sub)] == [64, 64, 17] and int(nc.max()) == 145
    assert all(_counts("ragged", "forward")[(0, s)] == [] for s in (0, 1, 3))


# ---- the two references of the forward against each other
@pytest.mark.parametrize("name", list(FC.LAYOUTS))
@pytest.mark.parametrize("Cn,bg", [(5, True), (17, False)])
def test_references_agree_on_the_layouts(name, Cn, bg):
    o = FC.reference(dict(table="Q", layout=name))["o"]
    f, b = FC.features(o["P"], Cn, bg)
    b = None if b is None else b.numpy()
    err = float(np.abs(FR.forward_ref(o, f.numpy(), b) - FR.blend_f64(o, f.numpy(), b)).max())
    print(f"[features cases] {name} C={Cn}: |forward_ref - blend_f64| = {err:.2e}")
    assert err <= 1e-5


def test_table_f_scenes_are_those_of_the_blend_instances():
    for c in FC.TABLE_F:
        assert FC.inputs(c) is IC.inputs(dict(scene=c["scene"]))
        assert int(FC.reference(c)["o"]["n_contrib"].max()) >= 60
