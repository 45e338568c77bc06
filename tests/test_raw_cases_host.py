"""The raw-attribute case tables (tests/_raw_cases.py) proved sound on the CPU, from the oracle alone: the reference stays within
half of the helpers' caps, the float32 twins of tests/_raw_ref.py take the same integer decisions as the float64-activated
reference, the tables reach every kernel instance they name, the chain is float64 autograd of the torch getters, and the constants
of the bars in tests/_raw_cases.py are four times what the twins need -- measured here, printed, and held to the stored values."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import _instance_cases as IC
import _raw_cases as RC
import _raw_ref as RR
from _util import KAPPA, run_oracle

MEASURED = RC.TABLE_R + RC.TABLE_E + RC.TABLE_V      # (table S shares table R's references: the absolute sums pass no activation)
TWINS = (None,) + RC.PERTURB_SEEDS
_ids = lambda cases: [c["id"] for c in cases]


@functools.lru_cache(maxsize=None)
def _twin_forwards(case_id):
    case = next(c for c in RC.ALL if c["id"] == case_id)
    raw = RC.raw_inputs(case)
    return [run_oracle(RR.oracle_inputs(RR.activated32(raw, seed), RC.has_aa(case))) for seed in TWINS]


def _masked_upstream(case):
    """upstream gradients, zero on the reference's fragile pixels at RAW_WINDOW and where a twin stops at another contributor"""
    r = RC.reference(case)
    o = r["o"]
    differ = np.zeros_like(r["frag"])
    for t in _twin_forwards(case["id"]):
        differ |= t["n_contrib"] != o["n_contrib"]
    g, gD, gA = IC.upstream_gradients(o["H"], o["W"], r["frag"] | differ)
    return g.numpy(), gD.numpy(), gA.numpy(), differ


@functools.lru_cache(maxsize=None)
def _measure(case_id):
    """per case: the chained reference on the oracle's own lists and, for each twin, its share per array and forward deviation"""
    case = next(c for c in RC.ALL if c["id"] == case_id)
    r = RC.reference(case)
    g, gD, gA, _ = _masked_upstream(case)
    ref = RR.reference(r["raw"], r["act"], r["o"], case["feature"], g, gD, gA, absgrad=case["absgrad"], kappa=RC.KAPPA_RAW)
    shares, devs, cam = [], [], []
    if case["table"] == "V":
        camera = RR.camera_reference(r["act"], r["o"], case["feature"], ref["blend"], gD, gA)
    for seed in TWINS:
        tw = RR.twin32(r["raw"], case["feature"], g, gD, gA, perturb_seed=seed)
        shares.append(RR.share(tw["grads"], ref["ref2"], ref["bud2"], ref["frag"]))
        devs.append(RR.forward_deviation(r["o"], tw["o"]))
        if case["table"] == "V":
            cam.append(RR.camera_share(camera, r["o"], ref["blend"], tw["o"], tw["act"]))
    return dict(ref=ref, shares=shares, devs=devs, cam=cam)


@pytest.mark.parametrize("case", RC.ALL, ids=_ids(RC.ALL))
def test_reference_stays_within_half_of_the_caps(case):
    r = RC.reference(case)
    g, gD, gA, differ = _masked_upstream(case)
    ref = RR.reference(r["raw"], r["act"], r["o"], case["feature"], g, gD, gA, absgrad=case["absgrad"], kappa=RC.KAPPA_RAW) \
        if case["table"] == "S" else _measure(case["id"])["ref"]
    px, gs = int(r["frag"].sum()), int((ref["frag"] > 0).sum())
    cap_px, cap_g = RC.caps(case)
    print(f"[raw cases] {case['id']}: {px} fragile pixels at RAW_WINDOW (cap {cap_px}), {gs} fragile Gaussians (cap {cap_g}), "
          f"{int(differ.sum())} pixels where a twin stops elsewhere, conditioning of h {r['cond']:.1f}")
    assert px <= cap_px and gs <= cap_g
    assert int(differ.sum()) <= 2
    assert r["cond"] <= IC.COND_MAX, "the float32 h of a visible Gaussian is not pinned by the formula"
    assert int((r["o"]["radii"] > 0).sum()) >= min(200, r["raw"]["P"] // 2)


@pytest.mark.parametrize("case", MEASURED, ids=_ids(MEASURED))
def test_twins_take_the_references_integer_decisions(case):
    o = RC.reference(case)["o"]
    for seed, t in zip(TWINS, _twin_forwards(case["id"])):
        what = f"{case['id']} twin {seed}"
        assert t["num_rendered"] == o["num_rendered"], what
        for k in ("radii", "point_list", "ranges"):
            np.testing.assert_array_equal(t[k], o[k], err_msg=f"{what}: {k}")
        vis = o["radii"] > 0
        for k in ("xy", "rgb", "depths"):     # no activation enters them
            np.testing.assert_array_equal(t[k][vis], o[k][vis], err_msg=f"{what}: {k}")


def test_tables_reach_every_instance():
    reached = set(RC.NORMALS_INSTANCES)     # (tests/test_raw_instances_gpu.py::test_normals_under_the_clamp)
    for case in RC.ALL:
        reached |= RC.instances(case)
    assert reached == RC.every_instance(), (sorted(RC.every_instance() - reached), sorted(reached - RC.every_instance()))
    # each table reaches what it names
    bwd = lambda table: {RC.preprocess_backward_instance(c) for c in table}
    assert len(bwd(RC.TABLE_R)) == 12 and all(k.startswith("preprocess_backward") for k in bwd(RC.TABLE_R))
    assert len(bwd(RC.TABLE_S)) == 12 and all(k.startswith("preprocess_abs_backward") for k in bwd(RC.TABLE_S))
    assert len({RC.camera_instance(c) for c in RC.TABLE_V}) == 4
    assert len({k for c in RC.TABLE_R for k in RC.preprocess_instances(c)}) == 8
    for f in RC.FEATURES:     # the edge rows meet the plain, the _vec and the _staged form under every feature
        forms = {RC.preprocess_backward_instance(c).split("<")[0] for c in RC.TABLE_E if c["feature"] == f}
        assert forms == {"preprocess_backward_kernel", "preprocess_backward_vec_kernel", "preprocess_backward_staged_kernel"}
    # the restated rules are those of tests/_instance_cases.py on the same scene
    for c in RC.TABLE_R:
        if c["feature"] != "plain":
            assert RC.preprocess_backward_instance(c) == IC.preprocess_backward_instance(c)
            assert RC.preprocess_instances(c) == IC.preprocess_instances(c)


@pytest.mark.parametrize("case", [c for c in MEASURED if c["feature"] == "plain"], ids=lambda c: c["id"])
def test_chain_is_float64_autograd_of_the_getters(case):
    """the closed forms of tests/_raw_ref.py::jacobians in float64 against torch.exp / torch.nn.functional.normalize / torch.sigmoid
    under float64 autograd, to 1e-12 of each array's largest element -- the rows under the clamp included"""
    raw = RC.raw_inputs(case)
    gen = torch.Generator().manual_seed(3)
    P = raw["P"]
    ref = dict(dL_dscales=torch.randn(P, 3, generator=gen, dtype=torch.float64).numpy(),
               dL_drots=torch.randn(P, 4, generator=gen, dtype=torch.float64).numpy(),
               dL_dopacity=torch.randn(P, generator=gen, dtype=torch.float64).numpy())
    ref2, bud2 = RR.chain(raw, ref, {k: np.abs(v) for k, v in ref.items()})
    ls, rr, ol = (raw[k].double().requires_grad_(True) for k in ("scales", "rotations", "opacities"))
    outs = [torch.exp(ls), torch.nn.functional.normalize(rr), torch.sigmoid(ol)]
    torch.autograd.backward(outs, [torch.from_numpy(ref["dL_dscales"]), torch.from_numpy(ref["dL_drots"]),
                                   torch.from_numpy(ref["dL_dopacity"]).reshape(ol.shape)])
    act = RR.activated64(raw)
    for k, t in (("scales", outs[0]), ("rotations", outs[1]), ("opacities", outs[2])):
        assert torch.equal(act[k], t.detach().float().reshape(act[k].shape)), k
    for k, t in (("dL_dscales", ls), ("dL_drots", rr), ("dL_dopacity", ol)):
        want = t.grad.numpy().reshape(ref2[k].shape)
        assert np.isfinite(ref2[k]).all() and (bud2[k] >= 0).all()
        assert np.abs(ref2[k] - want).max() <= 1e-12 * np.abs(want).max(), k
    if case["edge"]:
        rows = RC.edge_rows(case)
        for j in RC.UNDER_CLAMP_ROWS:     # g / eps, no projection
            np.testing.assert_allclose(ref2["dL_drots"][rows[j]], ref["dL_drots"][rows[j]] / 1e-12, rtol=1e-14)


@pytest.mark.parametrize("case", RC.TABLE_E, ids=_ids(RC.TABLE_E))
def test_edge_rows_are_what_the_table_says(case):
    r = RC.reference(case)
    rows, o, act = RC.edge_rows(case), r["o"], r["act"]
    assert len(rows) == len(RC.EDGE_ROWS) and (o["radii"][rows] > 0).all()
    q = r["raw"]["rotations"].double().numpy()[rows]
    np.testing.assert_allclose(np.linalg.norm(q[:4], axis=1), [3.4, 0.01, 1e-6, 1e6], rtol=1e-6)
    assert (q[list(RC.ZERO_QUATERNION_ROWS)] == 0).all()
    assert (np.linalg.norm(q[list(RC.UNDER_CLAMP_ROWS)], axis=1) < 1e-12).all() and (q[list(RC.UNDER_CLAMP_ROWS)] != 0).any()
    # every row set by hand stays 1e-2 in log-alpha away from the 1 / 255 floor at its centre
    peak = o["conic_opacity"][rows, 3].astype(np.float64)
    assert (np.abs(np.log(peak * 255.0)) >= 1e-2).all()
    assert (peak[list(RC.UNDER_FLOOR_ROWS)] < 1.0 / 255.0).all()
    assert RR.activate(r["raw"], np.float32)[2][rows[11]] == 1.0, "1 / (1 + expf(-17)) is 1 in float32: a derivative of exactly 0"
    assert float(act["opacities"].reshape(-1)[rows[11]]) >= 1.0 - 2.0 ** -24
    ref = _measure(case["id"])["ref"]
    for k, v in ref["ref2"].items():
        if v is not None:
            assert (v[rows[list(RC.UNDER_FLOOR_ROWS)]] == 0).all(), k
    # the rows under the clamp are blended and carry a rotation gradient of the order 1e12 |g|; the +17 row's float64 derivative
    # stays under the floor of the bar
    if case["feature"] == "plain":
        assert (np.abs(ref["ref2"]["dL_drots"][rows[5]]).max() > 1e6)
    assert abs(ref["ref2"]["dL_dopacity"].reshape(-1)[rows[11]]) < 1e-5


def _round_up(x, digits=2):
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x)) - (digits - 1)
    return math.ceil(x / 10 ** e - 1e-9) * 10 ** e


def test_constants_are_four_times_the_twins_share():
    """the three constants of tests/_raw_cases.py against this file's own measurement, printed per array"""
    per_array, worst_case = {}, {}
    dev_c = dev_o = share_v = 0.0
    for case in MEASURED:
        m = _measure(case["id"])
        for sh in m["shares"]:
            for k, v in sh.items():
                if v > per_array.get(k, -1.0):
                    per_array[k], worst_case[k] = v, case["id"]
        dev_c = max(dev_c, max(d[0] for d in m["devs"]))
        if not RC.has_aa(case):     # (with anti-aliasing the record holds o h; the bar adds the conditioning of h there)
            dev_o = max(dev_o, max(d[1] for d in m["devs"]))
        share_v = max([share_v] + m["cam"])
    for k in sorted(per_array):
        print(f"[raw cases] twin share of {k}: {per_array[k]:.4f} ({worst_case[k]})")
    share = max(per_array.values())
    print(f"[raw cases] twin share {share:.4f} -> kappa_raw = max({KAPPA}, 4 x {_round_up(share)}) = {max(KAPPA, 4 * _round_up(share)):.3f}; "
          f"forward deviation: conic {dev_c:.1f}, opacity {dev_o:.1f} units; camera share {share_v:.4f} -> K_raw {math.ceil(4 * _round_up(share_v))}")
    assert RC.TWIN_SHARE == _round_up(share)
    assert RC.KAPPA_RAW == max(KAPPA, 4 * RC.TWIN_SHARE)
    assert RC.TWIN_CONIC_UNITS == math.ceil(dev_c) and RC.TWIN_OPACITY_UNITS == math.ceil(dev_o)
    assert RC.TWIN_SHARE_V == _round_up(share_v) and RC.K_RAW == math.ceil(4 * RC.TWIN_SHARE_V)
