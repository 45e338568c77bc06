"""The case tables of tests/_instance_cases.py are sound, without a GPU: together they reach every depth / alpha (AUX) and
anti-aliasing (AA) kernel instance the built library holds, every cap the GPU tests' helpers assert is met by the CPU oracle
alone with half of it to spare, and the tables are not vacuous."""
from __future__ import annotations

import importlib.util
import os
import re

import pytest

import _instance_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AB = IC.TABLE_A + IC.TABLE_B
C = IC.table_c()
ALL = AB + C


def _kernel_names():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    from gaussian_gan_decoder_amd import _capi
    return {kr.short(k) for k in kr.kernel_resources(_capi.LIB_PATH)}


def _targs(name):
    m = re.search(r"<(.*)>$", name)
    return [a.strip() for a in m.group(1).split(",")] if m else []


def _reached(cases, rule):
    out = set()
    for c in cases:
        r = rule(c)
        out |= r if isinstance(r, set) else ({r} if r is not None else set())
    return out


# family -> (the library's instances of it, the dispatch rule, table C reaches each again)
FAMILIES = {
    "aux forward blend": (lambda n: n.startswith("blend_forward_kernel<") and _targs(n)[-1] == "true",
                          IC.forward_blend_instance, 6, True),
    # (table C draws the exp modes 0, 2 and 3 only)
    "aux backward blend": (lambda n: n.startswith("blend_backward_quarter_kernel<") and _targs(n)[-1] == "true",
                           IC.backward_blend_instance, 8, False),
    "preprocess backward with AA or AUX": (lambda n: n.startswith("preprocess_backward") and "true" in _targs(n)[-2:],
                                           IC.preprocess_backward_instance, 9, True),
    "preprocess with AA": (lambda n: n.startswith("preprocess_kernel<") and _targs(n)[-1] == "true",
                           IC.preprocess_instances, 4, True),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_tables_reach_every_instance_of_the_library(native_lib, family):
    in_library, rule, count, again = FAMILIES[family]
    want = {n for n in _kernel_names() if in_library(n)}
    assert len(want) == count, sorted(want)
    got = {n for n in _reached(AB, rule) if in_library(n)}
    assert got == want, f"tables A and B miss {sorted(want - got)} / name {sorted(got - want)}"
    if again:
        got_c = {n for n in _reached(C, rule) if in_library(n)}
        assert got_c == want, f"table C misses {sorted(want - got_c)} / names {sorted(got_c - want)}"


def test_every_reached_name_is_a_kernel_of_the_library(native_lib):
    names = _kernel_names()
    for rule in (IC.forward_blend_instance, IC.backward_blend_instance, IC.preprocess_backward_instance,
                 IC.preprocess_instances):
        missing = _reached(ALL, rule) - names
        assert not missing, sorted(missing)


def test_table_sizes():
    assert len(IC.TABLE_A) == 32 and len({c["id"] for c in IC.TABLE_A}) == 32
    assert sum(c["options"]["split"] == 3 for c in IC.TABLE_A) == 16
    plain_b = [c for c in IC.TABLE_B if not c["raw"]]
    assert len(plain_b) == 27 and len(IC.TABLE_B) == 27 + 3 * len(IC.B_RAW_SCENES)
    # every scene of table B with scales and rotations but the adversarial one also runs with raw attributes
    assert IC.B_RAW_SCENES == [s for s in IC.B_SCENES if s != "adversarial" and IC.SCENES[s]()["scales"] is not None]
    assert len(C) == 96 and len({c["id"] for c in ALL}) == len(ALL)


@pytest.mark.parametrize("case", ALL, ids=[c["id"] for c in ALL])
def test_caps_are_met_by_the_reference_alone(case):
    px, gaussians = IC.fragile_counts(case)
    cap_px, cap_gaussians = IC.caps(case)
    assert px <= cap_px, f"{px} fragile pixels"
    assert gaussians <= cap_gaussians, f"{gaussians} Gaussians sit on the alpha floor"
    # the helper's o_eff is then the reference everywhere (test_antialiasing_gpu._oracle_opacities never takes the GPU's value);
    # the needles of the adversarial scene are the stated exception
    if IC.has_aa(case) and case["scene"] != "adversarial":
        assert IC.reference(case)["cond"] <= IC.COND_MAX
    if case["raw"]:   # the raw / activated comparison leaves out the pixels an activation's rounding can flip: as few
        assert int(IC.raw_fragile_pixels(case).sum()) <= cap_px


def test_kept_seeds_follow_the_rule():
    kept, seed = [], 0
    while len(kept) < len(IC.C_SEEDS):
        case = IC.fuzz_case(seed)
        if all(n <= cap for n, cap in zip(IC.fragile_counts(case), IC.caps(case))):
            kept.append(seed)
        seed += 1
    assert tuple(kept) == IC.C_SEEDS


def test_tables_are_not_vacuous():
    assert sum(IC.reference(c)["o"]["num_rendered"] > 0 for c in C) >= 60
    assert sum(min(IC.inputs(c)["W"], IC.inputs(c)["H"]) < 16 for c in C) >= 10
    assert sum(max(IC.inputs(c)["W"], IC.inputs(c)["H"]) > 64 * 16 for c in C) >= 10
    for c in AB:
        assert int(IC.reference(c)["o"]["n_contrib"].max()) >= 60, c["id"]
    for c in C:   # the options drawn are the ones the fuzz is there for
        assert c["options"]["exp_mode"] in (0, 2, 3) and c["options"]["split"] == 1
    assert {c["options"]["binning"] for c in C} == {0, 1, 2, 3}
    assert {(c["options"]["fold"], c["options"]["cull"]) for c in C} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert sum(c["raw"] for c in C) >= 10
    assert any(IC.inputs(c)["scale_modifier"] != 1.0 and IC.has_aux(c) for c in C)


def _early_stops(o):
    """pixels of the oracle forward `o` that the T < 1e-4 test ended: walking on from the last contributor, the next record
    with alpha >= 1/255 takes the transmittance under 1e-4 (a blended record removes at most 99 %: final_T < 1e-2 there)"""
    import numpy as np
    gx, count = (o["W"] + 15) // 16, 0
    for y, x in zip(*np.nonzero(o["final_T"] < 1e-2)):
        lo, hi = (int(v) for v in o["ranges"][(y // 16) * gx + x // 16])
        for g in o["point_list"][lo + int(o["n_contrib"][y, x]):hi]:
            dx, dy = float(o["xy"][g, 0]) - x, float(o["xy"][g, 1]) - y
            a, b, c, op = (float(v) for v in o["conic_opacity"][g])
            power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
            alpha = min(0.99, op * np.exp(power)) if power <= 0.0 else 0.0
            if alpha >= 1.0 / 255.0:
                count += float(o["final_T"][y, x]) * (1.0 - alpha) < 1e-4
                break
    return count


def test_table_a_scenes_hold_what_they_are_there_for():
    """grids of 7 x 5 and 5 x 7 tiles, the T < 1e-4 early stop, and effective opacities on both sides of the 1/255 floor"""
    import _antialias_ref as AA
    for scene, grid in (("A1", (7, 5)), ("A2", (5, 7))):
        case = next(c for c in IC.TABLE_A if c["scene"] == scene and IC.has_aa(c))
        d, o = IC.inputs(case), IC.reference(case)["o"]
        assert ((d["W"] + 15) // 16, (d["H"] + 15) // 16) == grid
        assert _early_stops(o) > 0
        oe, vis = AA.o_eff(d), o["radii"] > 0
        assert ((oe < 1.0 / 255.0) & vis).sum() > 0 and ((oe >= 1.0 / 255.0) & vis).sum() > 0
