"""Host checks of tests/_planes_ref.py: the float64 restatement of the plane gather / scatter against torch's float64
sample_from_planes + autograd on every case of the table, the measurement of KAPPA (torch's own fp32 evaluation against
the restatement's budgets), and the self-checks that every case hits the edge it is named for."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd.decoder import sample_from_planes
import _planes_ref as R

GROUPS = ("A", "Bg", "Bs", "C", "D", "E", "F")


def _torch_eval(c, b, dtype):
    """sample_from_planes(planes * mod).mean(0) and the gradient w.r.t. planes in `dtype` on the CPU, non-finite rows left out"""
    fin = torch.isfinite(b.pos).all(1)
    p = b.planes.to(dtype).requires_grad_(True)
    src = p if b.mod is None else p * b.mod.to(dtype).t().reshape(-1)[None, :, None, None]   # channel index c * D + d
    out = sample_from_planes(src, b.pos[fin].to(dtype), c.box_warp, c.axes, c.D or None).mean(0)
    out.backward(b.gout[fin].to(dtype))
    return fin, out.detach(), p.grad


@functools.lru_cache(maxsize=None)
def _measure(grp):
    """(worst feature ratio, worst gradient ratio, case) of torch fp32 over a group; asserts the float64 agreement on the way"""
    worst = (0.0, 0.0, "")
    for c in R.group(grp):
        b = R.build(c)
        fin, f64, g64 = _torch_eval(c, b, torch.float64)
        feat, grad, fbud, gbud = R.reference(b.planes, b.pos[fin], b.gout[fin], c.box_warp, c.axes, c.D, b.mod)
        assert float((feat - f64).abs().max()) <= 1e-12, c.name
        assert float((grad - g64).abs().max()) <= 1e-11 * max(1.0, float(g64.abs().max())), c.name
        _, f32, g32 = _torch_eval(c, b, torch.float32)
        rf, rg = R.worst_ratio(f32, feat, fbud), R.worst_ratio(g32, grad, gbud)
        assert math.isfinite(rf) and math.isfinite(rg), f"{c.name}: torch fp32 is not exactly 0 where the budget is 0"
        if max(rf, rg) > max(worst[:2]):
            worst = (rf, rg, c.name)
    return worst


@pytest.mark.parametrize("grp", GROUPS)
def test_restatement_matches_torch_float64_and_fp32_torch_sits_inside_the_budget(grp):
    """(a) restatement vs torch float64: features <= 1e-12, gradients <= 1e-11 * max(1, gmax);  (b) torch fp32 vs the
    restatement: the worst (|err| - ATOL) / (2^-24 * budget) over the group, elements of zero budget exactly zero -- the
    measurement KAPPA comes from."""
    worst = _measure(grp)
    print(f"\n  group {grp}: worst fp32-torch / (2^-24 * budget): features {worst[0]:.3f}, gradients {worst[1]:.3f} ({worst[2]})")
    assert max(worst[:2]) <= R.KAPPA / 4.0


def test_kappa_is_four_times_the_measured_ratio_rounded_up():
    w = max(max(_measure(g)[:2]) for g in GROUPS)
    print(f"\n  worst fp32-reference ratio over the table: {w:.3f} -> KAPPA = ceil(4 * {w:.3f}) = {math.ceil(4.0 * w)}"
          f" (recorded: {R.KAPPA_MEASURED}, KAPPA = {R.KAPPA})")
    assert math.ceil(4.0 * w) == R.KAPPA          # neither tighter nor wider than 4 x what is measured here, rounded up
    assert R.KAPPA == math.ceil(4.0 * R.KAPPA_MEASURED)


@pytest.mark.parametrize("c", R.group("A"), ids=lambda c: c.name)
def test_an_infinite_coordinate_is_a_far_one(c):
    """A +-inf row has no tap on the planes that read that coordinate and every tap on the others: the same features as the
    +-1e30 row next to it (same other coordinates), and both within torch's reach through the finite one."""
    b = R.build(c)
    feat = R.reference_of(c)[0]
    inf = (~torch.isfinite(b.pos).all(1)).nonzero().squeeze(1)
    assert inf.numel() == 6
    for i in inf.tolist():
        a = int((~torch.isfinite(b.pos[i])).nonzero())
        twin = [j for j in range(b.pos.shape[0]) if abs(float(b.pos[j, a])) == float(np.float32(1e30)) and
                math.copysign(1.0, float(b.pos[j, a])) == math.copysign(1.0, float(b.pos[i, a]))
                and all(float(b.pos[j, k]) == float(b.pos[i, k]) for k in range(3) if k != a)]
        assert len(twin) == 1
        assert torch.equal(feat[i], feat[twin[0]])


@pytest.mark.parametrize("c", [c for c in R.CASES if c.taps_check], ids=lambda c: c.name)
def test_every_case_has_items_with_every_number_of_taps_inside(c):
    b = R.build(c)
    taps, _ = R.item_stats(b.pos, c.box_warp, c.axes, c.D, c.H, c.W)
    assert set(np.unique(taps).tolist()) == ({0, 1, 2, 4, 8} if c.D > 0 else {0, 1, 2, 4})


@pytest.mark.parametrize("c", R.group("D"), ids=lambda c: c.name)
def test_kept_item_cases_keep_exactly_that_many_items(c):
    """counted by sr_item's rule in float64 and in the kernel's own fp32 arithmetic"""
    b = R.build(c)
    assert b.pos.shape[0] == R.SR_MIN_POINTS
    for dt in (np.float64, np.float32):
        _, kept = R.item_stats(b.pos, c.box_warp, c.axes, c.D, c.H, c.W, dt)
        assert int(kept.sum()) == c.kept
    assert {c.kept for c in R.group("D")} == {0, 1, R.SR_CHUNK - 1, R.SR_CHUNK, R.SR_CHUNK + 1, 4 * R.SR_CHUNK - 1, 4 * R.SR_CHUNK,
                                              4 * R.SR_CHUNK + 1, 3 * R.SR_MIN_POINTS - 1}


def test_modulation_cases_sit_on_the_side_of_the_lds_limit_they_are_named_for():
    glob = [c for c in R.group("C") if "global" in c.name]
    lds = [c for c in R.group("C") if "lds" in c.name]
    assert len(glob) == 6 and len(lds) == 18
    assert all(c.mod and max(c.D, 1) * c.C > R.SR_MOD_LDS for c in glob)
    assert all(c.mod and max(c.D, 1) * c.C <= R.SR_MOD_LDS for c in lds)
    assert {(c.C, c.D) for c in glob} == {(64, 17), (32, 33), (16, 65)}


def test_switch_cases_share_their_points_on_both_sides():
    for c in R.group("C"):
        if c.N == R.SR_MIN_POINTS:
            lo = R.BY_NAME[c.name.replace(f"N{c.N}", f"N{c.N - 1}")]
            a, b = R.build(c), R.build(lo)
            assert lo.N == R.SR_MIN_POINTS - 1 and torch.equal(a.pos[:-1], b.pos) and torch.equal(a.gout[:-1], b.gout)
            assert torch.equal(a.planes, b.planes) and torch.isfinite(a.pos[-1]).all()


def test_lookback_case_launches_65_sort_tiles_and_keeps_64():
    c = R.BY_NAME["E-lookback-65-64"]
    b = R.build(c)
    for dt in (np.float64, np.float32):
        _, kept = R.item_stats(b.pos, c.box_warp, c.axes, c.D, c.H, c.W, dt)
        assert math.ceil(3 * c.N / R.SORT_TILE) == 65 and math.ceil(int(kept.sum()) / R.SORT_TILE) == 64
    assert int((b.pos == 5.0).all(1).sum()) == 700


def test_run_length_cases():
    one, same, short = (R.BY_NAME[n] for n in ("F-one-cell", "F-one-position", "F-short-runs"))
    for c in (one, same):
        b = R.build(c)
        E = R.edge_rows(c.box_warp, [8]).shape[0]
        rest = b.pos[E:]
        assert rest.shape[0] == R.SR_MIN_POINTS
        cell = torch.floor(((2.0 / c.box_warp * rest.double() + 1.0) * 8 - 1.0) / 2.0)
        assert bool((cell == cell[0, 0]).all())                       # one cell on every plane
        assert (torch.unique(rest, dim=0).shape[0] == 1) == (c is same)
    b = R.build(short)
    x = torch.floor(((2.0 / short.box_warp * b.pos.double() + 1.0) * 256 - 1.0) / 2.0)
    key = x[:, 0] * 1000 + x[:, 1]
    _, counts = torch.unique(key[torch.isfinite(key)], return_counts=True)
    assert float((counts <= 2).double().mean()) > 0.8               # plane 0: most cells hold one or two points
