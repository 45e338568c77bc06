"""Density control, host side: the one-pass plan equals the sequential op order bit for bit (tests/_densify_ref.py), the
C ABI carries the new entry points, the position schedule matches its closed form, and arguments are checked."""
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

from _densify_ref import DEGENERATE, KEYS, Rule, degenerate_case, make_case, one_pass, sequential
from gaussian_gan_decoder_amd.gaussian_model import GaussianModel, get_expon_lr_func

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ggd_densify_tmp_bytes", "ggd_densify_stats", "ggd_densify_plan", "ggd_prune_plan", "ggd_densify_emit",
               "ggd_densify_gather")


def training_args(**over):
    a = dict(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
             position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
    a.update(over)
    return SimpleNamespace(**a)


def cpu_model(P=5, sh_degree=1, spatial_lr_scale=2.0):
    pc = GaussianModel(sh_degree)
    M = (sh_degree + 1) ** 2
    g = torch.Generator().manual_seed(0)
    shapes = {"_xyz": (P, 3), "_features_dc": (P, 1, 3), "_features_rest": (P, M - 1, 3), "_opacity": (P, 1),
              "_scaling": (P, 3), "_rotation": (P, 4)}
    for attr, shape in shapes.items():
        setattr(pc, attr, torch.nn.Parameter(torch.randn(shape, generator=g)))
    pc.spatial_lr_scale = spatial_lr_scale
    return pc


def assert_same_state(a, b):
    assert set(a) == set(b) == set(KEYS)
    for k in KEYS:
        assert a[k].shape == b[k].shape, k
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("M", [1, 4, 16])
@pytest.mark.parametrize("screen", [None, 20])
def test_one_pass_equals_sequential_on_random_cases(M, screen):
    rule = Rule(max_screen_size=screen)
    seen = [0, 0, 0]
    for seed, P in enumerate((1, 2, 63, 257, 700, 1500)):
        case = make_case(P, M, 100 * M + seed, rule)
        got, counts = one_pass(case, rule)
        assert_same_state(got, sequential(case, rule))
        assert got["xyz"].shape[0] == counts[0] + counts[1] + 2 * counts[2]
        seen = [a + b for a, b in zip(seen, counts)]
    assert all(seen), f"the cases never exercised a segment: {seen}"


@pytest.mark.parametrize("kind", DEGENERATE)
@pytest.mark.parametrize("screen", [None, 20])
def test_one_pass_equals_sequential_on_degenerate_plans(kind, screen):
    rule = Rule(max_screen_size=screen)
    P = 300
    case = degenerate_case(kind, P, 4, 7, rule)
    got, counts = one_pass(case, rule)
    assert_same_state(got, sequential(case, rule))
    if kind == "identity":
        assert counts == (P, 0, 0) and torch.equal(got["xyz"], case["xyz"]) and torch.equal(got["f_rest.m1"], case["f_rest.m1"])
    if kind == "all_cloned":
        assert counts == (P, P, 0) and not got["xyz.m2"][P:].any()
    if kind == "all_split":
        assert counts == (0, 0, P) and not got["scaling.m1"].any()
    if kind == "all_pruned":
        assert counts == (0, 0, 0) and got["f_rest"].shape == (0, 3, 3)
    if kind == "unseen":
        assert counts[1] == counts[2] == 0 and 0 < counts[0] < P


def test_new_symbols_are_declared_and_exported(native_lib):
    from gaussian_gan_decoder_amd import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggd_raster.h")).read(), flags=re.S)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", hdr), f"{sym} is not declared in ggd_raster.h"
        assert sym in _capi.EXPORTS and hasattr(native_lib, sym), sym
    per_row = native_lib.ggd_densify_tmp_bytes(1_000_000) / 1e6
    assert 9.0 <= per_row <= 10.0                       # a flag byte and at most two source-map words per row
    assert native_lib.ggd_densify_tmp_bytes(-1) == 0 and native_lib.ggd_densify_tmp_bytes((1 << 26) + 1) == 0
    assert native_lib.ggd_densify_tmp_bytes(0) > 0


def test_library_rejects_bad_arguments_without_a_device(native_lib):
    """ctx == NULL is refused before anything else (the other argument checks need a context: tests/test_densify_gpu.py)."""
    assert native_lib.ggd_densify_stats(None, None, 4, None, None, None, None, None, None) != 0
    assert native_lib.ggd_densify_plan(None, None, 4, None, None, None, None, 0.1, 0.1, 0.1, 0, 0.1, None, 0, None) != 0
    assert native_lib.ggd_prune_plan(None, None, 4, None, None, 0, None) != 0
    assert native_lib.ggd_densify_emit(None, None, 4, 4, 1, None, None, None, None, 0) != 0
    assert native_lib.ggd_densify_gather(None, None, 4, 4, 1, None, None, None, 0) != 0


@pytest.mark.parametrize("step", [0, 1, 100, 15_000, 30_000, 40_000])
def test_update_learning_rate_matches_the_closed_form(step):
    pc = cpu_model()
    args = training_args()
    pc.training_setup(args)
    lr0, lr1 = args.position_lr_init * pc.spatial_lr_scale, args.position_lr_final * pc.spatial_lr_scale
    t = min(step / args.position_lr_max_steps, 1.0)
    expect = lr0 ** (1 - t) * lr1 ** t                   # log-linear; no delay steps are configured, so no delay factor
    got = pc.update_learning_rate(step)
    assert got == pytest.approx(expect, rel=1e-12)
    assert [g["lr"] for g in pc.optimizer.param_groups if g["name"] == "xyz"] == [got]
    if step == 0:
        assert got == pytest.approx(lr0, rel=1e-12)
    if step >= args.position_lr_max_steps:
        assert got == pytest.approx(lr1, rel=1e-12)


def test_expon_lr_func_edge_cases():
    assert get_expon_lr_func(1e-2, 1e-4)(-1) == 0.0
    assert get_expon_lr_func(0.0, 0.0)(10) == 0.0
    f = get_expon_lr_func(1e-2, 1e-4, lr_delay_steps=100, lr_delay_mult=0.01, max_steps=1000)
    assert f(0) == pytest.approx(1e-2 * 0.01, rel=1e-12)
    assert f(50) == pytest.approx((0.01 + 0.99 * math.sin(0.25 * math.pi)) * 1e-2 ** 0.95 * 1e-4 ** 0.05, rel=1e-12)
    assert f(100) == pytest.approx(1e-2 ** 0.9 * 1e-4 ** 0.1, rel=1e-12)
    assert f(5000) == pytest.approx(1e-4, rel=1e-12)


def test_training_setup_groups_rates_and_statistics():
    pc = cpu_model(P=5)
    assert pc.optimizer is None and pc.percent_dense == 0
    args = training_args()
    pc.training_setup(args, decoder_params=[{"params": [torch.nn.Parameter(torch.zeros(2))], "lr": 0.5, "name": "pre_offset_decoder"}])
    groups = pc.optimizer.param_groups
    assert [g["name"] for g in groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "pre_offset_decoder"]
    assert [g["lr"] for g in groups] == [0.00016 * 2.0, 0.0025, 0.0025 / 20.0, 0.05, 0.005, 0.001, 0.5]
    assert all(g["eps"] == 1e-15 for g in groups) and isinstance(pc.optimizer, torch.optim.Adam)
    assert groups[0]["params"][0] is pc._xyz and groups[2]["params"][0] is pc._features_rest
    assert pc.percent_dense == 0.01
    for t in (pc.xyz_gradient_accum, pc.denom):
        assert t.shape == (5, 1) and t.device == pc._xyz.device and not t.any()


def test_reset_opacity_and_replace_tensor_rekey_the_optimizer_state():
    """The torch-only part of the bookkeeping runs on the CPU: new nn.Parameter, state re-keyed, moments zeroed, step kept."""
    pc = cpu_model(P=6)
    pc.training_setup(training_args())
    sum(p.sum() for p in (pc._xyz, pc._opacity, pc._scaling)).backward()
    pc.optimizer.step()
    pc.optimizer.step()
    old, old_xyz = pc._opacity, pc._xyz
    before = torch.sigmoid(old.detach())
    step = pc.optimizer.state[old]["step"]
    pc.reset_opacity()
    new = pc._opacity
    assert new is not old and isinstance(new, torch.nn.Parameter) and new.requires_grad
    assert old not in pc.optimizer.state and len(pc.optimizer.state) == 3
    state = pc.optimizer.state[new]
    assert state["step"] == step == 2 and not state["exp_avg"].any() and not state["exp_avg_sq"].any()
    assert [g["params"][0] for g in pc.optimizer.param_groups if g["name"] == "opacity"] == [new]
    assert torch.allclose(torch.sigmoid(new.detach()), torch.clamp(before, max=0.01), rtol=1e-5, atol=0)
    assert pc._xyz is old_xyz and pc.optimizer.state[old_xyz]["exp_avg"].any()
    out = pc.replace_tensor_to_optimizer(torch.ones(6, 3), "xyz")
    assert out["xyz"] is pc._xyz and pc._xyz is not old_xyz and not pc.optimizer.state[pc._xyz]["exp_avg"].any()
    pc.optimizer.zero_grad()
    pc._xyz.sum().backward()
    pc.optimizer.step()                                   # the optimizer still steps the swapped parameter
    assert pc.optimizer.state[pc._xyz]["step"] == 3


def test_capture_restore_round_trip_on_the_cpu():
    pc = cpu_model(P=4)
    pc.training_setup(training_args())
    pc._xyz.sum().backward()
    pc.optimizer.step()
    pc.xyz_gradient_accum += 1.5
    pc.max_radii2D = torch.arange(4.0)
    snap = pc.capture()
    assert len(snap) == 12
    other = GaussianModel(1)
    other.restore(snap, training_args())
    assert other._xyz is pc._xyz and torch.equal(other.xyz_gradient_accum, pc.xyz_gradient_accum)
    assert torch.equal(other.max_radii2D, torch.arange(4.0)) and other.spatial_lr_scale == 2.0
    assert torch.equal(other.optimizer.state[other._xyz]["exp_avg"], pc.optimizer.state[pc._xyz]["exp_avg"])


def test_kernel_backed_methods_refuse_cpu_tensors():
    pc = cpu_model(P=4)
    pc.training_setup(training_args())
    vs = torch.zeros(4, 3, requires_grad=True)
    vs.sum().backward()
    calls = [lambda: pc.add_densification_stats(vs, torch.ones(4, dtype=torch.bool)),
             lambda: pc.update_densification_stats(vs, torch.ones(4, dtype=torch.int32)),
             lambda: pc.densify_and_prune(0.0002, 0.005, 4.0, None),
             lambda: pc.prune_points(torch.zeros(4, dtype=torch.bool))]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert pc._xyz.shape[0] == 4
