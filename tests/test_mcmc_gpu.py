"""MCMC density control on the device (csrc/ggd_mcmc.hip through GaussianModel and mcmc.compute_relocation) against
tests/_mcmc_ref.py: the integer sampling plan exactly, copied data and moments bit for bit, the relocation values and the
position noise against float64 under the bars derived in _mcmc_ref.py, and a short fit under a row budget.

Row counts: 1, 63 / 64 / 65 (a wave), 2047 / 2048 / 2049 (one scan tile of the plan), 3 * 2048 + 7 and 20 011 (several
workgroups, several tiles in the tile search).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _mcmc_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 7, 20_011)
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ATTRS = dict(zip(NAMES, ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")))
COPIED = ("xyz", "f_dc", "f_rest", "rotation")
TOP = (1 << 32) - 1


def training_args(**over):
    a = dict(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
             position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001)
    a.update(over)
    return SimpleNamespace(**a)


def make_case(P, M, seed, dead="mixed"):
    """Parameters and moments of P rows; raw opacities with o >= 0.011 on alive and o <= 0.0037 on dead rows: an ulp of the
    device's sigmoid cannot move a row across 0.005."""
    gen = torch.Generator().manual_seed(seed)
    shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, M - 1, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
    case = {n: torch.randn(s, generator=gen) for n, s in shapes.items()}
    case["scaling"] = -7.0 + 8.0 * torch.rand((P, 3), generator=gen)
    is_dead = {"mixed": torch.rand(P, generator=gen) < 0.3, "none": torch.zeros(P, dtype=torch.bool),
               "all": torch.ones(P, dtype=torch.bool)}[dead]
    u = torch.rand((P, 1), generator=gen)
    case["opacity"] = torch.where(is_dead[:, None], -9.0 + 3.4 * u, -4.5 + 10.5 * u)
    for n, s in shapes.items():
        case[n + ".m1"], case[n + ".m2"] = torch.randn(s, generator=gen), torch.rand(s, generator=gen)
    case["dead"] = is_dead
    case["draws"] = torch.randint(0, 1 << 32, (P,), generator=gen, dtype=torch.int64)
    return case


def model_of(case, M, moments=True, optimizer_type="default"):
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel
    pc = GaussianModel({1: 0, 4: 1, 9: 2, 16: 3}[M])
    for n, attr in ATTRS.items():
        setattr(pc, attr, torch.nn.Parameter(case[n].clone().to(DEV)))
    pc.spatial_lr_scale = 1.0
    pc.training_setup(training_args(optimizer_type=optimizer_type))
    P = case["xyz"].shape[0]
    pc.max_radii2D = torch.full((P,), 7.0, device=DEV)
    pc.xyz_gradient_accum, pc.denom = torch.full((P, 1), 3.0, device=DEV), torch.full((P, 1), 2.0, device=DEV)
    if moments:
        for attr in ATTRS.values():
            getattr(pc, attr).grad = torch.zeros_like(getattr(pc, attr))
        torch.optim.Adam.step(pc.optimizer)               # zero gradients: the parameters do not move, the state exists
        pc.optimizer.zero_grad(set_to_none=True)
        for n, attr in ATTRS.items():
            st = pc.optimizer.state[getattr(pc, attr)]
            st["exp_avg"], st["exp_avg_sq"] = case[n + ".m1"].clone().to(DEV), case[n + ".m2"].clone().to(DEV)
    return pc


def state_on_host(pc, moments=True):
    out = {}
    for n, attr in ATTRS.items():
        p = getattr(pc, attr)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad
        out[n] = p.detach().cpu()
        if moments:
            st = pc.optimizer.state[p]
            assert int(st["step"]) == 1
            out[n + ".m1"], out[n + ".m2"] = st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()
    assert len(pc.optimizer.state) == (6 if moments else 0)
    assert [g["params"][0] for g in pc.optimizer.param_groups] == [getattr(pc, a) for a in ATTRS.values()]
    return out


def poisoned(pc):
    from gaussian_gan_decoder_amd import _capi
    cx = _capi.context_for(pc._xyz.device)

    class Scope:
        def __enter__(self):
            cx.poison_outputs = True

        def __exit__(self, *exc):
            cx.poison_outputs = False
    return Scope()


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def check_weights(plan, case, dead, what):
    w = plan["weights"].cpu().numpy()
    o = sigmoid64(case["opacity"].numpy().reshape(-1))
    want = np.maximum(1, np.rint(o * R.WEIGHT_ONE))
    dead = dead.numpy().astype(bool)
    assert (w[dead] == 0).all() and (w[~dead] >= 1).all(), what
    assert (np.abs(w[~dead] - want[~dead]) <= 1).all(), what
    return [int(v) for v in w]


def check_values(got, case, rows, src, N, what):
    """Raw opacity and raw scales of `rows` (tensor of output rows) against the float64 rule on the sources' fp32 inputs."""
    if len(rows) == 0:
        return
    x = case["opacity"].numpy().reshape(-1)[src]
    raw64, s64, cond = R.raw_values64(x, case["scaling"].numpy()[src], N)
    bar = R.ATOL + R.C_REL * R.EPS32 * cond
    err_o = np.abs(got["opacity"].numpy().reshape(-1)[rows].astype(np.float64) - raw64)
    err_s = np.abs(got["scaling"].numpy()[rows].astype(np.float64) - s64)
    assert (err_o <= bar).all(), (what, float((err_o / bar).max()))
    assert (err_s <= bar[:, None]).all(), (what, float((err_s / bar[:, None]).max()))
    sig = sigmoid64(got["opacity"].numpy().reshape(-1)[rows])
    assert sig.min() >= R.O_MIN and sig.max() <= R.O_MAX, (what, sig.min(), sig.max())   # the clamps, exactly
    return float((err_o / bar).max()), float((err_s / bar[:, None]).max())


def check_relocated(pc, case, M, dead, plan, draws, objects, what):
    P = case["xyz"].shape[0]
    weights = check_weights(plan, case, dead, what)
    dead_rows = [int(j) for j in torch.nonzero(dead).reshape(-1)]
    sources, counts = R.sample_sources(weights, {j: int(draws[j]) for j in dead_rows})
    got_src, got_cnt = plan["sources"].cpu().tolist(), plan["counts"].cpu().tolist()
    assert got_cnt == counts, what
    assert [got_src[j] for j in dead_rows] == sources and all(got_src[j] == -1 for j in range(P) if not dead[j]), what
    got = state_on_host(pc)
    assert [getattr(pc, a) for a in ATTRS.values()] == objects, what          # in place: the same nn.Parameters
    if sum(weights) == 0 or not dead_rows:
        for k in got:
            assert torch.equal(got[k], case[k]), (what, k, "a no-op changed the state")
        return
    dst, src = torch.tensor(dead_rows), torch.tensor(sources)
    sampled = torch.tensor([c > 0 for c in counts])
    untouched = ~sampled & ~dead
    for n in NAMES:
        assert not torch.isnan(got[n]).any()
        if n in COPIED:
            assert torch.equal(got[n][dst], case[n][src]), (what, n, "a destination is not a copy of its source")
            assert torch.equal(got[n][~dead], case[n][~dead]), (what, n)
        else:
            assert torch.equal(got[n][untouched], case[n][untouched]), (what, n)
            assert torch.equal(got[n][dst], got[n][src]), (what, n, "source and copy differ")
        for m in (".m1", ".m2"):
            assert not got[n + m][sampled].any(), (what, n + m, "a sampled source kept a moment")
            assert torch.equal(got[n + m][~sampled], case[n + m][~sampled]), (what, n + m)   # (destinations keep theirs)
    rows = torch.nonzero(sampled).reshape(-1).numpy()
    N = np.minimum(R.N_MAX, 1 + np.array(counts)[rows])
    return check_values(got, case, rows, rows, N, what)


@pytest.mark.parametrize("M", [1, 4, 16])
def test_relocate_matches_the_plan_and_the_float64_values(M):
    worst = (0.0, 0.0)
    for P in SIZES:
        case = make_case(P, M, 100 * M + P)
        dead, draws = case["dead"], case["draws"]
        hit = torch.nonzero(dead).reshape(-1)[:2]
        draws[hit] = torch.tensor([0, TOP])[:len(hit)]                          # the two ends of the weight line
        pc = model_of(case, M)
        objects = [getattr(pc, a) for a in ATTRS.values()]
        with poisoned(pc):
            plan = pc.relocate_gs(draws=draws.to(DEV), return_plan=True)        # the device's own dead rule
        res = check_relocated(pc, case, M, dead, plan, draws, objects, f"P={P} M={M}")
        if res:
            worst = tuple(max(a, b) for a, b in zip(worst, res))
        for t, v, shape in ((pc.xyz_gradient_accum, 3.0, (P, 1)), (pc.denom, 2.0, (P, 1)), (pc.max_radii2D, 7.0, (P,))):
            assert tuple(t.shape) == shape and bool((t == v).all())
    print(f"relocate M={M}: worst error / bar: opacity {worst[0]:.3f}, scales {worst[1]:.3f}")


@pytest.mark.parametrize("kind", ["none", "all"])
def test_relocate_without_dead_or_without_alive_rows_changes_nothing(kind):
    for P in (1, 2049):
        case = make_case(P, 4, 7 + P, dead=kind)
        pc = model_of(case, 4)
        objects = [getattr(pc, a) for a in ATTRS.values()]
        with poisoned(pc):
            plan = pc.relocate_gs(draws=case["draws"].to(DEV), return_plan=True)
        check_relocated(pc, case, 4, case["dead"], plan, case["draws"], objects, f"{kind} P={P}")
        assert not plan["counts"].any() and bool((plan["sources"] == -1).all())


def test_one_alive_row_with_more_than_fifty_dead_clamps_the_ratio():
    P, alive = 65, 17
    case = make_case(P, 4, 3, dead="all")
    case["dead"][alive] = False
    case["opacity"][alive] = 2.0
    pc = model_of(case, 4)
    objects = [getattr(pc, a) for a in ATTRS.values()]
    with poisoned(pc):
        plan = pc.relocate_gs(draws=case["draws"].to(DEV), return_plan=True)
    assert int(plan["counts"][alive]) == P - 1 and bool((plan["sources"].cpu()[case["dead"]] == alive).all())
    check_relocated(pc, case, 4, case["dead"], plan, case["draws"], objects, "one alive")        # (its values: N = min(51, 65))
    got = state_on_host(pc)
    assert torch.equal(got["opacity"], got["opacity"][alive].expand(P, 1)) and torch.equal(got["xyz"], case["xyz"][alive].expand(P, 3))


def test_an_explicit_dead_mask_replaces_the_device_rule():
    P, M = 3 * 2048 + 7, 4
    case = make_case(P, M, 11)
    mask = torch.rand(P, generator=torch.Generator().manual_seed(5)) < 0.2      # unrelated to the opacities
    pc = model_of(case, M)
    objects = [getattr(pc, a) for a in ATTRS.values()]
    with poisoned(pc):
        plan = pc.relocate_gs(dead_mask=mask.to(DEV), draws=case["draws"].to(DEV), return_plan=True)
    check_relocated(pc, case, M, mask, plan, case["draws"], objects, "explicit mask")
    by_rule, by_mask = model_of(case, M), model_of(case, M)
    by_rule.relocate_gs(draws=case["draws"].to(DEV))
    by_mask.relocate_gs(dead_mask=case["dead"].to(DEV).view(torch.uint8), draws=case["draws"].to(DEV))
    a, b = state_on_host(by_rule), state_on_host(by_mask)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["xyz"], case["xyz"])


def targeted_draws(weights, want):
    """want: {source row: times} -> list of draws, each the smallest one whose tau is the first unit of its source's interval."""
    W, start, run = sum(weights), [], 0
    for w in weights:
        start.append(run)
        run += w
    out = []
    for s, times in want.items():
        d = -(-(start[s] << 32) // W)
        assert (d * W) >> 32 == start[s] and weights[s] > 0
        out += [d] * times
    return out


def test_values_over_the_opacity_ladder_and_every_ratio():
    """o from 0.005 to 1 - 1e-6 against N = 1 .. 51: one alive row per (o, N), drawn N - 1 times by draws aimed at it."""
    x, s, N = R.value_inputs()
    A = x.size
    D = int((N - 1).sum())
    P, M = A + D, 1
    case = make_case(P, M, 21, dead="all")
    case["dead"][:A] = False
    case["opacity"][:A, 0] = torch.from_numpy(x)
    case["scaling"][:A] = torch.from_numpy(s)
    mask = case["dead"].to(DEV)
    weights = [int(v) for v in model_of(case, M).relocate_gs(dead_mask=mask, return_plan=True)["weights"].cpu()]
    draws = torch.zeros(P, dtype=torch.int64)
    draws[A:] = torch.tensor(targeted_draws(weights, {i: int(N[i]) - 1 for i in range(A)}))
    pc = model_of(case, M)
    objects = [getattr(pc, a) for a in ATTRS.values()]
    with poisoned(pc):
        plan = pc.relocate_gs(dead_mask=mask, draws=draws.to(DEV), return_plan=True)
    assert plan["counts"][:A].cpu().tolist() == [int(n) - 1 for n in N]
    res = check_relocated(pc, case, M, case["dead"], plan, draws, objects, "ladder")
    print(f"ladder: worst error / bar: opacity {res[0]:.3f}, scales {res[1]:.3f}")
    got = state_on_host(pc)
    once = N == 1
    assert torch.equal(got["opacity"][:A][once], case["opacity"][:A][once]) and torch.equal(got["scaling"][:A][once], case["scaling"][:A][once])
    clamped = sigmoid64(got["opacity"][:A].numpy().reshape(-1))
    assert (clamped <= R.O_MIN * (1 + 1e-6)).sum() >= 50                        # the ladder does reach the lower clamp


def test_compute_relocation_on_activated_values():
    from gaussian_gan_decoder_amd import _capi
    from gaussian_gan_decoder_amd.mcmc import compute_relocation
    x, s_raw, N = R.value_inputs()
    o32 = sigmoid64(x).astype(np.float32)
    s32 = np.exp(s_raw)
    op64, coeff64, cond = R.relocation64(o32.astype(np.float64), N)
    cx = _capi.context_for(torch.device(DEV))
    cx.poison_outputs = True
    try:
        new_o, new_s = compute_relocation(torch.from_numpy(o32).to(DEV)[:, None], torch.from_numpy(s32).to(DEV),
                                          torch.from_numpy(N).to(DEV)[:, None], None, 51)
        same = compute_relocation(torch.from_numpy(o32).to(DEV), torch.from_numpy(s32).to(DEV), torch.from_numpy(N).int().to(DEV))
        over = compute_relocation(torch.from_numpy(o32).to(DEV), torch.from_numpy(s32).to(DEV), torch.from_numpy(N + 60).to(DEV))
        none = compute_relocation(torch.zeros(0, device=DEV), torch.zeros((0, 3), device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV))
    finally:
        cx.poison_outputs = False
    assert new_o.shape == (x.size, 1) and new_s.shape == (x.size, 3) and none[0].shape == (0,) and none[1].shape == (0, 3)
    assert torch.equal(new_o.reshape(-1), same[0]) and torch.equal(new_s, same[1])
    top = N == R.N_MAX
    assert torch.equal(over[0].cpu()[top], same[0].cpu()[top]) and torch.equal(over[1].cpu()[top], same[1].cpu()[top])   # ratios clamp at 51
    bar = R.ATOL + R.C_REL * R.EPS32 * cond
    err_o = np.abs(np.log(new_o.cpu().numpy().reshape(-1).astype(np.float64)) - np.log(op64))
    err_s = np.abs(np.log(new_s.cpu().numpy().astype(np.float64)) - np.log(s32.astype(np.float64) * coeff64[:, None]))
    print(f"compute_relocation: worst error / bar: opacity {(err_o / bar).max():.3f}, scales {(err_s / bar[:, None]).max():.3f}")
    assert (err_o <= bar).all() and (err_s <= bar[:, None]).all()
    once = N == 1
    assert torch.equal(new_o.cpu().reshape(-1)[once], torch.from_numpy(o32)[once]) and torch.equal(new_s.cpu()[once], torch.from_numpy(s32)[once])


@pytest.mark.parametrize("M", [1, 4, 16])
def test_add_new_gs_grows_to_the_budget(M):
    for P in SIZES:
        case = make_case(P, M, 300 * M + P, dead="none")
        want = int(1.05 * P)
        for cap in (10 * P + 10, P + 3, P):
            target = min(cap, want)
            num = max(0, target - P)
            pc = model_of(case, M)
            objects = [getattr(pc, a) for a in ATTRS.values()]
            draws = torch.randint(0, 1 << 32, (num,), generator=torch.Generator().manual_seed(P + cap), dtype=torch.int64)
            if num >= 2:
                draws[:2] = torch.tensor([0, TOP])
            with poisoned(pc):
                added, plan = pc.add_new_gs(cap, draws=draws.to(DEV), return_plan=True)
            what = f"P={P} M={M} cap={cap}"
            assert added == num and pc.get_xyz.shape[0] == max(P, target), what
            got = state_on_host(pc)
            if num == 0:
                assert plan is None and [getattr(pc, a) for a in ATTRS.values()] == objects, what
                assert all(torch.equal(got[k], case[k]) for k in got), what
                continue
            assert all(new is not old for new, old in zip((getattr(pc, a) for a in ATTRS.values()), objects)), what
            weights = check_weights(plan, case, case["dead"], what)
            sources, counts = R.sample_sources(weights, [int(d) for d in draws])
            assert plan["sources"].cpu().tolist() == sources and plan["counts"].cpu().tolist() == counts, what
            if num >= 2:
                assert sources[0] == 0 and sources[1] == P - 1, what
            src, sampled = torch.tensor(sources), torch.tensor([c > 0 for c in counts])
            for n in NAMES:
                assert got[n].shape[0] == P + num and not torch.isnan(got[n]).any(), (what, n)
                if n in COPIED:
                    assert torch.equal(got[n][:P], case[n]) and torch.equal(got[n][P:], case[n][src]), (what, n)
                else:
                    assert torch.equal(got[n][:P][~sampled], case[n][~sampled]) and torch.equal(got[n][P:], got[n][src]), (what, n)
                for m in (".m1", ".m2"):
                    assert not torch.isnan(got[n + m]).any() and not got[n + m][P:].any() and not got[n + m][:P][sampled].any(), (what, n + m)
                    assert torch.equal(got[n + m][:P][~sampled], case[n + m][~sampled]), (what, n + m)
            rows = torch.nonzero(sampled).reshape(-1).numpy()
            check_values(got, case, rows, rows, np.minimum(R.N_MAX, 1 + np.array(counts)[rows]), what)
            for t, v, shape in ((pc.xyz_gradient_accum, 3.0, (P + num, 1)), (pc.denom, 2.0, (P + num, 1)), (pc.max_radii2D, 7.0, (P + num,))):
                assert tuple(t.shape) == shape and bool((t[:P] == v).all()) and not t[P:].any(), what


def test_before_the_first_step_there_are_no_moments_to_zero():
    case = make_case(2049, 4, 9)
    pc = model_of(case, 4, moments=False)
    pc.relocate_gs(draws=case["draws"].to(DEV))
    got = state_on_host(pc, moments=False)
    dead = case["dead"]
    assert torch.equal(got["xyz"][~dead], case["xyz"][~dead]) and not torch.equal(got["xyz"][dead], case["xyz"][dead])
    assert pc.add_new_gs(5000) == int(1.05 * 2049) - 2049 and state_on_host(pc, moments=False)["f_rest"].shape == (2151, 3, 3)
    assert pc.add_new_gs(2151) == 0
    with pytest.raises(ValueError, match="draws"):
        pc.relocate_gs(draws=torch.zeros(3, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.relocate_gs(draws=torch.zeros(2151, dtype=torch.int64))
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel
    fresh = GaussianModel(1)
    for n, attr in ATTRS.items():
        setattr(fresh, attr, torch.nn.Parameter(case[n].clone().to(DEV)))
    for call in (fresh.relocate_gs, lambda: fresh.add_new_gs(5000), lambda: fresh.inject_position_noise(1.0)):
        with pytest.raises(ValueError, match="training_setup"):
            call()


def test_position_noise_against_float64():
    noise_lr, xyz_lr = 5e5, 1.6e-4
    worst = 0.0
    for P in SIZES:
        s, q, x, xi = R.noise_inputs(P, P)
        case = make_case(P, 4, P, dead="none")
        case.update(scaling=s, rotation=q, opacity=x)
        pc = model_of(case, 4)
        objects = [getattr(pc, a) for a in ATTRS.values()]
        pc.inject_position_noise(noise_lr, xyz_lr, noise=xi.to(DEV))
        got = state_on_host(pc)
        assert [getattr(pc, a) for a in ATTRS.values()] == objects
        for k in got:
            if k != "xyz":
                assert torch.equal(got[k], case[k]), (P, k)
        ref = R.noise64(s, q, x, xi, noise_lr, xyz_lr)
        moved = got["xyz"].double() - case["xyz"].double()
        # the device adds in fp32: half an ulp of the position is not the kernel's error
        slack = (case["xyz"].abs() + ref.abs().float()).double().amax(dim=1) * 2.0 ** -23
        err = (moved - ref).abs().amax(dim=1)
        bar = R.NOISE_RTOL * ref.abs().amax(dim=1) + slack
        worst = max(worst, float((err / bar).max()))
        assert bool((err <= bar).all()), (P, float((err / bar).max()))
        if P >= 8:
            gate = torch.sigmoid(100 * (torch.sigmoid(-x.double().reshape(-1)) - 0.995))
            assert bool(((gate[:2] > 0.5) & (gate[:2] < 1)).all()) and bool((moved[:2].abs().amax(dim=1) > 0).all())
            assert bool((moved[2:4].abs().amax(dim=1) < R.NOISE_RTOL * torch.exp(s[2:4]).amin(dim=1)).all())   # o = 0.5 stays
        lr_model = model_of(case, 4)
        lr_model.update_learning_rate(100)
        rate = lr_model._own_groups()["xyz"]["lr"]
        explicit = model_of(case, 4)
        lr_model.inject_position_noise(noise_lr, noise=xi.to(DEV))               # xyz_lr=None: the group's current rate
        explicit.inject_position_noise(noise_lr, rate, noise=xi.to(DEV))
        assert torch.equal(lr_model._xyz, explicit._xyz) and 0 < rate < 0.00016
    print(f"noise: worst error / bar {worst:.3f}")
    drawn = model_of(case, 4)
    drawn.inject_position_noise(noise_lr, xyz_lr)
    delta = (drawn._xyz.detach().cpu() - case["xyz"]).abs().amax(dim=1)
    assert torch.isfinite(delta).all() and int((delta > 0).sum()) > P // 100
    with pytest.raises(ValueError, match="noise"):
        drawn.inject_position_noise(noise_lr, xyz_lr, noise=torch.zeros(3, 3, device=DEV))


@pytest.mark.parametrize("optimizer_type", ["default", "sparse_adam"])
def test_short_fit_under_a_budget(optimizer_type):
    """400 seeded Gaussians, a 64 x 64 target, 16 iterations: render, backward, relocate + add every 4, step, noise.  The row
    count grows by 5 % a time and stops at the budget."""
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel
    from gaussian_gan_decoder_amd.gaussian_renderer import render
    from gaussian_gan_decoder_amd.mcmc import mcmc_regularizers
    from gaussian_gan_decoder_amd.synthetic import make_scene
    pipe = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    sc = make_scene(4000, 64, "cube", seed=3, log_scale_mean=-4.0).to(DEV)
    with torch.no_grad():
        target = render(sc.cam, sc.gaussian_model(), pipe, sc.bg)["render"].clone()
    gen = torch.Generator().manual_seed(0)
    pc = GaussianModel(1)
    pc.create_from_pos_col((torch.rand((400, 3), generator=gen) - 0.5).to(DEV), torch.rand((400, 3), generator=gen).to(DEV))
    pc.oneupSHdegree()
    pc.training_setup(training_args(position_lr_init=0.002, position_lr_final=0.0002, feature_lr=0.02, opacity_lr=0.1,
                                    scaling_lr=0.01, optimizer_type=optimizer_type))
    cap, sizes, want = 450, [400], [400]
    for _ in range(4):
        want.append(min(cap, int(1.05 * want[-1])))
    with torch.no_grad():
        pc._opacity[:40] = -7.0                            # some rows start dead
    for it in range(1, 17):
        pc.update_learning_rate(it)
        out = render(sc.cam, pc, pipe, sc.bg)
        loss = (out["render"] - target).abs().mean() + mcmc_regularizers(pc)
        loss.backward()
        with torch.no_grad():
            if it % 4 == 0:
                steps = {a: int(pc.optimizer.state[getattr(pc, a)]["step"]) for a in ATTRS.values() if getattr(pc, a) in pc.optimizer.state}
                plan = pc.relocate_gs(return_plan=True)
                if it == 4:
                    assert int(plan["counts"].sum()) >= 30
                grads = {a: getattr(pc, a).grad for a in ATTRS.values()}
                added = pc.add_new_gs(cap)
                sizes.append(pc.get_xyz.shape[0])
                assert added == sizes[-1] - sizes[-2]
                for a in ATTRS.values():
                    p = getattr(pc, a)
                    if p in pc.optimizer.state:
                        st = pc.optimizer.state[p]
                        assert st["exp_avg"].shape == p.shape == st["exp_avg_sq"].shape and int(st["step"]) == steps[a]
                if added:                                 # the gradients belong to the old parameters: this iteration takes no step
                    pc.optimizer.zero_grad(set_to_none=True)
                    continue
                assert all(getattr(pc, a).grad is grads[a] for a in ATTRS.values())
            if optimizer_type == "sparse_adam":
                pc.optimizer.step(out["radii"], pc.get_xyz.shape[0])
            else:
                pc.optimizer.step()
            pc.optimizer.zero_grad(set_to_none=True)
            pc.inject_position_noise(5e4)
            for a in ATTRS.values():
                assert bool(torch.isfinite(getattr(pc, a)).all()), (it, a)
    print(f"fit ({optimizer_type}): rows {sizes}, last loss {loss.item():.5f}")
    assert sizes == want and want[1] > 400 and want[-1] == want[-2] == cap, (sizes, want)
    assert np.isfinite(loss.item())
    with torch.no_grad():
        assert bool(torch.isfinite(render(sc.cam, pc, pipe, sc.bg)["render"]).all())


def test_c_abi_refuses_bad_arguments():
    """The library's own checks, reached with a real context (the Python layer refuses most of these earlier)."""
    import ctypes as C
    from gaussian_gan_decoder_amd import _capi
    dev = torch.device(DEV)
    cx, stream = _capi.context_and_stream(dev)
    lib, h, st = cx.lib, cx.handle, C.c_void_p(stream)
    P, M, num = 100, 4, 5
    nbytes = lib.ggd_mcmc_tmp_bytes(P, P)
    tmp = torch.zeros((nbytes + 16,), dtype=torch.uint8, device=dev)
    buf = torch.zeros((4 * P * 16,), device=dev)            # stands for every array: nothing may be launched
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    table = lambda skip=(): (C.c_void_p * 18)(*[None if k in skip else buf.data_ptr() for k in range(18)])
    reloc = lambda p=P, m=M, io=None, draws=vp(buf), t=vp(tmp), n=nbytes: lib.ggd_mcmc_relocate(h, st, p, m, io or table(), None, draws, t, n)
    plan = lambda p=P, k=num, o=vp(buf), t=vp(tmp), n=nbytes: lib.ggd_mcmc_add_plan(h, st, p, k, o, vp(buf), vp(buf), t, n)
    emit = lambda p=P, k=num, m=M, tin=None, tout=None, t=vp(tmp), n=nbytes: lib.ggd_mcmc_add_emit(h, st, p, k, m, tin or table(), tout or table(), t, n)
    with torch.cuda.device(dev):
        bad = {"P < 0": reloc(p=-1), "P > 2^26": reloc(p=(1 << 26) + 1), "M 0": reloc(m=0), "M 17": reloc(m=17),
               "tmp small": reloc(n=nbytes - 1), "tmp NULL": reloc(t=None), "tmp misaligned": reloc(t=vp(tmp, 4)),
               "draws NULL": reloc(draws=None), "param NULL": reloc(io=table(skip=(9,))), "half moments": reloc(io=table(skip=(2,))),
               "plan num < 0": plan(k=-1), "plan opacity NULL": plan(o=None), "plan tmp small": plan(n=8), "plan no rows": plan(p=0),
               "emit num 0": emit(k=0), "emit M 17": emit(m=17), "emit out NULL": emit(tout=table(skip=(12,))),
               "emit moments out without in": emit(tin=table(skip=(4, 5))), "emit tmp misaligned": emit(t=vp(tmp, 8)),
               "noise NULL": lib.ggd_mcmc_noise(h, st, P, None, vp(buf), vp(buf), vp(buf), vp(buf), 1.0, 1.0),
               "noise rotation misaligned": lib.ggd_mcmc_noise(h, st, P, vp(buf), vp(buf), vp(buf, 4), vp(buf), vp(buf), 1.0, 1.0),
               "noise P < 0": lib.ggd_mcmc_noise(h, st, -1, vp(buf), vp(buf), vp(buf), vp(buf), vp(buf), 1.0, 1.0),
               "relocation NULL": lib.ggd_compute_relocation(h, st, P, vp(buf), vp(buf), None, vp(buf), vp(buf)),
               "relocation n < 0": lib.ggd_compute_relocation(h, st, -1, vp(buf), vp(buf), vp(buf), vp(buf), vp(buf))}
    torch.cuda.synchronize()
    assert {k: v for k, v in bad.items() if v != -1} == {}
    assert reloc(m=0) == -1 and b"M (SH" in lib.ggd_last_error(h)
    assert not buf.any() and not tmp.any()                # nothing was launched
    assert lib.ggd_mcmc_add_plan(h, st, P, 0, None, None, None, vp(tmp), nbytes) == 0        # nothing to add is legal
    assert lib.ggd_mcmc_noise(h, st, 0, None, None, None, None, None, 1.0, 1.0) == 0
