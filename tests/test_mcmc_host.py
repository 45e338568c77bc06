"""MCMC density control without a GPU: the float64 / integer restatement of tests/_mcmc_ref.py against closed forms, the bars'
constants against their own yardsticks, the scratch layout the Python layer reads against the library's, and the argument checks
of the public surface (which raise before anything is launched)."""
import inspect
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _mcmc_ref as R


def test_relocation_at_n1_is_the_identity():
    o = np.array([0.005, 0.01, 0.1, 0.5, 0.9, 0.999, 1 - 1e-6])
    op, coeff, cond = R.relocation64(o, np.ones(o.size, np.int64))
    assert np.abs(op - o).max() <= 1e-15 and np.abs(coeff - 1).max() <= 1e-14 and np.abs(cond - 1).max() <= 1e-14
    x = np.log(o / (1 - o)).astype(np.float32)
    s = np.linspace(-6, 1, 3 * o.size).reshape(-1, 3).astype(np.float32)
    raw, new_s, _ = R.raw_values64(x, s, np.ones(o.size, np.int64))
    o32 = 1 / (1 + np.exp(-x.astype(np.float64)))
    keep = (o32 >= R.O_MIN) & (o32 <= R.O_MAX)
    assert keep.sum() >= 5 and np.abs(raw - x)[keep].max() <= 1e-12 and np.abs(new_s - s).max() <= 1e-12


def test_relocation_at_n2_matches_the_hand_expansion():
    """N = 2: o' = 1 - sqrt(1 - o); D = o' + (o' - o'^2 / sqrt 2) = 2 o' - o'^2 / sqrt 2."""
    o = np.array([0.005, 0.02, 0.3, 0.5, 0.8, 0.99, 1 - 1e-6])
    op, coeff, _ = R.relocation64(o, np.full(o.size, 2))
    hand_op = 1 - np.sqrt(1 - o)
    assert np.abs(op - hand_op).max() <= 1e-13
    assert np.abs(coeff - o / (2 * hand_op - hand_op ** 2 / math.sqrt(2))).max() <= 1e-12 * coeff.max()


def test_the_ratio_is_what_conserves_the_total_opacity():
    """N copies of opacity o' stacked at one place let through (1 - o')^N = 1 - o: the defining property of o'."""
    o = np.array([0.01, 0.4, 0.95])
    for N in (3, 17, 51):
        op, _, _ = R.relocation64(o, np.full(o.size, N))
        assert np.abs((1 - op) ** N - (1 - o)).max() <= 1e-14


def test_sampling_restatement_on_hand_made_weights():
    w = [0, 5, 0, 0, 3, 1, 0]
    top = (1 << 32) - 1
    assert R.sample_sources(w, [0])[0] == [1]                       # the first alive row
    assert R.sample_sources(w, [top])[0] == [5]                     # the last alive row
    W = sum(w)
    seen = set()
    for tau, want in ((0, 1), (4, 1), (5, 4), (7, 4), (8, 5)):      # every interval's two ends
        d = -(-(tau << 32) // W)                                    # the smallest draw with floor(d W / 2^32) = tau
        assert (d * W) >> 32 == tau
        assert R.sample_sources(w, [d])[0] == [want]
        seen.add(want)
    sources, counts = R.sample_sources(w, list(range(0, 1 << 32, (1 << 32) // 997)))
    assert set(sources) == seen == {1, 4, 5} and all(counts[i] == 0 for i in (0, 2, 3, 6)) and sum(counts) == len(sources)
    assert R.sample_sources(w, {6: top, 0: 0, 2: 0})[0] == [1, 1, 5]            # dict form: in the order of the destinations
    assert R.sample_sources([0, 0], [5]) == ([-1], [0, 0])          # nothing alive
    assert R.weights_ref([0.5, 1e-9, 1.0, 0.3], [False, False, False, True]) == [1 << 19, 1, 1 << 20, 0]


def test_the_bars_contain_their_own_yardsticks():
    """C_REL and NOISE_RTOL are twice what the fp32 restatements measure against float64 (the figures are in _mcmc_ref's
    docstring and DESIGN.md); here: the measurement itself lies inside the bar it defines."""
    c = R.measure_c()
    rtol = R.measure_noise_rtol()
    print(f"value bar: measured c = {c}, C_REL = {R.C_REL}; noise: measured rtol = {rtol:.3e}, NOISE_RTOL = {R.NOISE_RTOL}")
    assert max(c) <= R.C_REL and rtol <= R.NOISE_RTOL
    x, s, N = R.value_inputs()
    o = 1 / (1 + np.exp(-x.astype(np.float64)))
    assert o.min() <= 0.00501 and o.max() >= 1 - 1.1e-6 and set(N) == set(range(1, 52))
    raw, _, cond = R.raw_values64(x, s, N)
    sig = 1 / (1 + np.exp(-raw))
    assert sig.min() >= R.O_MIN * (1 - 1e-12) and sig.max() <= R.O_MAX and cond.max() > 1000


def test_scratch_layout_matches_the_library(native_lib):
    from gaussian_gan_decoder_amd.gaussian_model import mcmc_tmp_layout
    for P, n in ((0, 0), (1, 1), (2047, 5), (2048, 2048), (2049, 102), (20_011, 20_011), (1 << 20, 52_428), (1 << 26, 1 << 26)):
        assert native_lib.ggd_mcmc_tmp_bytes(P, n) == mcmc_tmp_layout(P, n)["total"], (P, n)
    assert native_lib.ggd_mcmc_tmp_bytes((1 << 26) + 1, 0) == 0 and native_lib.ggd_mcmc_tmp_bytes(5, -1) == 0


def cpu_model(P=10, M=4, setup=True):
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel
    pc = GaussianModel(1)
    gen = torch.Generator().manual_seed(0)
    for attr, shape in (("_xyz", (P, 3)), ("_features_dc", (P, 1, 3)), ("_features_rest", (P, M - 1, 3)), ("_opacity", (P, 1)),
                        ("_scaling", (P, 3)), ("_rotation", (P, 4))):
        setattr(pc, attr, torch.nn.Parameter(torch.randn(shape, generator=gen)))
    pc.spatial_lr_scale = 1.0
    if setup:
        pc.training_setup(SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016,
                                          position_lr_delay_mult=0.01, position_lr_max_steps=30_000, feature_lr=0.0025,
                                          opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001))
    return pc


def test_model_methods_refuse_cpu_tensors_and_wrong_shapes():
    pc = cpu_model()
    before = {a: getattr(pc, a).detach().clone() for a in ("_xyz", "_opacity", "_scaling")}
    P = 10
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.relocate_gs()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.relocate_gs(draws=torch.zeros(P, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.add_new_gs(100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.inject_position_noise(5e5)
    with pytest.raises(ValueError, match="draws"):
        pc.relocate_gs(draws=torch.zeros(P + 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="draws"):
        pc.relocate_gs(draws=torch.zeros(P, dtype=torch.int32))
    with pytest.raises(ValueError, match="dead_mask"):
        pc.relocate_gs(dead_mask=torch.zeros(P - 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="dead_mask"):
        pc.relocate_gs(dead_mask=torch.zeros(P))
    with pytest.raises(ValueError, match="draws"):
        pc.add_new_gs(100, draws=torch.zeros(3, dtype=torch.int64))          # int(1.05 * 10) - 10 = 0 rows to add
    with pytest.raises(ValueError, match="noise"):
        pc.inject_position_noise(5e5, noise=torch.zeros(P, 2))
    with pytest.raises(ValueError, match="noise"):
        pc.inject_position_noise(5e5, noise=torch.zeros(P, 3, dtype=torch.float64))
    for a, t in before.items():
        assert torch.equal(getattr(pc, a).detach(), t)


def test_compute_relocation_refuses_cpu_tensors_and_wrong_shapes():
    from gaussian_gan_decoder_amd.mcmc import compute_relocation
    o, s, r = torch.full((4,), 0.5), torch.ones(4, 3), torch.ones(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_relocation(o, s, r)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_relocation(o[:, None], s, r[:, None].long(), None, 51)
    for bad in ((o[:3], s, r), (o, s[:, :2], r), (o, s, r[:3]), (o.double(), s, r), (o, s, r.float()), (o, s.double(), r),
                (o, [1.0], r)):
        with pytest.raises(ValueError):
            compute_relocation(*bad)


def test_shim_exports_compute_relocation_with_upstreams_signature():
    import diff_gaussian_rasterization as shim
    from gaussian_gan_decoder_amd import mcmc
    assert shim.compute_relocation is mcmc.compute_relocation
    assert list(inspect.signature(shim.compute_relocation).parameters) == ["opacities", "scales", "ratios", "binoms", "n_max"]


def test_regularizers_are_the_two_means_and_differentiable():
    from gaussian_gan_decoder_amd.mcmc import mcmc_regularizers
    pc = cpu_model(setup=False)
    loss = mcmc_regularizers(pc, opacity_reg=0.02, scale_reg=0.03)
    want = 0.02 * torch.sigmoid(pc._opacity).mean() + 0.03 * torch.exp(pc._scaling).mean()
    assert torch.allclose(loss, want, rtol=1e-6, atol=0)
    loss.backward()
    assert pc._opacity.grad.abs().min() > 0 and pc._scaling.grad.abs().min() > 0 and pc._xyz.grad is None
    assert torch.allclose(mcmc_regularizers(pc), 0.01 * torch.sigmoid(pc._opacity).mean() + 0.01 * torch.exp(pc._scaling).mean())
