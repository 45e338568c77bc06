"""Device time of the MCMC density control (csrc/ggd_mcmc.hip) against the same steps composed from torch ops, as upstream's
fitting loop composes them.  python scripts/mcmc_timing.py [--rounds R] [--points N]

N rows (default 1 M), 16 SH coefficients per channel, torch.optim.Adam state present.  Variants, alternated inside ONE process
(every round times each variant once, the order rotating), hipEvent pairs (around 10 back-to-back calls for the two noise
forms, around one relocation), R rounds (default 20) after 3 warm-up rounds:
  noise_hip       GaussianModel.inject_position_noise with given noise: one launch
  noise_torch     L = R S, covariance = L L^T, noise * op_sigmoid(1 - opacity) * noise_lr * xyz_lr, bmm, add_ -- upstream's lines
  relocate_hip    GaussianModel.relocate_gs with given draws on a model with 5 % dead rows: five launches, no host wait
  relocate_torch  upstream's relocate_gs: nonzero of the dead and alive masks, multinomial over the alive opacities, bincount,
                  the relocation values (mcmc.compute_relocation, the same HIP op in both: upstream calls its CUDA op here),
                  index assignments into the six tensors, zeroed moments of the sampled rows
Both relocations start every sample from the same state (restored outside the timed window).  Before the timing both noise
forms are compared with the same rule in float64 on the device (per row, largest error over the row's largest component).
Per variant: median, min, 10th and 90th percentile in ms.  Bytes of the noise launch: 17 floats read and 3 written per row, set against 6.3 TB/s.  One JSON line."""
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from gaussian_gan_decoder_amd.gaussian_model import PARAM_GROUPS, GaussianModel, build_rotation  # noqa: E402
from gaussian_gan_decoder_amd.mcmc import compute_relocation  # noqa: E402

HBM_TBS = 6.3
M = 16
NOISE_REPS = 10
SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (M - 1, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}


def option(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def percentile(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def noise_torch(pc, xi, noise_lr, xyz_lr):
    L = build_rotation(pc._rotation) @ torch.diag_embed(pc.get_scaling)
    cov = L @ L.transpose(1, 2)
    gate = 1 / (1 + torch.exp(-100 * ((1 - pc.get_opacity) - 0.995)))
    noise = xi * gate * noise_lr * xyz_lr
    pc._xyz.add_(torch.bmm(cov, noise.unsqueeze(-1)).squeeze(-1))


def relocate_torch(pc):
    """upstream's relocate_gs / _update_params / replace_tensors_to_optimizer on this model's tensors"""
    opacity = pc.get_opacity
    dead_mask = (opacity <= 0.005).squeeze(-1)
    dead_idx = dead_mask.nonzero(as_tuple=True)[0]
    alive_idx = (~dead_mask).nonzero(as_tuple=True)[0]
    if dead_idx.shape[0] == 0:
        return
    probs = opacity[alive_idx, 0]
    sampled = alive_idx[torch.multinomial(probs / probs.sum(), dead_idx.shape[0], replacement=True)]
    ratio = torch.bincount(sampled, minlength=opacity.shape[0])[sampled] + 1
    new_opacity, new_scaling = compute_relocation(opacity[sampled], pc.get_scaling[sampled], ratio.clamp(1, 51).int())
    new_opacity = torch.clamp(new_opacity, max=1.0 - torch.finfo(torch.float32).eps, min=0.005)
    new = {"_xyz": pc._xyz[sampled], "_features_dc": pc._features_dc[sampled], "_features_rest": pc._features_rest[sampled],
           "_opacity": torch.log(new_opacity / (1 - new_opacity)), "_scaling": torch.log(new_scaling), "_rotation": pc._rotation[sampled]}
    for attr, value in new.items():
        p = getattr(pc, attr)
        p[dead_idx] = value
        if attr in ("_opacity", "_scaling"):
            p[sampled] = value
        st = pc.optimizer.state[p]
        st["exp_avg"][sampled] = 0
        st["exp_avg_sq"][sampled] = 0


def main():
    rounds, N = max(5, option("--rounds", 20)), option("--points", 1_000_000)
    if not torch.cuda.is_available():
        raise RuntimeError("mcmc_timing.py needs an MI355X: no HIP device visible")
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    values = {n: torch.randn((N,) + s, generator=gen) for n, s in SHAPES.items()}
    values["scaling"] = -7.0 + 4.0 * torch.rand((N, 3), generator=gen)
    dead = torch.rand(N, generator=gen) < 0.05
    u = torch.rand((N, 1), generator=gen)
    values["opacity"] = torch.where(dead[:, None], -9.0 + 3.0 * u, -4.0 + 8.0 * u)
    pc = GaussianModel(3)
    for name, attr in PARAM_GROUPS:
        setattr(pc, attr, torch.nn.Parameter(values[name].to(dev)))
    pc.spatial_lr_scale = 1.0
    pc.training_setup(SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016,
                                      position_lr_delay_mult=0.01, position_lr_max_steps=30_000, feature_lr=0.0025,
                                      opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001))
    for _, attr in PARAM_GROUPS:
        getattr(pc, attr).grad = torch.zeros_like(getattr(pc, attr))
    pc.optimizer.step()
    pc.optimizer.zero_grad(set_to_none=True)
    saved = {attr: getattr(pc, attr).detach().clone() for _, attr in PARAM_GROUPS}
    xi = torch.randn((N, 3), generator=gen).to(dev)
    draws = torch.randint(0, 1 << 32, (N,), generator=gen, dtype=torch.int64).to(dev)
    noise_lr, xyz_lr = 5e5, 1.6e-4

    def restore():
        with torch.no_grad():
            for _, attr in PARAM_GROUPS:
                getattr(pc, attr).copy_(saved[attr])

    def noise64():                                         # the same rule in float64 on the device: the yardstick of both forms
        s, q, x = pc._scaling.double(), pc._rotation.double(), pc._opacity.double()
        L = build_rotation(q) * torch.exp(s)[:, None, :]
        gate = torch.sigmoid(100.0 * (torch.sigmoid(-x) - 0.995))
        return torch.bmm(L @ L.transpose(1, 2), (xi.double() * gate * noise_lr * xyz_lr).unsqueeze(-1)).squeeze(-1)

    errors = {}
    with torch.no_grad():                                  # same result first: both forms against float64, per row, relative
        ref = noise64()                                    # to the row's largest component
        scale = ref.abs().amax(dim=1)
        for name, run in (("noise_hip", lambda: pc.inject_position_noise(noise_lr, xyz_lr, noise=xi)),
                          ("noise_torch", lambda: noise_torch(pc, xi, noise_lr, xyz_lr))):
            run()
            moved = pc._xyz.double() - saved["_xyz"].double()
            ulp = (saved["_xyz"].abs().amax(dim=1).double() + scale) * 2.0 ** -23   # the in-place fp32 add
            errors[name] = (((moved - ref).abs().amax(dim=1) - ulp).clamp_min(0) / scale.clamp_min(1e-300))[scale > 1e-12].max().item()
            restore()
    variants = {"noise_hip": lambda: pc.inject_position_noise(noise_lr, xyz_lr, noise=xi),
                "noise_torch": lambda: noise_torch(pc, xi, noise_lr, xyz_lr),
                "relocate_hip": lambda: pc.relocate_gs(draws=draws),
                "relocate_torch": lambda: relocate_torch(pc)}
    names = list(variants)
    ms = {n: [] for n in names}
    with torch.no_grad():
        for rnd in range(3 + rounds):
            for k in range(len(names)):
                name = names[(k + rnd) % len(names)]
                restore()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                reps = NOISE_REPS if name.startswith("noise") else 1   # (a relocation needs its dead rows back every time)
                a.record()
                for _ in range(reps):
                    variants[name]()
                b.record()
                b.synchronize()
                if rnd >= 3:
                    ms[name].append(a.elapsed_time(b) / reps)
    out = dict(N=N, sh_coefficients=M, dead_rows=int(dead.sum()), rounds=rounds, noise_reps=NOISE_REPS,
               noise_max_row_error_vs_float64=errors)
    for name in names:
        med, lo, hi = statistics.median(ms[name]), percentile(ms[name], 0.1), percentile(ms[name], 0.9)
        out[name] = dict(median_ms=round(med, 4), min_ms=round(min(ms[name]), 4), p10_ms=round(lo, 4), p90_ms=round(hi, 4))
    moved_bytes = N * 20 * 4
    out["noise_hip"].update(mb=round(moved_bytes / 1e6, 1), tb_s=round(moved_bytes / out["noise_hip"]["median_ms"] / 1e9, 2),
                            fraction_of_hbm=round(moved_bytes / out["noise_hip"]["median_ms"] / 1e9 / HBM_TBS, 2))
    out["noise_torch_over_hip"] = round(out["noise_torch"]["median_ms"] / out["noise_hip"]["median_ms"], 2)
    out["relocate_torch_over_hip"] = round(out["relocate_torch"]["median_ms"] / out["relocate_hip"]["median_ms"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
