"""Density control under a fixed budget: "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al. 2024) on
csrc/ggd_mcmc.hip.  This module holds the two free functions; the model-side steps are GaussianModel.relocate_gs,
add_new_gs and inject_position_noise.  The rule is restated from the paper's published source (the compute_relocation op
of its rasterizer fork and of gsplat, relocate_gs, add_new_gs, the noise lines of its train.py); the reference tree this
package was modelled on does not contain it.  DESIGN.md section 6zg has the per-row rules.

A fitting loop uses them as upstream's does:

    loss = image_loss + mcmc_regularizers(pc)
    loss.backward()
    with torch.no_grad():
        grown = 0
        if it % 100 == 0:
            pc.relocate_gs()
            grown = pc.add_new_gs(cap_max)        # new parameters: this iteration's gradients belong to the old ones
        if not grown:
            pc.optimizer.step()
        pc.optimizer.zero_grad(set_to_none=True)
        pc.inject_position_noise(noise_lr=5e5)
"""
from __future__ import annotations

import ctypes as C

import torch

N_MAX = 51


def compute_relocation(opacities, scales, ratios, binoms=None, n_max=None):
    """Relocation values on ACTIVATED inputs: opacities float32 [n] or [n, 1], scales float32 [n, 3], ratios an integer
    tensor [n] or [n, 1] (clamped to 1..51).  Returns (new_opacities, new_scales) in the shapes given:
        o' = 1 - (1 - o)^(1/N)      s' = s o / sum_{i=1..N} sum_{k<i} C(i-1, k) (-1)^k / sqrt(k+1) o'^(k+1)
    One HIP launch, evaluated in fp64 and rounded once.  Upstream's trailing `binoms, n_max` are accepted and ignored: the
    table is built into the library, for n_max = 51.  Device tensors only: there is no CPU fallback."""
    who = "compute_relocation"
    for t, name in ((opacities, "opacities"), (scales, "scales"), (ratios, "ratios")):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who}: {name} must be a tensor")
    n = scales.shape[0] if scales.dim() == 2 else -1
    if scales.dtype != torch.float32 or scales.dim() != 2 or scales.shape[1] != 3:
        raise ValueError(f"{who}: scales must be float32 [n, 3]")
    if opacities.dtype != torch.float32 or tuple(opacities.shape) not in ((n,), (n, 1)):
        raise ValueError(f"{who}: opacities must be float32 [{n}] or [{n}, 1]")
    if ratios.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8) or tuple(ratios.shape) not in ((n,), (n, 1)):
        raise ValueError(f"{who}: ratios must be an integer tensor [{n}] or [{n}, 1]")
    for t, name in ((opacities, "opacities"), (scales, "scales"), (ratios, "ratios")):
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {name} must be a HIP device tensor (there is no CPU fallback)")
        if t.device != scales.device:
            raise ValueError(f"{who}: every tensor must be on {scales.device}")
    if n >= 1 << 31:
        raise ValueError(f"{who}: fewer than 2^31 rows")
    from . import _capi
    dev = scales.device
    o, s = opacities.detach().contiguous(), scales.detach().contiguous()
    r = ratios.clamp(1, N_MAX).to(torch.int32).contiguous()
    new_o, new_s = torch.empty_like(o), torch.empty_like(s)
    cx, stream = _capi.context_and_stream(dev)
    if cx.poison_outputs:                                 # tests: an element the launch does not write shows as NaN
        new_o.fill_(float("nan")), new_s.fill_(float("nan"))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        cx.check(cx.lib.ggd_compute_relocation(cx.handle, C.c_void_p(stream), n, ptr(o), ptr(s), ptr(r), ptr(new_o), ptr(new_s)))
    return new_o, new_s


def mcmc_regularizers(pc, opacity_reg=0.01, scale_reg=0.01):
    """opacity_reg * mean|opacity| + scale_reg * mean|scale| on the activated values: the two terms upstream adds to the image
    loss so that Gaussians which explain nothing fade out and are relocated.  Plain torch ops (differentiable; not hot)."""
    return opacity_reg * torch.abs(pc.get_opacity).mean() + scale_reg * torch.abs(pc.get_scaling).mean()
