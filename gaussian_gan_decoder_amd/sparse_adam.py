"""SparseGaussianAdam: the accelerated 3DGS rasterizer's optimizer (`optimizer_type="sparse_adam"`, its
`from diff_gaussian_rasterization import SparseGaussianAdam`) on csrc/ggd_adam.hip.

One `step(visibility, N)` is ONE launch over all groups (ggd_adam_sparse): rows the frame did not see keep their parameter
and both Adam moments, and are neither read nor written.  Per element of a visible row, in fp32,
    m' = b1 m + (1 - b1) g      v' = b2 v + ((1 - b2) g) g      p' = p - lr m' / (sqrt(v') + eps)
with betas 0.9 / 0.999, no bias correction and no step counter (the published adamUpdate rule).  Device
tensors only: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

BETAS = (0.9, 0.999)
MAX_GROUPS = 8
MAX_ROWS = 1 << 26


class SparseGaussianAdam(torch.optim.Adam):
    def __init__(self, params, lr, eps):
        super().__init__(params=params, lr=lr, eps=eps)

    @torch.no_grad()
    def step(self, visibility, N):
        """visibility: bool / uint8 [N] device tensor (row i is updated when set) or the rasterizer's int32 radii [N] (when
        radii[i] > 0).  Every group holds one [N, ...] float32 parameter; a group whose parameter has no gradient is skipped.
        Everything is checked before anything is launched."""
        N = int(N)
        if not 0 <= N <= MAX_ROWS:
            raise ValueError(f"SparseGaussianAdam.step: N must be in [0, 2^26] (got {N})")
        if not isinstance(visibility, torch.Tensor):
            raise ValueError("SparseGaussianAdam.step: visibility must be a tensor")
        if not visibility.is_cuda:
            raise RuntimeError("SparseGaussianAdam.step: visibility must be a HIP device tensor (there is no CPU fallback)")
        if visibility.dtype not in (torch.bool, torch.uint8, torch.int32) or tuple(visibility.shape) != (N,):
            raise ValueError(f"SparseGaussianAdam.step: visibility must be bool / uint8 [{N}] or the int32 radii [{N}]")
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"SparseGaussianAdam.step: at most {MAX_GROUPS} groups (have {len(self.param_groups)})")
        dev = visibility.device
        work = []
        for group in self.param_groups:
            if len(group["params"]) != 1:
                raise ValueError("SparseGaussianAdam: one tensor per group (the group "
                                 f"{group.get('name', '?')!r} has {len(group['params'])})")
            param = group["params"][0]
            if param.grad is None:
                continue
            grad = param.grad
            state = self.state[param]
            moments = [state[k] for k in ("exp_avg", "exp_avg_sq")] if len(state) else []
            for t, what in [(param, "parameter"), (grad, "gradient")] + [(t, "Adam moment") for t in moments]:
                if not t.is_cuda:
                    raise RuntimeError(f"SparseGaussianAdam.step: the {what} of group {group.get('name', '?')!r} must be a HIP "
                                       "device tensor (there is no CPU fallback)")
                if t.device != dev:
                    raise ValueError(f"SparseGaussianAdam.step: every tensor must be on {dev} (a {what} is on {t.device})")
                if t.dtype != torch.float32:
                    raise ValueError(f"SparseGaussianAdam.step: the {what} of group {group.get('name', '?')!r} must be float32")
                if t.numel() != param.numel():
                    raise ValueError(f"SparseGaussianAdam.step: the {what} of group {group.get('name', '?')!r} has "
                                     f"{t.numel()} elements, the parameter {param.numel()}")
                if what != "gradient" and not t.is_contiguous():
                    raise ValueError(f"SparseGaussianAdam.step: the {what} of group {group.get('name', '?')!r} must be contiguous")
            width = param.numel() // N if N else 0
            if param.numel() != N * width:
                raise ValueError(f"SparseGaussianAdam.step: group {group.get('name', '?')!r} has {param.numel()} elements, "
                                 f"not a multiple of N = {N}")
            if N * width >= 1 << 31:
                raise ValueError("SparseGaussianAdam.step: a group must hold fewer than 2^31 elements")
            work.append((group, param, grad.contiguous(), state))
        if N == 0 or not work:
            return
        for group, param, grad, state in work:           # lazily, as upstream does; the kernel does not advance `step`
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(param, memory_format=torch.contiguous_format)
                state["exp_avg_sq"] = torch.zeros_like(param, memory_format=torch.contiguous_format)
        from . import _capi
        cx, stream = _capi.context_and_stream(dev)
        table = (_capi.AdamGroup * len(work))()
        for slot, (group, param, grad, state) in zip(table, work):
            slot.param, slot.grad = param.data_ptr(), grad.data_ptr()
            slot.exp_avg, slot.exp_avg_sq = state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr()
            slot.width, slot.lr, slot.eps = param.numel() // N, float(group["lr"]), float(group["eps"])
        vis = visibility.contiguous()
        radii = vis.dtype == torch.int32
        ptr = C.c_void_p(vis.data_ptr())
        with torch.cuda.device(dev):
            cx.check(cx.lib.ggd_adam_sparse(cx.handle, C.c_void_p(stream), N, len(work), table, None if radii else ptr,
                                            ptr if radii else None, BETAS[0], BETAS[1]))
