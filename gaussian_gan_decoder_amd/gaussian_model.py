"""Gaussian attribute container: the decoder path's getters and the per-scene fitting loop's optimizer and density control.

Mirrors gaussian_splatting/scene/gaussian_model.py: the constructor (:47-63), the activation getters that form the
rasterizer's input prologue (:100-124: exp / normalize / sigmoid / pass-through), get_covariance (:29-33,123-124),
create_from_pcd / create_from_pos_col (:126-185; their `distCUDA2` is knn.dist_cuda2), and what the reference's fitting
loop (gaussian_splatting/train.py:31-132) calls: training_setup / update_learning_rate (:217-246), capture / restore
(:65-97), reset_opacity (:305-308), add_densification_stats (:544-546), densify_and_prune (:453-542) and prune_points
(:390-404).  The reference builds the last three from boolean-mask indexing (a `nonzero` and a host wait per mask, four
copies of every parameter and Adam moment per densification); here they are csrc/ggd_densify.hip: one launch without a
host wait per iteration (update_densification_stats also keeps max_radii2D), and per densification three small launches,
one read-back of the new row count and one gather launch that writes every parameter and moment once (DESIGN.md section
6k).  Those methods need device tensors: there is no CPU fallback.  Absent on purpose: the fork's GUI-only
manual_densification masks (off by default in the reference), the kill_*_learning_rate helpers, the plyfile import.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
from torch import nn

from .sh import RGB2SH

# optimizer group name -> attribute, in the order training_setup registers them (and csrc/ggd_densify.hip gathers them)
PARAM_GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
                ("scaling", "_scaling"), ("rotation", "_rotation"))


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """step -> learning rate: lr_init at step 0, lr_final from max_steps on, log-linear in between; while step <
    lr_delay_steps the rate is scaled by a factor that rises from lr_delay_mult to 1 along a quarter sine.  0 for a negative
    step or when both rates are 0 (reference: utils/general_utils.py:29-62)."""
    def rate(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        delay = 1.0
        if lr_delay_steps > 0:
            delay = lr_delay_mult + (1.0 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
        t = min(max(step / max_steps, 0.0), 1.0)
        return delay * math.exp(math.log(lr_init) * (1.0 - t) + math.log(lr_final) * t)
    return rate


def build_rotation(q: torch.Tensor) -> torch.Tensor:
    """[N,4] (w,x,y,z), normalised here -> [N,3,3] (reference: utils/general_utils.py:78-99)."""
    q = q / torch.sqrt((q * q).sum(dim=1, keepdim=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
            2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
            2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).view(-1, 3, 3)


def build_covariance_from_scaling_rotation(scaling, scaling_modifier, rotation):
    """Sigma = L L^T with L = R diag(mod*s); returns the 6 upper-triangular entries [N,6]
    (reference: gaussian_model.py:29-33, general_utils.py:64-73,101-110)."""
    L = build_rotation(rotation) * (scaling_modifier * scaling)[:, None, :]
    cov = L @ L.transpose(1, 2)
    return torch.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], dim=1)


def inverse_sigmoid(x):
    """logit (reference: utils/general_utils.py:18-19)."""
    return torch.log(x / (1 - x))


def _device_float(a, device=None) -> torch.Tensor:
    """numpy array / sequence / tensor -> float32 tensor on the HIP device (a device tensor stays where it is)."""
    if isinstance(a, torch.Tensor):
        t = a.detach()
        return t.float() if t.is_cuda and device is None else t.float().to(device or "cuda")
    return torch.as_tensor(np.asarray(a)).float().to(device or "cuda")


_ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # a tensor's device address for the C ABI (None: NULL)


def _group_table(groups):
    """The C ABI's 18-pointer table of a [[parameter, exp_avg, exp_avg_sq] x 6] list (None: NULL, a group without moments)."""
    return (C.c_void_p * 18)(*[t.data_ptr() if t is not None else None for row in groups for t in row])


def mcmc_tmp_layout(P, n_dest):
    """Byte offsets of the arrays in the scratch of ggd_mcmc_relocate / ggd_mcmc_add_plan (include/ggd_raster.h), each
    aligned to 256 bytes, and the total (= ggd_mcmc_tmp_bytes)."""
    align = lambda n: (n + 255) // 256 * 256
    T = (P + 2047) // 2048 * 2048
    lay, off = {}, 0
    for name, nbytes in (("weights", 4 * T), ("prefix", 4 * T), ("tiles", 8 * (T // 2048 + 1)), ("counts", 4 * P),
                         ("sources", 4 * n_dest), ("values", 16 * P)):
        lay[name], off = off, off + align(nbytes)
    lay["total"] = off
    return lay


class GaussianModel:
    def __init__(self, sh_degree: int):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        self._xyz = torch.empty(0)
        self._features_dc = torch.empty(0)
        self._features_rest = torch.empty(0)
        self._scaling = torch.empty(0)
        self._rotation = torch.empty(0)
        self._opacity = torch.empty(0)
        self.max_radii2D = torch.empty(0)
        self.xyz_gradient_accum = torch.empty(0)
        self.denom = torch.empty(0)
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0
        self.scaling_activation = torch.exp
        self.scaling_inverse_activation = torch.log
        self.opacity_activation = torch.sigmoid
        self.inverse_opacity_activation = inverse_sigmoid
        self.rotation_activation = torch.nn.functional.normalize
        self.covariance_activation = build_covariance_from_scaling_rotation

    @property
    def get_scaling(self):
        return self.scaling_activation(self._scaling)

    @property
    def get_rotation(self):
        return self.rotation_activation(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        if self.active_sh_degree == 0:
            return self._features_dc
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return self.opacity_activation(self._opacity)

    def get_covariance(self, scaling_modifier=1):
        return self.covariance_activation(self.get_scaling, scaling_modifier, self._rotation)

    def save_ply(self, path):
        """Binary PLY in the reference's field order (gaussian_model.py:281-302), raw pre-activation values."""
        from .ply_io import save_ply
        save_ply(path, self)

    def load_ply(self, path, device="cpu"):
        from .ply_io import load_ply
        return load_ply(path, self, device)

    def _seed(self, xyz, colors):
        """Shared part of the two constructors below: SH features (DC = RGB2SH(colour), the rest zero), isotropic scales
        log(sqrt(mean squared distance to the three nearest points)) floored at 1e-7, identity quaternions."""
        from .knn import dist_cuda2
        P = xyz.shape[0]
        features = torch.zeros((P, 3, (self.max_sh_degree + 1) ** 2), dtype=torch.float32, device=xyz.device)
        features[:, :, 0] = RGB2SH(colors)
        dist2 = torch.clamp_min(dist_cuda2(xyz), 0.0000001)
        scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
        rots = torch.zeros((P, 4), dtype=torch.float32, device=xyz.device)
        rots[:, 0] = 1
        return features, scales, rots

    def _adopt(self, xyz, features, scales, rots, opacities):
        self._xyz = nn.Parameter(xyz.requires_grad_(True))
        self._features_dc = nn.Parameter(features[:, :, 0:1].transpose(1, 2).contiguous().requires_grad_(True))
        self._features_rest = nn.Parameter(features[:, :, 1:].transpose(1, 2).contiguous().requires_grad_(True))
        self._scaling = nn.Parameter(scales.requires_grad_(True))
        self._rotation = nn.Parameter(rots.requires_grad_(True))
        self._opacity = nn.Parameter(opacities.requires_grad_(True))
        self.max_radii2D = torch.zeros((xyz.shape[0],), device=xyz.device)

    def create_from_pcd(self, pcd, spatial_lr_scale: float):
        """Initial model from a point cloud: any object with `.points` and `.colors` ([P, 3], colours in 0..1), P >= 4
        (reference: gaussian_model.py:126-150).  Opacity inverse_sigmoid(0.1)."""
        self.spatial_lr_scale = spatial_lr_scale
        xyz = _device_float(pcd.points).clone()
        features, scales, rots = self._seed(xyz, _device_float(pcd.colors, xyz.device))
        opacities = inverse_sigmoid(0.1 * torch.ones((xyz.shape[0], 1), dtype=torch.float32, device=xyz.device))
        self._adopt(xyz, features, scales, rots, opacities)

    def create_from_pos_col(self, positions, colors=None, opacity=None, rotation=None, scaling=None):
        """Initial model from positions and optional colours (clipped to 0..1; grey when absent), per-point opacities
        (floored at 0.1 before the logit) and `rotation` / `scaling` rows that overwrite the LEADING rows of the defaults
        (reference: gaussian_model.py:152-185).  The seeded scales / rotations stay reachable as target_scales / target_rots."""
        self.spatial_lr_scale = 1
        xyz = _device_float(positions).clone()
        colors = torch.full_like(xyz, 0.5) if colors is None else _device_float(colors, xyz.device)
        features, scales, rots = self._seed(xyz, torch.clamp(colors, 0, 1))
        if scaling is not None:
            given = _device_float(scaling, xyz.device)
            scales[:given.shape[0]] = given
        if rotation is not None:
            given = _device_float(rotation, xyz.device)
            rots[:given.shape[0]] = given
        self.target_scales = scales
        self.target_rots = rots
        if opacity is not None:
            opacities = inverse_sigmoid(torch.clamp(_device_float(opacity, xyz.device), min=0.1))
        else:
            opacities = inverse_sigmoid(0.1 * torch.ones((xyz.shape[0], 1), dtype=torch.float32, device=xyz.device))
        self._adopt(xyz, features, scales, rots, opacities)

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ---- optimizer (reference: gaussian_model.py:65-97, 217-246) ------------------------------------------------------
    def training_setup(self, training_args, decoder_params=None):
        """Adam over the six named groups (lr 0.0 / eps 1e-15 defaults, per-group rates from `training_args`), the position
        schedule, and zeroed densification statistics on the parameters' device.  training_args.optimizer_type (absent:
        "default") chooses torch.optim.Adam ("default") or sparse_adam.SparseGaussianAdam ("sparse_adam": one launch per
        step, over the rows the frame saw; `optimizer.step(radii, P)`; the six [P, ...] groups only, no decoder_params)."""
        optimizer_type = getattr(training_args, "optimizer_type", "default")
        if optimizer_type not in ("default", "sparse_adam"):
            raise ValueError(f"training_setup: optimizer_type must be 'default' or 'sparse_adam' (got {optimizer_type!r})")
        if optimizer_type == "sparse_adam" and decoder_params is not None:
            raise ValueError("training_setup: optimizer_type='sparse_adam' takes no decoder_params (one [P, ...] tensor per group)")
        self.percent_dense = training_args.percent_dense
        P, dev = self._xyz.shape[0], self._xyz.device
        self.xyz_gradient_accum = torch.zeros((P, 1), device=dev)
        self.denom = torch.zeros((P, 1), device=dev)
        rates = {"xyz": training_args.position_lr_init * self.spatial_lr_scale, "f_dc": training_args.feature_lr,
                 "f_rest": training_args.feature_lr / 20.0, "opacity": training_args.opacity_lr,
                 "scaling": training_args.scaling_lr, "rotation": training_args.rotation_lr}
        groups = [{"params": [getattr(self, attr)], "lr": rates[name], "name": name} for name, attr in PARAM_GROUPS]
        if decoder_params is not None:
            groups += decoder_params
        if optimizer_type == "sparse_adam":
            from .sparse_adam import SparseGaussianAdam
            self.optimizer = SparseGaussianAdam(groups, lr=0.0, eps=1e-15)
        else:
            self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        self.xyz_scheduler_args = get_expon_lr_func(lr_init=training_args.position_lr_init * self.spatial_lr_scale,
                                                    lr_final=training_args.position_lr_final * self.spatial_lr_scale,
                                                    lr_delay_mult=training_args.position_lr_delay_mult,
                                                    max_steps=training_args.position_lr_max_steps)

    def update_learning_rate(self, iteration):
        """Sets and returns the position group's rate for this iteration."""
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                group["lr"] = self.xyz_scheduler_args(iteration)
                return group["lr"]

    def capture(self):
        return (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
                self._opacity, self.max_radii2D, self.xyz_gradient_accum, self.denom, self.optimizer.state_dict(),
                self.spatial_lr_scale)

    def restore(self, model_args, training_args):
        (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
         self._opacity, self.max_radii2D, accum, denom, opt_dict, self.spatial_lr_scale) = model_args
        self.training_setup(training_args)
        self.xyz_gradient_accum = accum
        self.denom = denom
        self.optimizer.load_state_dict(opt_dict)

    def _own_groups(self):
        """The optimizer's groups of this model's six tensors (decoder groups ride along untouched), or None."""
        if self.optimizer is None:
            return None
        names = {name for name, _ in PARAM_GROUPS}
        return {g["name"]: g for g in self.optimizer.param_groups if g.get("name") in names}

    def _swap(self, name, attr, tensor, exp_avg=None, exp_avg_sq=None):
        """`tensor` becomes the group's nn.Parameter; its optimizer state (if any) is re-keyed to it with the given moments,
        `step` kept (the reference's _prune_optimizer / cat_tensors_to_optimizer / replace_tensor_to_optimizer)."""
        new = nn.Parameter(tensor.requires_grad_(True))
        groups = self._own_groups()
        if groups is not None and name in groups:
            old = groups[name]["params"][0]
            state = self.optimizer.state.pop(old, None)
            groups[name]["params"][0] = new
            if state is not None:
                if exp_avg is not None:
                    state["exp_avg"], state["exp_avg_sq"] = exp_avg, exp_avg_sq
                self.optimizer.state[new] = state
        setattr(self, attr, new)
        return new

    def _adopt_groups(self, groups):
        """_swap of all six groups: a [[parameter, exp_avg, exp_avg_sq] x 6] list in the order of PARAM_GROUPS."""
        for (name, attr), (p, m1, m2) in zip(PARAM_GROUPS, groups):
            self._swap(name, attr, p, m1, m2)

    @staticmethod
    def _fresh_groups(src, rows, cx):
        """Uninitialised arrays of `rows` rows for every tensor of src (a list of _checked_groups)."""
        out = [[torch.empty((rows,) + tuple(t.shape[1:]), device=t.device) if t is not None else None for t in ins] for ins in src]
        if cx.poison_outputs:                             # tests: an element the launch does not write shows as NaN
            for t in (t for row in out for t in row if t is not None):
                t.fill_(float("nan"))
        return out

    def replace_tensor_to_optimizer(self, tensor, name):
        """Replaces group `name`'s parameter by `tensor` and zeroes its Adam moments; returns {name: new parameter}."""
        attr = dict(PARAM_GROUPS)[name]
        state = self.optimizer.state.get(self._own_groups()[name]["params"][0])
        zeros = (torch.zeros_like(tensor), torch.zeros_like(tensor)) if state is not None else (None, None)
        return {name: self._swap(name, attr, tensor, *zeros)}

    def reset_opacity(self):
        """Opacities above 0.01 drop to 0.01; the group's moments restart at zero."""
        opacity = self.get_opacity.detach()
        self.replace_tensor_to_optimizer(inverse_sigmoid(torch.min(opacity, torch.ones_like(opacity) * 0.01)), "opacity")

    # ---- density control (csrc/ggd_densify.hip) -------------------------------------------------------------------------
    def _device_rows(self, who):
        if not (isinstance(self._xyz, torch.Tensor) and self._xyz.is_cuda):
            raise RuntimeError(f"GaussianModel.{who} needs HIP device tensors (there is no CPU fallback)")
        return int(self._xyz.shape[0])

    def _stats(self, who, viewspace_point_tensor, radii, update_filter, use_absgrad=False):
        from . import _capi
        if use_absgrad:   # the same [P, 3] layout, handed to the same launch
            grad = getattr(viewspace_point_tensor, "absgrad", None)
            if grad is None:
                raise ValueError(f"{who}: use_absgrad=True, but viewspace_point_tensor has no .absgrad (render with "
                                 "absgrad=True and call backward first)")
        P = self._device_rows(who)
        if not use_absgrad:
            grad = viewspace_point_tensor.grad
        if grad is None:
            raise ValueError(f"{who}: viewspace_point_tensor has no .grad (call backward first)")
        for t in (self.xyz_gradient_accum, self.denom):   # updated in place
            if tuple(t.shape) != (P, 1) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{who}: call training_setup first (contiguous float32 device statistics [{P}, 1] expected)")
        for t, name, dtypes, shape in ((grad, "viewspace_point_tensor." + ("absgrad" if use_absgrad else "grad"), (torch.float32,), (P, 3)),
                                       (radii, "radii", (torch.int32,), (P,)),
                                       (update_filter, "update_filter", (torch.bool, torch.uint8), (P,))):
            if t is None:
                continue
            if not t.is_cuda:
                raise RuntimeError(f"{who}: {name} must be a HIP device tensor (there is no CPU fallback)")
            if t.dtype not in dtypes or tuple(t.shape) != shape:
                raise ValueError(f"{who}: {name} must be {' / '.join(str(d) for d in dtypes)} {list(shape)}")
        grad = grad.contiguous()
        radii = radii.contiguous() if radii is not None else None
        filt = update_filter.contiguous().view(torch.uint8) if update_filter is not None else None
        max_radii = None
        if radii is not None:
            t = self.max_radii2D
            if tuple(t.shape) != (P,) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{who}: max_radii2D must be a contiguous float32 device tensor [{P}]")
            max_radii = self.max_radii2D
        cx, stream = _capi.context_and_stream(grad.device)
        with torch.cuda.device(grad.device):
            cx.check(cx.lib.ggd_densify_stats(cx.handle, C.c_void_p(stream), P, _ptr(grad), _ptr(radii), _ptr(filt),
                                              _ptr(self.xyz_gradient_accum), _ptr(self.denom), _ptr(max_radii)))

    def add_densification_stats(self, viewspace_point_tensor, update_filter, use_absgrad=False):
        """On the rows of the bool filter: xyz_gradient_accum += |grad[:, :2]|, denom += 1.  One launch, no host wait.
        use_absgrad=True: the statistic is taken from `viewspace_point_tensor.absgrad` (a render with absgrad=True: the
        per-pixel ABSOLUTE screen-space gradients, AbsGS) instead of `.grad`; a ValueError if the attribute is missing.  The
        absolute statistic is larger than the signed one, so densify_and_prune wants a larger threshold: AbsGS used 2-4 x
        the usual 0.0002; no default in this package is tuned for it."""
        self._stats("add_densification_stats", viewspace_point_tensor, None, update_filter, use_absgrad)

    def update_densification_stats(self, viewspace_point_tensor, radii, use_absgrad=False):
        """The loop's two statistics lines in one launch: rows with radii > 0 are visible; on them max_radii2D =
        max(max_radii2D, radii) and add_densification_stats' update (use_absgrad: see there)."""
        self._stats("update_densification_stats", viewspace_point_tensor, radii, None, use_absgrad)

    def _checked_groups(self, in_place=False):
        """(P, device, M, [[parameter, exp_avg, exp_avg_sq] per group, None for absent moments]) of the six groups, every
        tensor checked: float32, on the parameters' device, the group's shape.  in_place: the tensors themselves (which
        must then be contiguous) instead of contiguous copies."""
        P, dev = int(self._xyz.shape[0]), self._xyz.device
        if self._features_rest.dim() != 3:
            raise ValueError("density control: _features_rest must be [P, M - 1, 3]")
        M = 1 + int(self._features_rest.shape[1])
        if not 1 <= M <= 16:
            raise ValueError(f"density control: at most 16 SH coefficients per channel (have {M})")
        shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, M - 1, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
        groups = self._own_groups() or {}
        src = []
        for name, attr in PARAM_GROUPS:
            param = getattr(self, attr)
            state = self.optimizer.state.get(groups[name]["params"][0]) if name in groups else None
            has = state is not None and "exp_avg" in state
            ins = [param.detach()] + ([state["exp_avg"], state["exp_avg_sq"]] if has else [])
            for t in ins:
                if t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != shapes[name]:
                    raise ValueError(f"density control: {attr} and its Adam moments must be float32 {list(shapes[name])} on {dev}")
                if in_place and not t.is_contiguous():
                    raise ValueError(f"density control: {attr} and its Adam moments must be contiguous (they are updated in place)")
            src.append([t if in_place else t.contiguous() for t in ins] + ([] if has else [None, None]))
        return P, dev, M, src

    def _regather(self, plan):
        """plan(context, stream, tmp pointer, tmp bytes, counts) fills the source map and the counts and returns the noise (or
        None); one launch then writes every parameter and Adam moment at the new size, and the six nn.Parameters and their
        optimizer state are swapped.  Every tensor is checked BEFORE the plan is launched: the kernels read P rows of the
        widths below.  Returns (new row count, gather), gather(t) being the rows of another float32 [P, ...] tensor."""
        from . import _capi
        P, dev, M, src = self._checked_groups()
        cx, stream = _capi.context_and_stream(dev)
        nbytes = cx.lib.ggd_densify_tmp_bytes(P)
        if nbytes == 0:
            raise ValueError(f"density control: at most 2^26 rows (have {P})")
        tmp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        counts = (C.c_int64 * 4)()
        st, tp = C.c_void_p(stream), _ptr(tmp)
        with torch.cuda.device(dev):
            noise = plan(cx, st, tp, nbytes, counts)
            new_P = int(counts[3])
            out = self._fresh_groups(src, new_P, cx)
            cx.check(cx.lib.ggd_densify_emit(cx.handle, st, P, new_P, M, _group_table(src), _group_table(out), _ptr(noise), tp, nbytes))
        self._adopt_groups(out)

        def gather(t, plan_buffer=tmp):                  # (holds the scratch with the source map alive)
            t = t.contiguous()
            res = torch.empty((new_P,) + tuple(t.shape[1:]), device=dev)
            with torch.cuda.device(dev):
                cx.check(cx.lib.ggd_densify_gather(cx.handle, st, P, new_P, t.numel() // max(P, 1) or 1, _ptr(t), _ptr(res), tp, nbytes))
            return res
        return new_P, gather

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, noise=None):
        """Clone, split (2 children) and prune in one pass, with the final state of the reference's sequence (see
        csrc/ggd_densify.hip for the per-row rule).  noise: standard-normal [2, P, 3] device tensor for the children's
        offsets (drawn here when None).  The statistics restart at zero at the new size."""
        P = self._device_rows("densify_and_prune")
        if not max_grad > 0:
            raise ValueError("densify_and_prune: max_grad must be > 0 (a clone's zero statistic would satisfy the split test)")
        dev = self._xyz.device
        for t in (self.xyz_gradient_accum, self.denom):
            if tuple(t.shape) != (P, 1) or t.dtype != torch.float32 or t.device != dev:
                raise ValueError(f"densify_and_prune: call training_setup first (float32 statistics [{P}, 1] on {dev} expected)")
        if noise is None:
            noise = torch.randn((2, P, 3), device=dev)
        elif not (isinstance(noise, torch.Tensor) and noise.is_cuda):
            raise RuntimeError("densify_and_prune: noise must be a HIP device tensor (there is no CPU fallback)")
        elif noise.dtype != torch.float32 or tuple(noise.shape) != (2, P, 3):
            raise ValueError(f"densify_and_prune: noise must be float32 [2, {P}, 3]")
        noise = noise.contiguous()
        accum, denom = self.xyz_gradient_accum.contiguous(), self.denom.contiguous()
        scaling, opacity = self._scaling.detach().contiguous(), self._opacity.detach().contiguous()

        def plan(cx, stream, tmp, nbytes, counts):
            cx.check(cx.lib.ggd_densify_plan(cx.handle, stream, P, _ptr(accum), _ptr(denom), _ptr(scaling), _ptr(opacity),
                                             float(max_grad), float(self.percent_dense * extent), float(min_opacity),
                                             int(bool(max_screen_size)), float(0.1 * extent), tmp, nbytes, counts))
            return noise
        new_P, _ = self._regather(plan)
        self.xyz_gradient_accum = torch.zeros((new_P, 1), device=dev)
        self.denom = torch.zeros((new_P, 1), device=dev)
        self.max_radii2D = torch.zeros((new_P,), device=dev)

    def prune_points(self, mask):
        """Drops the rows where the bool mask is set, from every parameter, Adam moment and statistic."""
        P = self._device_rows("prune_points")
        if not (isinstance(mask, torch.Tensor) and mask.is_cuda):
            raise RuntimeError("prune_points: mask must be a HIP device tensor (there is no CPU fallback)")
        if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (P,):
            raise ValueError(f"prune_points: mask must be bool [{P}]")
        m8 = mask.contiguous().view(torch.uint8)

        def plan(cx, stream, tmp, nbytes, counts):
            cx.check(cx.lib.ggd_prune_plan(cx.handle, stream, P, _ptr(m8), tmp, nbytes, counts))
            return None
        stats = [(n, getattr(self, n)) for n in ("xyz_gradient_accum", "denom", "max_radii2D")]
        stats = [(n, t) for n, t in stats if isinstance(t, torch.Tensor) and t.shape[:1] == (P,)]
        for n, t in stats:
            if t.dtype != torch.float32 or t.device != self._xyz.device or t.numel() != P:
                raise ValueError(f"prune_points: {n} must be float32 with one value per row on {self._xyz.device}")
        _, gather = self._regather(plan)
        for n, t in stats:                                # the same source map, one small launch each, no host wait
            setattr(self, n, gather(t))

    # ---- pruning by what the rendered frames used (contribution.py, csrc/ggd_contribution.hip) -------
    def _contribution_stats(self, who, stats):
        from .contribution import ContributionStats
        P = int(self._xyz.shape[0])
        if not isinstance(stats, ContributionStats):
            raise ValueError(f"{who}: stats must be a ContributionStats (got {type(stats).__name__})")
        if stats.P != P or stats.raw.device != self._xyz.device:
            raise ValueError(f"{who}: stats hold {stats.P} rows on {stats.raw.device}, the model {P} on {self._xyz.device}")
        return P

    def importance(self, stats, kind="sum", volume_power=0.1):
        """float32 [P]: the score a pruning ranks by, from the accumulated contribution statistics of rendered frames.  "sum": the
        summed blend weight (Mini-Splatting, gsplat); "max": the largest blend weight (RadSplat); "count": the pixel count;
        "lightgaussian": LightGaussian's global significance, pixel_count * opacity * clamp(V / V_90, 0, 1)^volume_power with V the
        product of the activated scales and V_90 its 90th percentile -- that project's code is not part of the reference tree, so
        the rule is restated here from the paper (Fan et al. 2023, section 3.2)."""
        self._contribution_stats("importance", stats)
        if kind != "lightgaussian":
            return stats.score(kind)
        with torch.no_grad():
            volume = self.get_scaling.detach().to(torch.float32).prod(dim=1)
            v90 = torch.quantile(volume, 0.9) if volume.numel() else volume.new_zeros(())
            norm = torch.clamp(volume / v90, 0.0, 1.0) ** float(volume_power)
            return stats.pixel_count.to(torch.float32) * self.get_opacity.detach().to(torch.float32).reshape(-1) * norm

    def contribution_prune_mask(self, stats, keep_fraction=None, min_max_weight=None, kind="sum"):
        """bool [P], set where prune_by_contribution drops the row: weight_max < min_max_weight, and / or outside the top
        ceil(keep_fraction P) rows by importance(kind) (ties: the lower index first, by a stable sort).  Torch ops only."""
        P = self._contribution_stats("prune_by_contribution", stats)
        if keep_fraction is None and min_max_weight is None:
            raise ValueError("prune_by_contribution: give keep_fraction, min_max_weight or both")
        drop = torch.zeros((P,), dtype=torch.bool, device=self._xyz.device)
        if min_max_weight is not None:
            drop |= stats.weight_max < float(min_max_weight)
        if keep_fraction is not None:
            if not 0.0 <= float(keep_fraction) <= 1.0:
                raise ValueError(f"prune_by_contribution: keep_fraction must lie in [0, 1] (got {keep_fraction})")
            keep = min(P, int(math.ceil(float(keep_fraction) * P)))
            order = torch.sort(self.importance(stats, kind), descending=True, stable=True).indices
            drop[order[keep:]] = True
        return drop

    def prune_by_contribution(self, stats, keep_fraction=None, min_max_weight=None, kind="sum"):
        """Drops the rows the accumulated statistics mark as unused -- contribution_prune_mask's rule -- from every parameter, Adam
        moment and statistic (prune_points).  Returns the number of rows kept.  `stats` describe the rows before the call: reset
        or rebuild them afterwards."""
        mask = self.contribution_prune_mask(stats, keep_fraction, min_max_weight, kind)
        self.prune_points(mask)
        return int(self._xyz.shape[0])

    # ---- density control under a fixed budget (csrc/ggd_mcmc.hip) -----------------------------------
    def _mcmc_argument(self, who, name, t, dtypes, shape):
        """An optional tensor argument of the three methods below: dtype and shape (ValueError), then the device (RuntimeError)."""
        if t is None:
            return None
        what = f"{who}: {name} must be {' / '.join(str(d).replace('torch.', '') for d in dtypes)} {list(shape)}"
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or tuple(t.shape) != tuple(shape):
            raise ValueError(what)
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {name} must be a HIP device tensor (there is no CPU fallback)")
        if t.device != self._xyz.device:
            raise ValueError(what + f" on {self._xyz.device}")
        return t.contiguous()

    def _mcmc_ready(self, who):
        P = self._device_rows(who)
        if self.optimizer is None:
            raise ValueError(f"{who}: call training_setup first")
        return P

    @staticmethod
    def _mcmc_plan_tensors(tmp, P, n_dest):
        """The plan left in the scratch of a relocate / add call, as int64 device tensors (copies)."""
        lay = mcmc_tmp_layout(P, n_dest)
        words = lambda off, n: tmp[off:off + 4 * n].view(torch.int32).to(torch.int64)
        return {"weights": words(lay["weights"], P), "sources": words(lay["sources"], n_dest), "counts": words(lay["counts"], P)}

    @torch.no_grad()
    def relocate_gs(self, dead_mask=None, draws=None, return_plan=False):
        """MCMC relocation (Kheradmand et al. 2024, relocate_gs), in place and without a host read-back: every dead row
        (dead_mask: bool [P]; None: sigmoid(opacity) <= 0.005, evaluated on the device) becomes a copy of an alive row
        sampled in proportion to its opacity, source and copies share the relocation values of compute_relocation (N = 1 +
        the times the source was drawn, at most 51), and the Adam moments of the sources restart at zero.  draws: int64 [P]
        in [0, 2^32), entry j decides for row j when it is dead (default: torch.randint on the device).  Nothing alive or
        nothing dead: no tensor changes.  return_plan=True returns {"weights", "sources", "counts"}: int64 device tensors [P],
        the integer weights (0 on dead rows), each dead row's source (-1 elsewhere) and how often each row was drawn."""
        who = "relocate_gs"
        P = int(self._xyz.shape[0]) if isinstance(self._xyz, torch.Tensor) else 0
        dead_mask = self._mcmc_argument(who, "dead_mask", dead_mask, (torch.bool, torch.uint8), (P,))
        draws = self._mcmc_argument(who, "draws", draws, (torch.int64,), (P,))
        P = self._mcmc_ready(who)
        from . import _capi
        P, dev, M, io = self._checked_groups(in_place=True)
        if draws is None:
            draws = torch.randint(0, 1 << 32, (P,), dtype=torch.int64, device=dev)
        cx, stream = _capi.context_and_stream(dev)
        nbytes = cx.lib.ggd_mcmc_tmp_bytes(P, P)
        if P > 0 and nbytes == 0:
            raise ValueError(f"{who}: at most 2^26 rows (have {P})")
        tmp = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
        if P > 0:
            mask8 = dead_mask.view(torch.uint8) if dead_mask is not None else None
            with torch.cuda.device(dev):
                cx.check(cx.lib.ggd_mcmc_relocate(cx.handle, C.c_void_p(stream), P, M, _group_table(io), _ptr(mask8), _ptr(draws),
                                                  _ptr(tmp), nbytes))
        if return_plan:
            return self._mcmc_plan_tensors(tmp, P, P)

    @torch.no_grad()
    def add_new_gs(self, cap_max, draws=None, return_plan=False):
        """MCMC growth (add_new_gs): the model grows to min(cap_max, int(1.05 P)) rows; each new row is a copy of a row
        sampled in proportion to its opacity, with the relocation values shared as in relocate_gs, zero Adam moments for the
        new rows and the sampled sources, and zero statistics for the new rows.  draws: int64 [num] in [0, 2^32).  Returns
        the number of rows added (0 at the cap: nothing changes); with return_plan=True, (number, plan) with the plan of
        relocate_gs (sources: [num]) or None when nothing was added."""
        who = "add_new_gs"
        P = int(self._xyz.shape[0]) if isinstance(self._xyz, torch.Tensor) else 0
        num = max(0, min(int(cap_max), int(1.05 * P)) - P)
        draws = self._mcmc_argument(who, "draws", draws, (torch.int64,), (num,))
        P = self._mcmc_ready(who)
        if num == 0:
            return (0, None) if return_plan else 0
        from . import _capi
        P, dev, M, src = self._checked_groups()
        if draws is None:
            draws = torch.randint(0, 1 << 32, (num,), dtype=torch.int64, device=dev)
        cx, stream = _capi.context_and_stream(dev)
        nbytes = cx.lib.ggd_mcmc_tmp_bytes(P, num)
        if nbytes == 0 or P + num > 1 << 26:
            raise ValueError(f"{who}: at most 2^26 rows (would have {P + num})")
        tmp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        st, tp = C.c_void_p(stream), _ptr(tmp)
        with torch.cuda.device(dev):
            cx.check(cx.lib.ggd_mcmc_add_plan(cx.handle, st, P, num, _ptr(src[3][0]), _ptr(src[4][0]), _ptr(draws), tp, nbytes))
            out = self._fresh_groups(src, P + num, cx)
            cx.check(cx.lib.ggd_mcmc_add_emit(cx.handle, st, P, num, M, _group_table(src), _group_table(out), tp, nbytes))
        self._adopt_groups(out)
        for n in ("xyz_gradient_accum", "denom", "max_radii2D"):
            t = getattr(self, n)
            if isinstance(t, torch.Tensor) and t.shape[:1] == (P,):
                setattr(self, n, torch.cat((t, torch.zeros((num,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device))))
        return (num, self._mcmc_plan_tensors(tmp, P, num)) if return_plan else num

    @torch.no_grad()
    def inject_position_noise(self, noise_lr, xyz_lr=None, noise=None):
        """The MCMC exploration term, one launch, in place on the positions (call it after optimizer.step):
        xyz += Sigma (gate * noise_lr * xyz_lr * noise) with Sigma = R S^2 R^T of each row and gate = sigmoid(100 ((1 -
        opacity) - 0.995)): transparent rows move, opaque ones stay.  xyz_lr=None reads the xyz group's current rate; noise:
        standard-normal float32 [P, 3] (drawn on the device when None)."""
        who = "inject_position_noise"
        P = int(self._xyz.shape[0]) if isinstance(self._xyz, torch.Tensor) else 0
        noise = self._mcmc_argument(who, "noise", noise, (torch.float32,), (P, 3))
        P = self._mcmc_ready(who)
        from . import _capi
        if xyz_lr is None:
            xyz_lr = self._own_groups()["xyz"]["lr"]
        P, dev, _, io = self._checked_groups(in_place=True)
        if noise is None:
            noise = torch.randn((P, 3), device=dev)
        cx, stream = _capi.context_and_stream(dev)
        with torch.cuda.device(dev):
            cx.check(cx.lib.ggd_mcmc_noise(cx.handle, C.c_void_p(stream), P, _ptr(io[0][0]), _ptr(io[4][0]), _ptr(io[5][0]),
                                           _ptr(io[3][0]), _ptr(noise), float(noise_lr), float(xyz_lr)))
