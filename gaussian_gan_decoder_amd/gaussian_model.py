"""Minimal Gaussian attribute container for the decoder path.

Mirrors the part of gaussian_splatting/scene/gaussian_model.py the raster hot path touches: the constructor
(:47-63), the activation getters that form the rasterizer's input prologue (:100-124: exp / normalize / sigmoid /
pass-through) and get_covariance (:29-33,123-124).  The decoder overwrites `_xyz/_scaling/_rotation/_opacity/
_features_dc` every step (main/train_pano2gaussian_decoder.py:223-227), so densification, the optimizer set-up
and the plyfile import of the reference class are intentionally absent.
create_from_pcd / create_from_pos_col (:126-185) seed a model from a point cloud; their `distCUDA2` is knn.dist_cuda2.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .sh import RGB2SH


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
        self.scaling_activation = torch.exp
        self.scaling_inverse_activation = torch.log
        self.opacity_activation = torch.sigmoid
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
