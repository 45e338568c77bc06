"""render() / render_simple(): the callers of the rasterizer, with the reference's signatures and result dicts.

Mirrors gaussian_splatting/gaussian_renderer/__init__.py:19-102 (render, stock 3DGS) and :105-186 (render_simple,
what main/train_pano2gaussian_decoder.py:232, main/eval.py:38,84 and main/load_decoder.py:24 call).  Differences,
both deliberate: tensors are created on the device of `pc.get_xyz` instead of a hard-coded "cuda" (reference
:28,:114), and the rasterizer behind it is the gfx950 library instead of the CUDA submodule.

`viewpoint_camera` duck-type: FoVx FoVy image_height image_width world_view_transform full_proj_transform
camera_center.  `pc` duck-type: get_xyz get_opacity get_scaling get_rotation get_features active_sh_degree
max_sh_degree get_covariance().
"""
from __future__ import annotations

import math

import torch

from . import _capi
from .contribution import resolve as _resolve_contribution
from .normals import gaussian_normals
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer, _check_camera_grad, _check_distortion
from .sh import eval_sh


def _screenspace_points(pc):
    # zero tensor whose .grad receives dL/d(screen-space mean) -- densification statistics upstream
    pts = torch.zeros_like(pc.get_xyz, dtype=pc.get_xyz.dtype, requires_grad=True) + 0
    try:
        pts.retain_grad()
    except Exception:
        pass
    return pts


def _check_normals(features, feature_bg, absgrad, camera_grad, cov3D_python=False):
    """The render_normals keyword's refusals (ValueError), before anything is built: returns the caller's channel count C."""
    if absgrad:
        raise ValueError("render_normals cannot be combined with absgrad=True: the normals ride the feature pass, which refuses it")
    if camera_grad:
        raise ValueError("render_normals cannot be combined with camera_grad=True: the normals' dependence on the view matrix is "
                         "not differentiated, and the camera's gradient would be silently incomplete")
    if cov3D_python:
        raise ValueError("render_normals needs scales and rotations: pipe.compute_cov3D_python hands the rasterizer neither")
    if features is None and feature_bg is not None:
        raise ValueError("feature_bg without features")
    if features is not None and features.dim() != 2:
        raise ValueError(f"features must have dimensions (num_points, C) (got {tuple(features.shape)})")
    Cn = 0 if features is None else int(features.shape[1])
    if Cn + 3 > _capi.FEATURES_MAX_CHANNELS:
        raise ValueError(f"render_normals adds 3 channels to the caller's {Cn}: at most {_capi.FEATURES_MAX_CHANNELS} are rendered "
                         "in one pass")
    return Cn


def _with_normals(features, feature_bg, rotations, scales, means3D, viewpoint_camera, raw):
    """The feature keywords of a render_normals call: the Gaussians' normals as three channels behind the caller's (background 0)."""
    normals = gaussian_normals(rotations, scales, means3D, viewpoint_camera.world_view_transform, raw=raw)
    if features is None:
        return dict(features=normals, feature_bg=None)
    if feature_bg is not None:
        feature_bg = torch.cat([feature_bg.reshape(-1), feature_bg.new_zeros(3)])
    return dict(features=torch.cat([features, normals], 1), feature_bg=feature_bg)


def _split_normals(res, fmap, n_feat):
    """out["features"] (the caller's channels, if any) and out["normals"] from the map of a render_normals call."""
    if n_feat:
        res["features"] = fmap[:n_feat]
    res["normals"] = fmap[n_feat:]


def _settings(viewpoint_camera, pc, bg_color, scaling_modifier, debug, raw_attributes=False, render_depth_alpha=False,
              antialiasing=False, absgrad=False, render_distortion=False, camera_grad=False, contribution=None):
    if render_distortion:   # (refused before anything is built; the keyword reaches the settings only when set)
        _check_distortion(render_depth_alpha, absgrad)
    if camera_grad:         # (likewise)
        _check_camera_grad(absgrad)
    return GaussianRasterizationSettings(
        **({"render_distortion": True} if render_distortion else {}),
        **({"camera_grad": True} if camera_grad else {}),
        **({"contribution": contribution.raw} if contribution is not None else {}),
        raw_attributes=raw_attributes,
        render_depth_alpha=render_depth_alpha,
        antialiasing=antialiasing,
        absgrad=absgrad,
        image_height=int(viewpoint_camera.image_height),
        image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5),
        tanfovy=math.tan(viewpoint_camera.FoVy * 0.5),
        bg=bg_color,
        scale_modifier=scaling_modifier,
        viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform,
        sh_degree=pc.active_sh_degree,
        campos=viewpoint_camera.camera_center,
        prefiltered=False,
        debug=debug,
    )


def render(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None,
           render_depth_alpha=False, antialiasing=False, absgrad=False, features=None, feature_bg=None,
           render_distortion=False, camera_grad=False, contribution=None, render_normals=False):
    """Stock 3DGS render (reference :19-102).  `pipe` needs .debug, .compute_cov3D_python, .convert_SHs_python.
    render_depth_alpha=True (extension): the dict also holds "depth" (sum alpha_i T_i z_i) and "alpha" (1 - final T),
    differentiable float32 [1, H, W] maps.
    antialiasing=True (extension, upstream's GaussianRasterizationSettings flag): the opacity-compensated 2D filter.
    absgrad=True (extension, gsplat's flag): after backward() `out["viewspace_points"].absgrad` holds the absolute
    screen-space gradients (float32 [P, 3], overwritten by each backward) for GaussianModel's use_absgrad statistics.
    features=[P, C] (extension, C <= 32; feature_bg=[C] or None = zeros): the dict also holds "features", the differentiable
    float32 [C, H, W] map sum alpha_i T_i f_i + T_final feature_bg over the colour's contributors, from the same render pass.
    render_distortion=True (extension; needs render_depth_alpha=True, refuses absgrad): the dict also holds "distortion", the
    differentiable float32 [1, H, W] map sum_ij w_i w_j |z_i - z_j| (w = alpha T, z the raw view-space depth of "depth") over the
    colour's contributors -- the distortion loss of Mip-NeRF 360 / 2DGS is its mean times a weight that carries the scene's scale.
    camera_grad=True (extension; refuses absgrad): the backward also differentiates the frame in the camera.  The dict is
    unchanged; the gradients arrive on viewpoint_camera.world_view_transform, .full_proj_transform and .camera_center, and through
    them on whatever built those with differentiable torch ops (CustomCam's `extr`, for instance).  FoVx / FoVy get none.
    render_normals=True (extension; refuses absgrad, camera_grad, pipe.compute_cov3D_python and more than 29 caller's feature
    channels): the dict also holds "normals", the differentiable float32 [3, H, W] map sum alpha_i T_i n_i of the Gaussians'
    camera-facing view-space normals (normals.gaussian_normals of the scales and rotations of this call), blended as three more
    channels of the feature pass -- what normals.fused_normal_loss compares with the depth map's surface.
    contribution=stats (extension; a contribution.ContributionStats of pc's size on its device, or True for a fresh one): the
    frame's per-Gaussian statistics -- summed blend weight alpha T, pixel count, largest blend weight -- are ACCUMULATED into it by
    one more forward-only launch, and the dict holds the object as "contribution".  Everything else in the dict, and the backward,
    are those of the call without it; combines with every keyword above, absgrad included, with or without gradients enabled."""
    stats = None
    if contribution is not None and contribution is not False:   # (refused before anything is built; only then is pc looked at)
        stats = _resolve_contribution(contribution, pc.get_xyz.shape[0], pc.get_xyz.device)
    if render_normals:
        n_feat = _check_normals(features, feature_bg, absgrad, camera_grad, pipe.compute_cov3D_python)
    screenspace_points = _screenspace_points(pc)
    rasterizer = GaussianRasterizer(_settings(viewpoint_camera, pc, bg_color, scaling_modifier, pipe.debug,
                                              render_depth_alpha=render_depth_alpha, antialiasing=antialiasing,
                                              absgrad=absgrad, render_distortion=render_distortion, camera_grad=camera_grad,
                                              contribution=stats))
    scales = rotations = cov3D_precomp = None
    if pipe.compute_cov3D_python:
        cov3D_precomp = pc.get_covariance(scaling_modifier)
    else:
        scales, rotations = pc.get_scaling, pc.get_rotation
    shs = colors_precomp = None
    if override_color is None:
        if pipe.convert_SHs_python:
            feats = pc.get_features
            shs_view = feats.transpose(1, 2).view(-1, 3, (pc.max_sh_degree + 1) ** 2)
            dir_pp = pc.get_xyz - viewpoint_camera.camera_center.repeat(feats.shape[0], 1)
            dir_pp = dir_pp / dir_pp.norm(dim=1, keepdim=True)
            colors_precomp = torch.clamp_min(eval_sh(pc.active_sh_degree, shs_view, dir_pp) + 0.5, 0.0)
        else:
            shs = pc.get_features
    else:
        colors_precomp = override_color
    feat_kw = {} if features is None and feature_bg is None else dict(features=features, feature_bg=feature_bg)
    if render_normals:
        feat_kw = _with_normals(features, feature_bg, rotations, scales, pc.get_xyz, viewpoint_camera, False)
    out = rasterizer(means3D=pc.get_xyz, means2D=screenspace_points, shs=shs, colors_precomp=colors_precomp,
                     opacities=pc.get_opacity, scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp, **feat_kw)
    rendered_image, radii = out[0], out[1]
    res = {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0,
           "radii": radii}
    if render_depth_alpha:
        res["depth"], res["alpha"] = out[2], out[3]
    if render_distortion:
        res["distortion"] = out[4]
    if render_normals:
        _split_normals(res, out[-1], n_feat)
    elif features is not None:
        res["features"] = out[-1]
    if stats is not None:
        stats.frames += 1
        res["contribution"] = stats
    return res


def render_simple(viewpoint_camera, pc, bg_color: torch.Tensor, xyz_offset=None, scaling_modifier=1.0,
                  override_color=None, debug=False, fused_activations=False, render_depth_alpha=False, antialiasing=False,
                  absgrad=False, features=None, feature_bg=None, render_distortion=False, camera_grad=False,
                  contribution=None, render_normals=False):
    """Decoder-path render (reference :105-186): scale/rotation always from the model, SH unless override_color.
    "alpha" and "depth" are the radii placeholders the reference returns (:184-185).
    fused_activations=True (extension): hand the RAW `_opacity/_scaling/_rotation` to the
    rasterizer, which applies sigmoid / exp / normalize (and their Jacobians in the backward) inside its kernels
    instead of three torch elementwise passes each way.
    render_depth_alpha=True (extension): "depth" (sum alpha_i T_i z_i, view-space z; depth / alpha is the expected depth)
    and "alpha" (1 - final T) are the rasterizer's differentiable float32 [1, H, W] maps instead of the placeholders.
    antialiasing=True (extension): the opacity-compensated 2D filter -- each Gaussian's opacity times
    sqrt(det(cov2D) / det(cov2D + 0.3 I)), so that a Gaussian far smaller than a pixel does not grow brighter and thicker
    when zoomed out; combines with fused_activations and render_depth_alpha.
    absgrad=True (extension): as in `render`; combines with all of the above.
    features=[P, C], feature_bg (extension): as in `render` -- "features" is the [C, H, W] map; combines with everything above but
    absgrad.
    render_distortion=True (extension): as in `render` -- "distortion" is the [1, H, W] map; needs render_depth_alpha=True, combines
    with everything above but absgrad.
    camera_grad=True (extension): as in `render` -- the dict is unchanged and the camera's tensors receive gradients; combines with
    everything above but absgrad.
    render_normals=True (extension): as in `render` -- "normals" is the [3, H, W] map, of the normals of the scales and rotations
    this call passes on (raw with fused_activations) at the means it passes on (xyz_offset included); combines with everything
    above but absgrad and camera_grad.
    contribution=stats or True (extension): as in `render` -- "contribution" is the ContributionStats the frame was accumulated
    into; combines with everything above."""
    stats = None
    if contribution is not None and contribution is not False:   # (refused before anything is built; only then is pc looked at)
        stats = _resolve_contribution(contribution, pc.get_xyz.shape[0], pc.get_xyz.device)
    if render_normals:
        n_feat = _check_normals(features, feature_bg, absgrad, camera_grad)
    screenspace_points = _screenspace_points(pc)
    rasterizer = GaussianRasterizer(_settings(viewpoint_camera, pc, bg_color, scaling_modifier, debug,
                                              raw_attributes=fused_activations, render_depth_alpha=render_depth_alpha,
                                              antialiasing=antialiasing, absgrad=absgrad, render_distortion=render_distortion,
                                              camera_grad=camera_grad, contribution=stats))
    means3D = pc.get_xyz
    if xyz_offset is not None:
        means3D = means3D + xyz_offset
    shs = colors_precomp = None
    if override_color is None:
        shs = pc.get_features
    else:
        colors_precomp = override_color
    if fused_activations:
        opacities, scales, rotations = pc._opacity, pc._scaling, pc._rotation
    else:
        opacities, scales, rotations = pc.get_opacity, pc.get_scaling, pc.get_rotation
    feat_kw = {} if features is None and feature_bg is None else dict(features=features, feature_bg=feature_bg)
    if render_normals:
        feat_kw = _with_normals(features, feature_bg, rotations, scales, means3D, viewpoint_camera, fused_activations)
    out = rasterizer(means3D=means3D, means2D=screenspace_points, shs=shs, colors_precomp=colors_precomp,
                     opacities=opacities, scales=scales, rotations=rotations, cov3D_precomp=None, **feat_kw)
    rendered_image, radii = out[0], out[1]
    alpha, depth = (out[3], out[2]) if render_depth_alpha else (radii, radii)
    res = {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0,
           "radii": radii, "alpha": alpha, "depth": depth}
    if render_distortion:
        res["distortion"] = out[4]
    if render_normals:
        _split_normals(res, out[-1], n_feat)
    elif features is not None:
        res["features"] = out[-1]
    if stats is not None:
        stats.frames += 1
        res["contribution"] = stats
    return res
