"""The teacher's feature, depth and mask maps on the device: rays -> composited features, depth and weights.

What the reference does on every training and eval step with ImportanceRenderer.forward (PanoHead
training/volumetric_rendering/renderer.py:100-196, eg3d .../renderer.py:88-140) and MipRayMarcher2 (ray_marcher.py:27-57):
stratified coarse depths, the field (density.sample_field) at the coarse samples, a march, importance resampling of the march's
weights, the field at the fine samples, the union ordered by depth and a second march, whose results TriPlaneGenerator.synthesis
(triplane.py:165-201) reshapes into image_raw's features, image_depth and image_mask.  camera_rays is its RaySampler.

On CUDA tensors render_teacher is csrc/ggd_teacher.hip (C ABI: ggd_teacher_render): three per-ray kernels, one wave64 per ray,
around two launches of the field kernel, and a last kernel that clamps the depths to the call's depth range -- no torch op, no
host wait, scratch in the context's workspace.  render_teacher_torch is the same computation in torch ops around
density.sample_field: the form CPU tensors take, and on CUDA tensors the composition that was available without the kernels
(the baseline they are timed against).

The arithmetic, all fp32 per element:
  coarse depth  fl(t[k] + fl(u * delta)), t = torch.linspace(ray_start, ray_end, Nc) made on the CPU, delta = (ray_end - ray_start)
                / (Nc - 1) formed in double and rounded;     coordinate  fl(o + fl(depth * d));
  field         sample_field(..., want_rgb=True), bit for bit;   crop  sigma = -1e3 where !(|x| <= lim and |z| <= lim), lim =
                box_warp / 2 - triplane_crop formed in double and rounded;
  march         midpoints, softplus(sigma_mid - 1), alpha = 1 - exp(-sigma_mid * delta) (as -expm1), w = alpha * exclusive cumprod(1 - alpha +
                1e-10);   importance  max_pool1d(2, 1, pad 1), avg_pool1d(2, 1), + 0.01, both ends dropped, + 1e-5, normalised,
                cumulative sum, searchsorted(right=True) and the linear interpolation of sample_pdf;
  composite     features = sum w rgb_mid (+ 1 - sum w with white_back), weights = sum w, depth = sum(w depth_mid) / sum w, NaN ->
                +inf, clamped to [min, max] over every sample depth of the call.
For given noise the result is bit-identical from run to run.  No autograd: the teacher runs under no_grad.
"""
from __future__ import annotations

import ctypes as C
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from . import _capi
from .density import ACTIVATIONS, RGB_CHANNELS, _check, _plane_args, sample_field

MIN_COARSE, MAX_SAMPLES = 4, 64
CROPPED_SIGMA = -1e3
_REFUSED = ("disparity_space_sampling", "density_noise", "cull_clouds", "binarize_clouds")

TeacherSamples = namedtuple("TeacherSamples", "depths_coarse depths_fine coords_coarse coords_fine sigma_coarse sigma_fine "
                                              "rgb_coarse rgb_fine")
TeacherSamples.__doc__ = """every stage's values: depths [M, Nc] / [M, Ni], sample coordinates [M, Nc, 3] / [M, Ni, 3], sigma after
the crop rule [M, Nc] / [M, Ni], rgb [M, Nc, 32] / [M, Ni, 32]"""


class TeacherRender(namedtuple("TeacherRender", "features depth weights activation samples")):
    """features [M, 32] (rgb_final), depth [M] (depth_final), weights [M] (weights.sum(2)); samples: TeacherSamples or None"""
    __slots__ = ()

    def images(self, resolution):
        """-> feature_image [N, 32, R, R], depth [N, 1, R, R], mask [N, 1, R, R] as TriPlaneGenerator.synthesis forms them
        (triplane.py:171-201): mask = weights * 1.002 - 0.001, features * 2 - 1 when the rgb activation is "sigmoid"."""
        R = int(resolution)
        M = self.depth.shape[0]
        if R <= 0 or M % (R * R):
            raise ValueError(f"{M} rays are no whole number of {R} x {R} images")
        N = M // (R * R)
        feat = self.features.view(N, R * R, RGB_CHANNELS).permute(0, 2, 1).reshape(N, RGB_CHANNELS, R, R).contiguous()
        if self.activation == "sigmoid":
            feat = feat * 2 - 1
        return feat, self.depth.view(N, 1, R, R), self.weights.view(N, 1, R, R) * (1 + 2 * 0.001) - 0.001

    def geometry(self, resolution):
        """-> depth [N, 1, R, R], weights [N, 1, R, R]: the raw maps, reshaped as images() reshapes them -- what the student's
        depth / alpha renders are supervised against (losses.fused_geometry_loss).  The weights are NOT image_mask's
        weights * 1.002 - 0.001: they stay in [0, 1] with exact zeros where no sample contributed."""
        R = int(resolution)
        M = self.depth.shape[0]
        if R <= 0 or M % (R * R):
            raise ValueError(f"{M} rays are no whole number of {R} x {R} images")
        N = M // (R * R)
        return self.depth.view(N, 1, R, R), self.weights.view(N, 1, R, R)


def camera_rays(cam2world, intrinsics, resolution):
    """RaySampler.forward (training/volumetric_rendering/ray_sampler.py:24-63) in torch ops: cam2world [N, 4, 4], intrinsics
    [N, 3, 3] (normalised, skew honoured) -> origins [N * R^2, 3], unit directions [N * R^2, 3], pixel centres row by row.
    Bit-equal to the reference on the CPU."""
    R = int(resolution)
    if cam2world.dim() != 3 or tuple(cam2world.shape[1:]) != (4, 4) or tuple(intrinsics.shape) != (cam2world.shape[0], 3, 3):
        raise ValueError("cam2world [N, 4, 4] and intrinsics [N, 3, 3] expected")
    if R <= 0:
        raise ValueError("resolution must be positive")
    with torch.no_grad():
        N, dev = cam2world.shape[0], cam2world.device
        centre = cam2world[:, :3, 3]
        fx, fy = intrinsics[:, 0, 0, None], intrinsics[:, 1, 1, None]
        cx, cy, sk = intrinsics[:, 0, 2, None], intrinsics[:, 1, 2, None], intrinsics[:, 0, 1, None]
        steps = torch.arange(R, dtype=torch.float32, device=dev)
        grid = torch.stack(torch.meshgrid(steps, steps, indexing="ij")) * (1.0 / R) + (0.5 / R)       # [row, column] centres
        xy = grid.flip(0).reshape(2, -1).transpose(1, 0).unsqueeze(0).repeat(N, 1, 1)                  # (x, y) per pixel
        x, y = xy[:, :, 0].view(N, -1), xy[:, :, 1].view(N, -1)
        one = torch.ones((N, R * R), device=dev)
        x_lift = (x - cx + cy * sk / fy - sk * y / fy) / fx * one
        y_lift = (y - cy) / fy * one
        points = torch.stack((x_lift, y_lift, one, torch.ones_like(one)), dim=-1)
        world = torch.bmm(cam2world, points.permute(0, 2, 1)).permute(0, 2, 1)[:, :, :3]
        dirs = F.normalize(world - centre[:, None, :], dim=2)
        origins = centre.unsqueeze(1).repeat(1, R * R, 1)
        return origins.reshape(-1, 3).contiguous(), dirs.reshape(-1, 3).contiguous()


@functools.lru_cache(maxsize=32)
def coarse_table(ray_start, ray_end, depth_resolution):
    """(the Nc values of torch.linspace(ray_start, ray_end, Nc) on the CPU, delta in double): what the reference adds its
    jitter to (renderer.py:258-260).  Cached: the kernel takes the table as an argument."""
    return torch.linspace(ray_start, ray_end, depth_resolution), (ray_end - ray_start) / (depth_resolution - 1)


def _arguments(planes_cl, weights, origins, dirs, ray_start, ray_end, depth_resolution, depth_resolution_importance, box_warp,
               plane_axes, triplane_depth, triplane_crop, noise, generator, unsupported):
    for name, value in unsupported.items():
        if name not in _REFUSED:
            raise TypeError(f"render_teacher: unexpected argument {name!r}")
        if value:
            raise ValueError(f"{name} is not supported by the teacher renderer")
    if isinstance(ray_start, str) or isinstance(ray_end, str):
        raise ValueError("ray_start / ray_end: numbers expected ('auto' ray limits are not supported)")
    ray_start, ray_end = float(ray_start), float(ray_end)
    if not ray_start < ray_end or ray_start in (float("inf"), float("-inf")) or ray_end in (float("inf"), float("-inf")):
        raise ValueError("finite ray_start < ray_end expected")
    Nc, Ni = int(depth_resolution), int(depth_resolution_importance)
    if not MIN_COARSE <= Nc <= MAX_SAMPLES:
        raise ValueError(f"depth_resolution = {Nc}: {MIN_COARSE} <= depth_resolution <= {MAX_SAMPLES}")
    if not 0 <= Ni <= MAX_SAMPLES:
        raise ValueError(f"depth_resolution_importance = {Ni}: 0 <= depth_resolution_importance <= {MAX_SAMPLES}")
    if origins.dim() != 2 or origins.shape[1] != 3 or origins.shape != dirs.shape:
        raise ValueError("origins [M, 3] and dirs [M, 3] expected")
    weights, depth, H, W = _check(planes_cl, weights, triplane_depth, plane_axes, (origins, dirs))
    M = int(origins.shape[0])
    if M * (Nc + Ni) >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 samples per call")
    lim = None if triplane_crop is None else float(box_warp) / 2 - float(triplane_crop)
    dev = planes_cl.device
    if noise is None:
        noise = (torch.rand((M, Nc), device=dev, generator=generator), torch.rand((M, Ni), device=dev, generator=generator))
    u_coarse, u_fine = (u.detach().float().contiguous() for u in noise)
    if tuple(u_coarse.shape) != (M, Nc) or tuple(u_fine.shape) != (M, Ni):
        raise ValueError(f"noise: (u_coarse [{M}, {Nc}], u_fine [{M}, {Ni}]) expected")
    if u_coarse.device != dev or u_fine.device != dev:
        raise ValueError("the noise must live on the planes' device")
    return weights, depth, H, W, M, Nc, Ni, ray_start, ray_end, lim, u_coarse, u_fine


def _crop(sigma, coords, lim):
    """triplane_crop_mask (renderer.py:75-86): outside |x| <= lim and |z| <= lim the density is -1e3"""
    if lim is None:
        return sigma
    inside = (coords[..., [0, 2]].abs() <= lim).all(dim=-1)
    return torch.where(inside, sigma, torch.full_like(sigma, CROPPED_SIGMA))


def _march(rgb, sigma, depths, white_back):
    """MipRayMarcher2.run_forward on [1, M, S, C], [1, M, S, 1], [1, M, S, 1] -> features [1, M, C], depth [1, M, 1], w"""
    widths = depths[:, :, 1:] - depths[:, :, :-1]
    rgb_mid = (rgb[:, :, :-1] + rgb[:, :, 1:]) / 2
    sigma_mid = F.softplus((sigma[:, :, :-1] + sigma[:, :, 1:]) / 2 - 1)
    depth_mid = (depths[:, :, :-1] + depths[:, :, 1:]) / 2
    alpha = -torch.expm1(-(sigma_mid * widths))          # 1 - exp(.) without the half ulp of 1 that the subtraction loses
    through = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :, :1]), 1 - alpha + 1e-10], -2), -2)[:, :, :-1]
    w = alpha * through
    features = torch.sum(w * rgb_mid, -2)
    total = w.sum(2)
    depth = torch.nan_to_num(torch.sum(w * depth_mid, -2) / total, float("inf"))
    depth = torch.clamp(depth, torch.min(depths), torch.max(depths))
    if white_back:
        features = features + 1 - total
    return features, depth, w


def _importance(depths, w, u, eps=1e-5):
    """sample_importance / sample_pdf (renderer.py:264-323) on depths [M, Nc], w [M, Nc - 1], u [M, Ni] -> fine depths [M, Ni]"""
    w = F.max_pool1d(w.unsqueeze(1).float(), 2, 1, padding=1)
    w = F.avg_pool1d(w, 2, 1).squeeze(1) + 0.01
    bins = 0.5 * (depths[:, :-1] + depths[:, 1:])
    w = w[:, 1:-1] + eps
    n = w.shape[1]
    pdf = w / torch.sum(w, -1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)
    u = u.contiguous()
    inds = torch.searchsorted(cdf, u, right=True)
    pair = torch.stack([torch.clamp_min(inds - 1, 0), torch.clamp_max(inds, n)], -1).view(u.shape[0], -1)
    cdf_g = torch.gather(cdf, 1, pair).view(u.shape[0], -1, 2)
    bins_g = torch.gather(bins, 1, pair).view(u.shape[0], -1, 2)
    denom = cdf_g[..., 1] - cdf_g[..., 0]
    denom = torch.where(denom < eps, torch.ones_like(denom), denom)
    return bins_g[..., 0] + (u - cdf_g[..., 0]) / denom * (bins_g[..., 1] - bins_g[..., 0])


def render_teacher_torch(planes_cl, weights, origins, dirs, ray_start=2.25, ray_end=3.3, depth_resolution=48,
                         depth_resolution_importance=48, box_warp=1.0, plane_axes="panohead", triplane_depth=3, triplane_crop=0.1,
                         white_back=False, noise=None, generator=None, return_samples=False, **unsupported):
    """render_teacher in torch ops around density.sample_field (the fused field kernel on CUDA tensors, the torch form on CPU
    tensors)."""
    weights, _, _, _, M, Nc, Ni, ray_start, ray_end, lim, u_coarse, u_fine = _arguments(
        planes_cl, weights, origins, dirs, ray_start, ray_end, depth_resolution, depth_resolution_importance, box_warp, plane_axes,
        triplane_depth, triplane_crop, noise, generator, unsupported)
    with torch.no_grad():
        o, d = origins.detach().float()[None, :, None, :], dirs.detach().float()[None, :, None, :]
        table, delta = coarse_table(ray_start, ray_end, Nc)

        def field(depths):
            coords = o + depths * d                                                    # [1, M, S, 3]
            sigma, rgb = sample_field(planes_cl, weights, coords.reshape(-1, 3), box_warp, plane_axes, triplane_depth, want_rgb=True)
            sigma = _crop(sigma.view(1, M, -1, 1), coords.view(1, M, -1, 1, 3), lim)
            return coords, sigma, rgb.view(1, M, -1, RGB_CHANNELS)

        depths_c = table.to(origins.device).reshape(1, 1, Nc, 1).repeat(1, M, 1, 1)
        depths_c += u_coarse.view(1, M, Nc, 1) * delta
        coords_c, sigma_c, rgb_c = field(depths_c)
        if Ni > 0:
            _, _, w = _march(rgb_c, sigma_c, depths_c, white_back)
            depths_f = _importance(depths_c.reshape(M, Nc), w.reshape(M, Nc - 1), u_fine).reshape(1, M, Ni, 1)
            coords_f, sigma_f, rgb_f = field(depths_f)
            depths = torch.cat([depths_c, depths_f], -2)
            order = torch.sort(depths, dim=-2)[1]
            features, depth, w = _march(torch.gather(torch.cat([rgb_c, rgb_f], -2), -2, order.expand(-1, -1, -1, RGB_CHANNELS)),
                                        torch.gather(torch.cat([sigma_c, sigma_f], -2), -2, order),
                                        torch.gather(depths, -2, order), white_back)
        else:
            depths_f, coords_f = depths_c.new_zeros((1, M, 0, 1)), coords_c.new_zeros((1, M, 0, 3))
            sigma_f, rgb_f = sigma_c.new_zeros((1, M, 0, 1)), rgb_c.new_zeros((1, M, 0, RGB_CHANNELS))
            features, depth, w = _march(rgb_c, sigma_c, depths_c, white_back)
        samples = None
        if return_samples:
            samples = TeacherSamples(depths_c.reshape(M, Nc), depths_f.reshape(M, Ni), coords_c.reshape(M, Nc, 3),
                                     coords_f.reshape(M, Ni, 3), sigma_c.reshape(M, Nc), sigma_f.reshape(M, Ni),
                                     rgb_c.reshape(M, Nc, RGB_CHANNELS), rgb_f.reshape(M, Ni, RGB_CHANNELS))
        return TeacherRender(features[0], depth[0, :, 0], w.sum(2)[0, :, 0], weights.activation, samples)


def sample_layout(M, Nc, Ni):
    """(offsets, shapes, total floats) of the sample block ggd_teacher_render fills, in TeacherSamples' field order"""
    sizes = {"rgb_coarse": (M, Nc, RGB_CHANNELS), "rgb_fine": (M, Ni, RGB_CHANNELS), "sigma_coarse": (M, Nc), "sigma_fine": (M, Ni),
             "depths_coarse": (M, Nc), "depths_fine": (M, Ni), "coords_coarse": (M, Nc, 3), "coords_fine": (M, Ni, 3)}
    offsets, at = {}, 0
    for name, shape in sizes.items():      # the order of the block: rgb rows first (16-byte aligned), see include/ggd_raster.h
        n = 1
        for s in shape:
            n *= s
        offsets[name] = at
        at += n
    return offsets, sizes, at


def render_teacher(planes_cl, weights, origins, dirs, ray_start=2.25, ray_end=3.3, depth_resolution=48,
                   depth_resolution_importance=48, box_warp=1.0, plane_axes="panohead", triplane_depth=3, triplane_crop=0.1,
                   white_back=False, noise=None, generator=None, return_samples=False, **unsupported):
    """planes_cl: channel-last planes (decoder.planes_channels_last), weights: osg_weights(...), origins / dirs [M, 3] (camera_rays)
    -> TeacherRender(features [M, 32], depth [M], weights [M]).  noise = (u_coarse [M, Nc], u_fine [M, Ni]) in [0, 1): the
    reference's two rand draws; None draws them with torch.rand on the planes' device (generator honoured).  return_samples adds
    TeacherSamples.  triplane_crop=None with plane_axes="eg3d", triplane_depth=None is EG3D's renderer.  'auto' ray limits,
    disparity_space_sampling, density_noise, cull_clouds and binarize_clouds are refused.  Six HIP launches on CUDA tensors;
    CPU tensors take render_teacher_torch."""
    if not planes_cl.is_cuda:
        return render_teacher_torch(planes_cl, weights, origins, dirs, ray_start, ray_end, depth_resolution,
                                    depth_resolution_importance, box_warp, plane_axes, triplane_depth, triplane_crop, white_back,
                                    noise, generator, return_samples, **unsupported)
    weights, depth, H, W, M, Nc, Ni, ray_start, ray_end, lim, u_coarse, u_fine = _arguments(
        planes_cl, weights, origins, dirs, ray_start, ray_end, depth_resolution, depth_resolution_importance, box_warp, plane_axes,
        triplane_depth, triplane_crop, noise, generator, unsupported)
    dev = planes_cl.device
    planes_cl = planes_cl.detach().contiguous()
    origins, dirs = origins.detach().float().contiguous(), dirs.detach().float().contiguous()
    table, _ = coarse_table(ray_start, ray_end, Nc)
    features = torch.empty((M, RGB_CHANNELS), dtype=torch.float32, device=dev)
    out_depth = torch.empty((M,), dtype=torch.float32, device=dev)
    out_weights = torch.empty((M,), dtype=torch.float32, device=dev)
    offsets, shapes, total = sample_layout(M, Nc, Ni)
    block = torch.empty((total,), dtype=torch.float32, device=dev) if return_samples else None
    vp = C.c_void_p
    cx, stream = _capi.context_and_stream(dev)
    with torch.cuda.device(dev):
        cx.check(cx.lib.ggd_teacher_render(
            cx.handle, vp(stream), *_plane_args(planes_cl, weights, depth, H, W, plane_axes, box_warp), vp(origins.data_ptr()),
            vp(dirs.data_ptr()), M, ray_start, ray_end, vp(table.data_ptr()), Nc, Ni, vp(u_coarse.data_ptr()),
            vp(u_fine.data_ptr()) if Ni else None, int(lim is not None), 0.0 if lim is None else lim, int(bool(white_back)),
            vp(features.data_ptr()), vp(out_depth.data_ptr()), vp(out_weights.data_ptr()),
            vp(block.data_ptr()) if return_samples else None))
    samples = None
    if return_samples:
        def part(name):
            n = 1
            for s in shapes[name]:
                n *= s
            return block[offsets[name]:offsets[name] + n].view(shapes[name])
        samples = TeacherSamples(*(part(name) for name in TeacherSamples._fields))
    return TeacherRender(features, out_depth, out_weights, weights.activation, samples)
