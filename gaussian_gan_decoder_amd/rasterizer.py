"""PyTorch-facing rasterizer API: the drop-in for the reference's `diff_gaussian_rasterization` module.

Mirrors (names, argument meaning, error behaviour) what the reference imports and calls at
gaussian_splatting/gaussian_renderer/__init__.py:14,38-53,87-95 (render) and :124-139,167-175 (render_simple):

    GaussianRasterizationSettings   NamedTuple of the per-frame parameters
    GaussianRasterizer              nn.Module: .forward(means3D, means2D, opacities, shs=None, colors_precomp=None,
                                    scales=None, rotations=None, cov3D_precomp=None) -> (color[3,H,W], radii[P]);
                                    .markVisible(positions) -> bool[P]
    rasterize_gaussians             functional form, positional arguments as upstream
    _RasterizeGaussians             the autograd.Function; backward returns gradients in INPUT order
                                    (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds, None)

and the three native entry points of upstream's `_C`, here thin wrappers over the C ABI
(include/ggd_raster.h) that pass raw device pointers and the current HIP stream:

    rasterize_gaussians_native / rasterize_gaussians_backward_native / mark_visible

All compute happens in libggd_raster.so (hand-written gfx950 kernels).  Tensors must be CUDA(HIP) fp32; there
is no CPU path -- a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import _capi
from .contribution import check_raw as _check_contribution


class _SettingsFields(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    raw_attributes: bool = False  # extension (default = upstream behaviour): opacities / scales / rotations are the raw
    #                               decoder outputs; sigmoid / exp / normalize are fused into the kernels (fwd + bwd)
    render_depth_alpha: bool = False  # extension: the rasterizer also returns differentiable per-pixel depth
    #                                   (sum alpha_i T_i z_i, view-space z) and alpha (1 - final T) maps, [1, H, W] each


class GaussianRasterizationSettings(_SettingsFields):
    """The settings tuple: upstream's twelve fields, then raw_attributes and render_depth_alpha (extensions).

    antialiasing (keyword only, default False): upstream's flag of the same name -- the opacity-compensated 2D filter,
    each Gaussian's opacity times sqrt(det(cov2D) / det(cov2D + 0.3 I)).  It is an attribute, not a tuple field: upstream's
    13th positional slot is our raw_attributes, and the fields and their positions stay what callers already rely on.

    absgrad (keyword only, default False; gsplat's flag of the same name): the backward also computes the ABSOLUTE
    screen-space gradients of AbsGS -- per Gaussian the sum over pixels of |each pixel's contribution| to means2D.grad's x
    and y -- and sets them as `means2D.absgrad`, a float32 [P, 3] tensor (third column 0), on the means2D tensor the
    rasterizer was called with.  As in gsplat the attribute is OVERWRITTEN by every backward, not accumulated.  An
    attribute like antialiasing, for the same reason.

    render_distortion (keyword only, default False; needs render_depth_alpha=True, refuses absgrad=True): the rasterizer also
    returns the differentiable depth-distortion map sum_ij w_i w_j |z_i - z_j| (w = alpha T, raw view-space z), [1, H, W],
    behind the depth and alpha maps.  An attribute like antialiasing, for the same reason.

    camera_grad (keyword only, default False; refuses absgrad=True): the backward also differentiates the frame in viewmatrix,
    projmatrix and campos, and autograd carries the three gradients on to whatever built those tensors (a pose, for instance).
    The bottom row of viewmatrix and row 2 of projmatrix (maths layout) are read by no kernel and get exactly 0; tanfovx and
    tanfovy get no gradient.  An attribute like antialiasing, for the same reason.

    contribution (keyword only, default None): an int64 [P, 3] device tensor (contribution.ContributionStats.raw) into which the
    forward ACCUMULATES the frame's per-Gaussian contribution statistics -- fixed-point sum, count and maximum of the blend weight
    alpha T over the pixels (ggd_contribution).  No autograd input or output: the returned tuple and the backward are those of
    the call without it.  An attribute like antialiasing, for the same reason."""
    antialiasing: bool = False   # (instances made without __new__, e.g. by _make, read these class defaults)
    absgrad: bool = False
    render_distortion: bool = False
    camera_grad: bool = False
    contribution: Optional[torch.Tensor] = None

    def __new__(cls, *args, antialiasing: bool = False, absgrad: bool = False, render_distortion: bool = False,
                camera_grad: bool = False, contribution: Optional[torch.Tensor] = None, **kwargs):
        self = super().__new__(cls, *args, **kwargs)
        self.antialiasing = bool(antialiasing)
        self.absgrad = bool(absgrad)
        self.render_distortion = bool(render_distortion)
        self.camera_grad = bool(camera_grad)
        self.contribution = contribution
        return self

    def _replace(self, **kwargs):
        aa = kwargs.pop("antialiasing", self.antialiasing)
        ab = kwargs.pop("absgrad", self.absgrad)
        rd = kwargs.pop("render_distortion", self.render_distortion)
        cg = kwargs.pop("camera_grad", self.camera_grad)
        co = kwargs.pop("contribution", self.contribution)
        return type(self)(*super()._replace(**kwargs), antialiasing=aa, absgrad=ab, render_distortion=rd, camera_grad=cg,
                          contribution=co)

    def __repr__(self):
        rd = f", render_distortion={self.render_distortion}" if self.render_distortion else ""
        cg = f", camera_grad={self.camera_grad}" if self.camera_grad else ""
        co = ", contribution=int64[%d, 3]" % self.contribution.shape[0] if isinstance(self.contribution, torch.Tensor) else ""
        return super().__repr__()[:-1] + f", antialiasing={self.antialiasing}, absgrad={self.absgrad}{rd}{cg}{co})"


def _f32c(t: torch.Tensor, name: str, device) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device} (all rasterizer inputs must share a device)")
    if t.dtype != torch.float32:
        # upstream's extension reads every tensor as float32; a silent cast would also make the fp32 gradients of the
        # backward mismatch the leaf's dtype
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    return t.contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return None if (t is None or t.numel() == 0) else C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=4096)
def _sizes(kind: str, a: int, b: int) -> int:
    """ggd_geom_bytes(P) / ggd_img_bytes(W, H) / ggd_binning_bytes(R): pure functions of their arguments, memoised."""
    lib = _capi.load()
    return int(lib.ggd_geom_bytes(a) if kind == "g" else (lib.ggd_img_bytes(a, b) if kind == "i" else lib.ggd_binning_bytes(a)))


_HINT_DECAY = 0.98      # per frame: a one-off large frame is forgotten after ~100 frames (0.98^100 = 0.13)


def _capacity(hint: int) -> int:
    """Instances the binning buffer of a single-call forward is laid out for: 25 % + 64 k above the hint, rounded UP to the
    next value of a geometric grid (2^(k/4)) so that the sizes repeat and the caching allocator reuses its blocks."""
    want = int(hint * 1.25) + 65536
    k = max(0, (want - 1).bit_length() - 1)            # 2^k <= want - 1 < 2^(k+1)
    for q in (1.0, 1.189207115, 1.414213562, 1.681792831, 2.0):
        cap = int(q * (1 << k)) + 1
        if cap >= want:
            return cap
    return want


class _NoGuard:
    def __enter__(self): return None
    def __exit__(self, *a): return False


_NO_GUARD = _NoGuard()


def _device_guard(dev):
    """torch.cuda.device(dev) only when another device is current (the context manager costs ~5 us per call)."""
    idx = dev.index
    return _NO_GUARD if (idx is None or idx == torch.cuda.current_device()) else torch.cuda.device(dev)


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _params(rs: GaussianRasterizationSettings, P: int, M: int, device, keep: list) -> _capi.Params:
    view = _f32c(rs.viewmatrix, "viewmatrix", device)
    proj = _f32c(rs.projmatrix, "projmatrix", device)
    campos = _f32c(rs.campos, "campos", device)
    bg = _f32c(rs.bg, "bg", device)
    if view.numel() != 16 or proj.numel() != 16 or campos.numel() != 3 or bg.numel() != 3:
        raise ValueError("viewmatrix/projmatrix must have 16 elements, campos/bg 3")
    keep += [view, proj, campos, bg]
    return _capi.Params(P, M, int(rs.sh_degree), int(rs.image_width), int(rs.image_height), float(rs.tanfovx),
                        float(rs.tanfovy), float(rs.scale_modifier), int(bool(rs.prefiltered)),
                        int(bool(rs.debug)), view.data_ptr(), proj.data_ptr(), campos.data_ptr(), bg.data_ptr(),
                        int(bool(getattr(rs, "raw_attributes", False))), int(bool(getattr(rs, "antialiasing", False))))


def _require_cuda(t: torch.Tensor):
    if not t.is_cuda:
        raise RuntimeError("gaussian_gan_decoder_amd rasterizer needs HIP device tensors (got a CPU tensor); "
                           "there is no CPU fallback")


def _marshal_inputs(means3D, sh, colors_precomp, scales, rotations, cov3D_precomp, opacities=None):
    """The per-Gaussian inputs of a forward or backward call: (dev, P, (means3D, sh, colors_precomp, opacities, scales, rotations,
    cov3D_precomp)) -- the order of the C entry points -- as contiguous fp32 tensors, None for an absent (None or empty) one.  A
    mis-sized input is a ValueError, not an out-of-bounds read.  opacities: the forward's, converted and counted where the forward
    has always reported them (the backward marshals its own: it reads them in two modes only).  means3D is a device tensor."""
    dev = means3D.device
    P = means3D.size(0)
    means3D = _f32c(means3D, "means3D", dev)
    if opacities is not None:
        opacities = _f32c(opacities, "opacities", dev)
        if opacities.numel() != P:
            raise ValueError("opacities must hold one value per point")
    have = lambda t: t is not None and t.numel() > 0
    sh_c = _f32c(sh, "sh", dev) if have(sh) else None
    col_c = _f32c(colors_precomp, "colors_precomp", dev) if have(colors_precomp) else None
    sc_c = _f32c(scales, "scales", dev) if have(scales) else None
    rot_c = _f32c(rotations, "rotations", dev) if have(rotations) else None
    cov_c = _f32c(cov3D_precomp, "cov3D_precomp", dev) if have(cov3D_precomp) else None
    for t, n, what in ((col_c, 3, "colors_precomp"), (sc_c, 3, "scales"), (rot_c, 4, "rotations"), (cov_c, 6, "cov3D_precomp")):
        if t is not None and t.numel() != P * n:
            raise ValueError(f"{what} must have dimensions (num_points, {n})")
    return dev, P, (means3D, sh_c, col_c, opacities, sc_c, rot_c, cov_c)


def _marshal_forward(bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                     projmatrix, tanfovx, tanfovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
                     raw_attributes=False, antialiasing=False):
    """Validation and marshalling of one forward call, shared by `rasterize_gaussians_native` and `FramePipeline.submit`.
    Returns (dev, P, the seven input tensors (or None) in the order of the C entry points, prm, keep): `keep` holds every tensor
    the C call reads, for as long as it may."""
    _require_cuda(means3D)
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise ValueError("means3D must have dimensions (num_points, 3)")
    if opacities is None:
        raise TypeError("opacities must be a torch.Tensor")
    dev, P, inputs = _marshal_inputs(means3D, sh, colors_precomp, scales, rotations, cov3D_precomp, opacities)
    sh_c = inputs[1]
    if sh_c is not None and (sh_c.dim() != 3 or sh_c.size(0) != P or sh_c.size(2) != 3):
        raise ValueError("sh must have dimensions (num_points, num_coeffs, 3)")
    M = sh_c.size(1) if sh_c is not None else 0
    rs = GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg, scale_modifier,
                                       viewmatrix, projmatrix, degree, campos, prefiltered, debug, raw_attributes,
                                       antialiasing=bool(antialiasing))
    keep: list = list(inputs)
    prm = _params(rs, P, M, dev, keep)
    return dev, P, inputs, prm, keep


def _check_features(features, feature_bg, P: int, absgrad: bool = False):
    """The feature keywords' refusals (ValueError), before any device call: returns C.  features [P, C] with 1 <= C <=
    _capi.FEATURES_MAX_CHANNELS, feature_bg None or C elements."""
    if absgrad:
        raise ValueError("features cannot be combined with absgrad=True: the absolute screen-space statistic is defined on the "
                         "colour terms (with the depth / alpha terms), and the feature map's terms are not part of it")
    if not isinstance(features, torch.Tensor):
        raise TypeError("features must be a torch.Tensor")
    if features.dim() != 2 or features.size(0) != P or features.size(1) < 1:
        raise ValueError(f"features must have dimensions (num_points, C) = ({P}, C) (got {tuple(features.shape)})")
    Cn = int(features.size(1))
    if Cn > _capi.FEATURES_MAX_CHANNELS:
        raise ValueError(f"features has {Cn} channels: at most {_capi.FEATURES_MAX_CHANNELS} are rendered in one pass")
    if feature_bg is not None:
        if not isinstance(feature_bg, torch.Tensor):
            raise TypeError("feature_bg must be a torch.Tensor")
        if feature_bg.numel() != Cn:
            raise ValueError(f"feature_bg must have {Cn} elements, one per feature channel (got {feature_bg.numel()})")
    return Cn


def _check_distortion(render_depth_alpha: bool, absgrad: bool = False):
    """The render_distortion keyword's refusals (ValueError), before any device call."""
    if not render_depth_alpha:
        raise ValueError("render_distortion=True needs render_depth_alpha=True: its backward extends the depth / alpha backward "
                         "(the gradient in z travels through the depth map's accumulator slot)")
    if absgrad:
        raise ValueError("render_distortion cannot be combined with absgrad=True: the absolute screen-space statistic is defined "
                         "on the colour terms (with the depth / alpha terms), and the distortion map's terms are not part of it")


def _check_camera_grad(absgrad: bool = False):
    """The camera_grad keyword's refusal (ValueError), before any device call."""
    if absgrad:
        raise ValueError("camera_grad cannot be combined with absgrad=True: the absolute screen-space statistic is no gradient "
                         "of the frame, and the camera's gradients are not defined on it")


def _bytes(n: int, dev) -> torch.Tensor:
    return torch.empty((n,), dtype=torch.uint8, device=dev)


def _alloc_outputs(dev, P: int, W: int, H: int, depth_alpha: bool = False):
    """A frame's outputs (color, radii, geom, img, depth, alpha); the binning buffer's size depends on the frame's route."""
    color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    depth = torch.empty((1, H, W), dtype=torch.float32, device=dev) if depth_alpha else None
    alpha = torch.empty((1, H, W), dtype=torch.float32, device=dev) if depth_alpha else None
    return color, radii, _bytes(_sizes("g", P, 0), dev), _bytes(_sizes("i", W, H), dev), depth, alpha


def rasterize_gaussians_native(bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier,
                               cov3D_precomp, viewmatrix, projmatrix, tanfovx, tanfovy, image_height, image_width,
                               sh, degree, campos, prefiltered, debug, raw_attributes=False, *, render_depth_alpha=False,
                               antialiasing=False, features=None, feature_bg=None, render_distortion=False,
                               contribution=None):
    """== upstream `_C.rasterize_gaussians(...)`: returns
    (num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer).  binningBuffer may be larger than
    num_rendered needs (single-call forward with a capacity hint); the sorted list sits at its offset 0 either way, so
    the backward takes num_rendered as R exactly like upstream.  render_depth_alpha=True (extension): the tuple goes on
    with the depth and alpha maps, float32 [1, H, W] each (ggd_forward_aux / ggd_forward_render_aux); everything else is
    bit-identical to the plain call.  antialiasing=True (extension): the opacity-compensated 2D filter (ggd_params.antialiasing);
    radii and the three buffers' sort / binning contents are those of the plain call, the colour changes.
    features (extension; float32 [P, C], C <= 32, with feature_bg float32 [C] or None = zeros): one more launch behind the finished
    forward (ggd_forward_features) blends the C channels over the colour's contributors; the map, float32 [C, H, W], is appended
    LAST to the tuple.  Everything in front of it is bit-identical to the call without the keyword.
    render_distortion=True (extension; needs render_depth_alpha=True): one more launch behind the finished forward
    (ggd_forward_distortion) walks the colour's contributors once more; the map, float32 [1, H, W], follows the depth and alpha
    maps and precedes the feature map.  Everything else is bit-identical to the call without the keyword.
    contribution (extension; a contiguous int64 [P, 3] tensor on the inputs' device): one more launch behind the finished forward
    and the two above (ggd_contribution) ACCUMULATES the frame's per-Gaussian statistics into it -- sum of rint(w 2^24), count and
    largest fp32 bits of w = alpha T over the pixels that blended the Gaussian.  The returned tuple is unchanged."""
    if render_distortion:      # (refused before any device call)
        _check_distortion(render_depth_alpha)
    if contribution is not None:   # (likewise)
        _check_contribution(contribution, means3D.size(0), means3D.device)
    if features is not None:   # (likewise)
        n_feat = _check_features(features, feature_bg, means3D.size(0))
    dev, P, inputs, prm, keep = _marshal_forward(
        bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
        tanfovx, tanfovy, image_height, image_width, sh, degree, campos, prefiltered, debug, raw_attributes, antialiasing)
    # (the GPU idles while this wrapper runs between two frames of a render loop: sizes are cached, the stream is looked
    # up once, and the device guard is only entered when another device is current)
    ctx, stream_handle = _capi.context_and_stream(dev)
    lib = ctx.lib
    H, W = int(image_height), int(image_width)
    color, radii, geom, img, depth, alpha = _alloc_outputs(dev, P, W, H, render_depth_alpha)
    aux = (_ptr(depth), _ptr(alpha)) if render_depth_alpha else ()
    R = C.c_int64(0)
    stream = C.c_void_p(stream_handle)
    key = (P, W, H)
    hint = ctx.capacity_hint.get(key)
    head = (ctx.handle, stream, C.byref(prm), *map(_ptr, inputs), _ptr(geom), _ptr(radii))   # every entry point with a per-Gaussian stage begins so
    with _device_guard(dev):
        binning = None
        if hint is not None and P > 0 and not debug:   # debug: exact two-call form, buffers laid out for num_rendered
            # single-call forward: binning buffer sized from the recent frames of this shape (see _capacity); the GPU does
            # not wait for the num_rendered round trip.  Falls through to the exact two-phase path on overflow.
            cap = _capacity(hint)
            binning = _bytes(_sizes("b", cap, 0), dev)
            rc = (lib.ggd_forward_aux if aux else lib.ggd_forward)(*head, _ptr(binning), cap, _ptr(img), _ptr(color), *aux,
                                                                   C.byref(R))
            if rc == -6:       # GGD_E_CAPACITY: R is valid, redo the render phase with an exact buffer
                binning = None
                ctx.capacity_retries += 1
            else:
                ctx.check(rc)
        else:
            ctx.check(lib.ggd_forward_geometry(*head, C.byref(R)))
        if binning is None:
            binning = _bytes(lib.ggd_binning_bytes(R.value), dev)
            ctx.check((lib.ggd_forward_render_aux if aux else lib.ggd_forward_render)(
                ctx.handle, stream, C.byref(prm), _ptr(geom), R.value, _ptr(binning), _ptr(img), _ptr(color), *aux))
    # the hint is a DECAYING RUNNING MAXIMUM of num_rendered, not the last frame's value: consecutive scenes of a training
    # step differ several-fold (the reference draws fov ~ U[5, 17] degrees per scene, target_dataloader.py:71), and with
    # "last frame x 1.25" every upward swing took the overflow -> exact-retry path, i.e. a host sync
    ctx.capacity_hint[key] = max(int(R.value), int((hint or 0) * _HINT_DECAY))
    out = (int(R.value), color, radii, geom, binning, img)
    if render_depth_alpha:
        out = out + (depth, alpha)
    if render_distortion:
        dist = torch.empty((1, H, W), dtype=torch.float32, device=dev)
        with _device_guard(dev):
            ctx.check(lib.ggd_forward_distortion(ctx.handle, stream, C.byref(prm), _ptr(geom), _ptr(binning), _ptr(img),
                                                 int(R.value), _ptr(dist)))
        out = out + (dist,)
    if features is not None:
        feat = _f32c(features, "features", dev)
        fbg = _f32c(feature_bg, "feature_bg", dev) if feature_bg is not None else None
        fmap = torch.empty((n_feat, H, W), dtype=torch.float32, device=dev)
        with _device_guard(dev):
            ctx.check(lib.ggd_forward_features(ctx.handle, stream, C.byref(prm), _ptr(geom), _ptr(binning), _ptr(img), int(R.value),
                                               _ptr(feat), n_feat, _ptr(fbg), _ptr(fmap)))
        out = out + (fmap,)
    if contribution is not None:
        with _device_guard(dev):
            ctx.check(lib.ggd_contribution(ctx.handle, stream, C.byref(prm), _ptr(geom), _ptr(binning), _ptr(img), int(R.value),
                                           _ptr(contribution)))
    return out


class FramePipeline:
    """Several forward frames in flight on one GPU: `slots` HIP streams, each with its own rasterizer context, used round-robin.
    `submit(...)` takes the arguments of `rasterize_gaussians_native`, launches the whole frame on the next slot's stream with
    `ggd_forward_enqueue` and returns WITHOUT waiting for its num_rendered -- the latency-bound front of that frame (per-Gaussian
    kernel, depth sort, binning: about one workgroup per CU) then runs under the blend of the frame before it.  What it returns
    is the result of the frame that used the slot last (None while the pipeline fills): the tuple of
    `rasterize_gaussians_native` plus a `torch.cuda.Event` recorded behind that frame -- make the consuming stream
    `wait_event` it (or synchronise) before reading the tensors.  `drain()` returns the results still pending, oldest first.

    The slot's stream first waits for the stream that is current at `submit`, so inputs produced there are safe to use; every
    input tensor is `record_stream`ed on the slot's stream (the frame's blend may still be reading `bg` when its num_rendered is
    collected and the references are dropped), so per-frame temporaries are safe to pass.  The OUTPUTS are
    allocated on the slot's stream: a consumer on another stream must `wait_event` the returned event and, if it lets go of
    the tensors before its own work on them has finished, `record_stream` them on its stream.  A
    frame for which no capacity hint exists yet (first frame of a shape), a `debug` frame, or one whose binning overflowed
    its capacity is rendered through the ordinary synchronous path on the slot's stream; results are identical either way."""

    def __init__(self, device, slots: int = 2):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("FramePipeline needs a HIP device (there is no CPU fallback)")
        self.slots = [dict(stream=torch.cuda.Stream(device=self.device), pending=None) for _ in range(max(1, int(slots)))]
        self._next = 0
        self.synchronous_frames = 0     # frames that took the ordinary path (no hint yet / overflow / unsupported)

    def _collect(self, slot):
        pend = slot["pending"]
        if pend is None:
            return None
        slot["pending"] = None
        # (the collected frame's binning / blend may still be running -- ggd_forward_collect returns with num_rendered; its inputs
        # were record_stream'ed on this slot's stream at submit, so dropping the references here is safe)
        with torch.cuda.stream(slot["stream"]):
            if "result" in pend:                      # rendered synchronously at submit time
                res = pend["result"]
            else:
                ctx, handle = _capi.context_and_stream(self.device)
                R = C.c_int64(0)
                rc = ctx.lib.ggd_forward_collect(ctx.handle, C.c_void_p(handle), C.byref(R))
                if rc == -6:                          # GGD_E_CAPACITY: this frame's outputs are not valid -- render it again
                    ctx.capacity_retries += 1
                    ctx.capacity_hint[pend["key"]] = max(int(R.value), ctx.capacity_hint.get(pend["key"]) or 0)
                    self.synchronous_frames += 1
                    res = rasterize_gaussians_native(*pend["args"], antialiasing=pend["antialiasing"])
                else:
                    ctx.check(rc)
                    hint = ctx.capacity_hint.get(pend["key"]) or 0
                    ctx.capacity_hint[pend["key"]] = max(int(R.value), int(hint * _HINT_DECAY))
                    res = (int(R.value),) + pend["outputs"]
            ev = torch.cuda.Event()
            ev.record(slot["stream"])
        return res + (ev,)

    def _submit_synchronously(self, slot, args, antialiasing, keep):
        """The frame through the ordinary path on the slot's stream (which is current): no hint yet, P = 0, debug, unsupported."""
        self.synchronous_frames += 1
        slot["pending"] = dict(result=rasterize_gaussians_native(*args, antialiasing=antialiasing), keep=keep)

    def submit(self, bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
               projmatrix, tanfovx, tanfovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
               raw_attributes=False, *, antialiasing=False):
        args = (bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                tanfovx, tanfovy, image_height, image_width, sh, degree, campos, prefiltered, debug, raw_attributes)
        aa = bool(antialiasing)
        slot = self.slots[self._next]
        self._next = (self._next + 1) % len(self.slots)
        prev = self._collect(slot)
        # (validation and marshalling on the CALLER's stream: a conversion to contiguous fp32 is the caller's work)
        dev, P, inputs, prm, keep = _marshal_forward(*args, antialiasing=aa)
        slot["stream"].wait_stream(torch.cuda.current_stream(dev))
        for t in keep:                            # allocated on the caller's stream, read on the slot's: the caching allocator
            if t is not None:                     # must not hand the block out again before the slot's work at the time of the
                t.record_stream(slot["stream"])   # free has run (the blend reads bg long after num_rendered has been collected)
        with torch.cuda.stream(slot["stream"]):
            H, W = int(image_height), int(image_width)
            ctx, handle = _capi.context_and_stream(dev)
            key = (P, W, H)
            hint = ctx.capacity_hint.get(key)
            cap = _capacity(hint) if hint is not None else 0
            lib = ctx.lib
            if hint is None or P == 0 or debug or not lib.ggd_forward_can_speculate(ctx.handle, C.byref(prm), cap):
                self._submit_synchronously(slot, args, aa, keep)
                return prev
            color, radii, geom, img, _, _ = _alloc_outputs(dev, P, W, H)
            binning = _bytes(_sizes("b", cap, 0), dev)
            with _device_guard(dev):
                ctx.check(lib.ggd_forward_enqueue(ctx.handle, C.c_void_p(handle), C.byref(prm), *map(_ptr, inputs), _ptr(geom),
                                                  _ptr(radii), _ptr(binning), cap, _ptr(img), _ptr(color)))
            slot["pending"] = dict(outputs=(color, radii, geom, binning, img), key=key, args=args, antialiasing=aa, keep=keep,
                                   prm=prm)
        return prev

    def drain(self):
        out = []
        n = len(self.slots)
        for k in range(n):                      # oldest first: the slot that would be used next holds the oldest frame
            res = self._collect(self.slots[(self._next + k) % n])
            if res is not None:
                out.append(res)
        return out


def rasterize_gaussians_backward_native(bg, means3D, radii, colors_precomp, scales, rotations, scale_modifier,
                                        cov3D_precomp, viewmatrix, projmatrix, tanfovx, tanfovy, dL_dout_color, sh,
                                        degree, campos, geomBuffer, R, binningBuffer, imgBuffer, debug,
                                        raw_attributes=False, opacities=None, *, dL_ddepth=None, dL_dalpha=None,
                                        antialiasing=False, absgrad=False, features=None, feature_bg=None, dL_dfeatmap=None,
                                        dL_ddistortion=None, camera_grad=False):
    """== upstream `_C.rasterize_gaussians_backward(...)`: returns
    (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations).
    dL_ddepth / dL_dalpha (extension, [1, H, W] or [H, W]; None = zero): gradients of the depth and alpha maps of a
    render_depth_alpha forward -- with either given the call is ggd_backward_aux, else today's ggd_backward.
    antialiasing=True: the backward of an antialiasing forward; it needs `opacities` (the forward's, as passed to it).
    absgrad=True (extension): the call is ggd_backward_abs and a NINTH tensor follows the eight, dL_dmeans2D_abs [P, 3] =
    (0.5 W sum_pixels |g_x|, 0.5 H sum_pixels |g_y|, 0) with g the per-pixel terms whose signed sums are dL_dmeans2D; the
    eight are those of ggd_backward (no dL_ddepth / dL_dalpha) or ggd_backward_aux (either given).
    features (extension; the forward's features [P, C] and feature_bg, with dL_dfeatmap [C, H, W], None = zero): the call is
    ggd_backward_features, the eight hold the gradients of the colour, depth / alpha (when given) AND feature maps together, and
    dL_dfeatures [P, C] follows them.
    dL_ddistortion (extension, [1, H, W] or [H, W]): the gradient of the distortion map of a render_distortion forward -- the call is
    ggd_backward_distortion (which carries the feature map's side as well when `features` is given) and the eight hold the
    gradients of every map together; the depth / alpha instances always run.
    camera_grad=True (extension; refuses absgrad): the call is ggd_backward_camera, which does the work of the entry point the other
    keywords select and then reduces the camera's gradients from the same accumulator records; (dL_dviewmatrix [4, 4],
    dL_dprojmatrix [4, 4], dL_dcampos [3]) follow everything else in the tuple.  Entry [i][j] is the derivative in entry [i][j] of
    the (contiguous) tensor passed in."""
    if camera_grad:
        _check_camera_grad(absgrad)
    if dL_ddistortion is not None:
        _check_distortion(True, absgrad)
    if features is not None:
        n_feat = _check_features(features, feature_bg, means3D.size(0), absgrad)
    if antialiasing and opacities is None:
        raise ValueError("the antialiasing backward needs the opacities of the forward (opacities=None)")
    H, W = int(dL_dout_color.size(-2)), int(dL_dout_color.size(-1))
    aux = dL_ddepth is not None or dL_dalpha is not None
    for t, name in ((dL_ddepth, "dL_ddepth"), (dL_dalpha, "dL_dalpha"), (dL_ddistortion, "dL_ddistortion")):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) not in ((1, H, W), (H, W))):
            raise ValueError(f"{name} must have dimensions (1, {H}, {W}) or ({H}, {W}) (got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__})")
    _require_cuda(means3D)
    dev, P, (means3D, sh_c, col_c, _, sc_c, rot_c, cov_c) = _marshal_inputs(means3D, sh, colors_precomp, scales, rotations, cov3D_precomp)
    M = sh_c.size(1) if sh_c is not None else 0
    g = _f32c(dL_dout_color, "dL_dout_color", dev)
    gD = _f32c(dL_ddepth, "dL_ddepth", dev) if dL_ddepth is not None else None
    gA = _f32c(dL_dalpha, "dL_dalpha", dev) if dL_dalpha is not None else None
    gDist = _f32c(dL_ddistortion, "dL_ddistortion", dev) if dL_ddistortion is not None else None
    rs = GaussianRasterizationSettings(H, W, tanfovx, tanfovy, bg, scale_modifier, viewmatrix, projmatrix, degree,
                                       campos, False, debug, raw_attributes, antialiasing=bool(antialiasing))
    op_c = _f32c(opacities, "opacities", dev) if ((raw_attributes or antialiasing) and opacities is not None) else None
    if antialiasing and op_c.numel() != P:
        raise ValueError("opacities must hold one value per point")
    keep: list = []
    prm = _params(rs, P, M, dev, keep)
    ctx = _capi.context_for(dev)
    # dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations[, dL_dmeans2D_abs]: C order
    shapes = [(P, 3), (P, 3), (P, 1), (P, 3), (P, 6), (P, M, 3), (P, 3), (P, 4)] + ([(P, 3)] if absgrad else [])
    if features is not None:
        shapes.append((P, n_feat))
        feat = _f32c(features, "features", dev)
        fbg = _f32c(feature_bg, "feature_bg", dev) if feature_bg is not None else None
        if dL_dfeatmap is None:
            dL_dfeatmap = torch.zeros((n_feat, H, W), dtype=torch.float32, device=dev)
        gF = _f32c(dL_dfeatmap, "dL_dfeatmap", dev)
        if tuple(gF.shape) != (n_feat, H, W):
            raise ValueError(f"dL_dfeatmap must have dimensions ({n_feat}, {H}, {W}) (got {tuple(gF.shape)})")
    n_per_gaussian = len(shapes)
    if camera_grad:
        shapes += [(4, 4), (4, 4), (3,)]
    grads = [torch.empty(shape, dtype=torch.float32, device=dev) for shape in shapes]
    if ctx.poison_outputs:   # tests: the library must write every element itself (it does not rely on pre-zeroed arrays)
        for t in grads:
            t.fill_(float("nan"))
    if P > 0:
        # the arguments the three entry points share, then the incoming gradients, then the results
        args = [ctx.handle, _stream(dev), C.byref(prm), _ptr(means3D), _ptr(sh_c), _ptr(col_c), _ptr(op_c), _ptr(sc_c),
                _ptr(rot_c), _ptr(cov_c), _ptr(radii), _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imgBuffer), int(R), _ptr(g)]
        if aux or absgrad or features is not None or gDist is not None or camera_grad:
            args += [_ptr(gD), _ptr(gA)]
        if gDist is not None or camera_grad:   # ggd_backward_aux's arguments, then the map's gradient and the feature bundle (or NULL)
            side = None
            if features is not None:
                side = C.byref(_capi.FeatureSide(feat.data_ptr(), n_feat, None if fbg is None else fbg.data_ptr(), gF.data_ptr(),
                                                 grads[n_per_gaussian - 1].data_ptr()))
            args += [_ptr(t) for t in grads[:8]] + [_ptr(gDist), side]
            fn = ctx.lib.ggd_backward_distortion
            if camera_grad:   # ... and the bundle of the three results
                args.append(C.byref(_capi.CameraGrads(*(t.data_ptr() for t in grads[n_per_gaussian:]))))
                fn = ctx.lib.ggd_backward_camera
        else:
            if features is not None:
                args += [_ptr(feat), n_feat, _ptr(fbg), _ptr(gF)]
            args += [_ptr(t) for t in grads]
            fn = ctx.lib.ggd_backward_abs if absgrad else (ctx.lib.ggd_backward_aux if aux else ctx.lib.ggd_backward)
            if features is not None:
                fn = ctx.lib.ggd_backward_features
        with torch.cuda.device(dev):
            ctx.check(fn(*args))
    elif camera_grad:   # (no Gaussian: no call, and the sums are empty)
        for t in grads[n_per_gaussian:]:
            t.zero_()
    return tuple(grads)


def mark_visible(positions, viewmatrix, projmatrix):
    """== upstream `_C.mark_visible`: bool[P], True where the point passes the z > 0.2 frustum test."""
    _require_cuda(positions)
    dev = positions.device
    pos = _f32c(positions, "positions", dev)
    view = _f32c(viewmatrix, "viewmatrix", dev)
    proj = _f32c(projmatrix, "projmatrix", dev)
    P = pos.size(0)
    out = torch.empty((P,), dtype=torch.uint8, device=dev)
    ctx = _capi.context_for(dev)
    with torch.cuda.device(dev):
        ctx.check(ctx.lib.ggd_mark_visible(ctx.handle, _stream(dev), P, _ptr(pos), _ptr(view), _ptr(proj), _ptr(out)))
    return out.bool()


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, features=None, feature_bg=None, viewmatrix=None, projmatrix=None, campos=None):
        rs = raster_settings
        # (camera_grad: apply() is called with rs.viewmatrix, rs.projmatrix and rs.campos as three trailing inputs, so that autograd
        # routes their gradients, and the backward returns fourteen.  The kernels read the three from rs: the same tensors)
        ctx.n_inputs = 14 if viewmatrix is not None else (11 if features is not None else 9)
        if viewmatrix is not None:
            _check_camera_grad(bool(getattr(rs, "absgrad", False)))
            ctx.camera_shapes = (viewmatrix.shape, projmatrix.shape, campos.shape)
        depth_alpha = bool(getattr(rs, "render_depth_alpha", False))
        distortion = bool(getattr(rs, "render_distortion", False))
        if distortion:
            _check_distortion(depth_alpha, bool(getattr(rs, "absgrad", False)))
        # (the statistics tensor is no autograd input: it is accumulated into behind the forward and the backward never sees it)
        contribution = getattr(rs, "contribution", None)
        # (apply() is called with the feature pair only when features are given: the backward then returns eleven gradients)
        ctx.has_features = features is not None
        feat_kw = {}
        if features is not None:
            _check_features(features, feature_bg, means3D.size(0), bool(getattr(rs, "absgrad", False)))
            feat_kw = dict(features=features, feature_bg=feature_bg)
        out = rasterize_gaussians_native(
            rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
            rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh, rs.sh_degree,
            rs.campos, rs.prefiltered, rs.debug, getattr(rs, "raw_attributes", False), render_depth_alpha=depth_alpha,
            **({"antialiasing": True} if getattr(rs, "antialiasing", False) else {}), **feat_kw,
            **({"render_distortion": True} if distortion else {}),
            **({"contribution": contribution} if contribution is not None else {}))
        num_rendered, color, radii, geom, binning, img = out[:6]
        ctx.raster_settings = rs
        ctx.num_rendered = num_rendered
        # absgrad: the backward sets `.absgrad` on the tensor the CALLER holds (inside apply() the inputs are the caller's own
        # objects), so it is kept by reference, not saved for backward
        ctx.means2D_ref = means2D if getattr(rs, "absgrad", False) else None
        if features is not None:
            # (feature_bg gets no gradient; saved as given -- None is allowed)
            ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom, binning,
                                  img, opacities, features, feature_bg)
            ctx.mark_non_differentiable(radii)
            ctx.set_materialize_grads(False)
            return (color, radii) + tuple(out[6:-1]) + (out[-1],)   # (depth, alpha[, distortion]), features
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom, binning,
                              img, opacities)
        ctx.mark_non_differentiable(radii)
        if depth_alpha:
            # unused outputs arrive as None in the backward: a graph that only reads the colour takes today's backward
            ctx.set_materialize_grads(False)
            return (color, radii) + tuple(out[6:])   # depth, alpha[, distortion]
        return color, radii

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, *grad_maps):
        rs = ctx.raster_settings
        features = feature_bg = grad_features = None
        if ctx.has_features:   # the map's gradient is the last one: (depth, alpha,) features
            *grad_maps, grad_features = grad_maps
            *saved, features, feature_bg = ctx.saved_tensors
        else:
            saved = ctx.saved_tensors
        grad_depth, grad_alpha, grad_distortion = (tuple(grad_maps) + (None, None, None))[:3]
        colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom, binning, img, opacities = saved
        raw = getattr(rs, "raw_attributes", False)
        aa = bool(getattr(rs, "antialiasing", False))   # (its backward reads the opacities, raw or not)
        if grad_out_color is None:   # (render_depth_alpha: gradients are not materialised)
            grad_out_color = torch.zeros((3, int(rs.image_height), int(rs.image_width)), dtype=torch.float32,
                                         device=means3D.device)
        aux = {}
        if grad_depth is not None or grad_alpha is not None:
            aux = dict(dL_ddepth=grad_depth, dL_dalpha=grad_alpha)
        if aa:   # (only when set: a plain render calls the backward exactly as before)
            aux["antialiasing"] = True
        absgrad = bool(getattr(rs, "absgrad", False))
        if absgrad:   # (likewise)
            aux["absgrad"] = True
        if ctx.has_features:
            aux.update(features=features, feature_bg=feature_bg, dL_dfeatmap=grad_features)
        if grad_distortion is not None:   # (a graph that does not read the map takes the backward it took without it)
            aux["dL_ddistortion"] = grad_distortion
        # (a camera none of whose three tensors needs a gradient takes the backward it took without the flag)
        want_camera = ctx.n_inputs == 14 and any(ctx.needs_input_grad[11:14])
        if want_camera:
            aux["camera_grad"] = True
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
         grad_rotations, *grad_abs) = rasterize_gaussians_backward_native(
            rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
            rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, sh, rs.sh_degree, rs.campos, geom,
            ctx.num_rendered, binning, img, rs.debug, raw, opacities if (raw or aa) else None, **aux)
        if absgrad and isinstance(ctx.means2D_ref, torch.Tensor):
            ctx.means2D_ref.absgrad = grad_abs[0]   # gsplat's convention: overwritten by each backward, not accumulated
        grads = (grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_opacities, grad_scales,
                 grad_rotations, grad_cov3Ds_precomp, None)
        grad_camera = (None, None, None)
        if want_camera:   # (the three follow everything else)
            *grad_abs, dview, dproj, dcampos = grad_abs
            grad_camera = tuple(g.reshape(shape) if need else None for g, shape, need in
                                zip((dview, dproj, dcampos), ctx.camera_shapes, ctx.needs_input_grad[11:14]))
        if ctx.n_inputs > 9:   # (dL_dfeatures is the last per-Gaussian array; feature_bg gets no gradient)
            grads = grads + (grad_abs[-1] if ctx.has_features else None, None)
        if ctx.n_inputs == 14:
            grads = grads + grad_camera
        return grads


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, features=None, feature_bg=None):
    """features / feature_bg (extension, keywords): C <= 32 per-Gaussian channels [P, C] blended over the colour's contributors; the
    map [C, H, W] is appended LAST to the returned tuple (colour, radii[, depth, alpha], features) and is differentiable in
    `features` and in everything alpha and T depend on.  Without `features` the call is exactly what it was.
    raster_settings.camera_grad (extension): viewmatrix, projmatrix and campos of the settings join the autograd inputs, and a
    backward also fills the gradients of those of them that require one."""
    absgrad = bool(getattr(raster_settings, "absgrad", False))
    camera = bool(getattr(raster_settings, "camera_grad", False))
    if camera:
        _check_camera_grad(absgrad)
    if features is None:
        if feature_bg is not None:
            raise ValueError("feature_bg without features")
        extra = (None, None) if camera else ()
    else:
        _check_features(features, feature_bg, means3D.size(0), absgrad)
        _require_cuda(means3D)
        extra = (features, feature_bg)
    if camera:   # (the feature pair, given or not, then the three camera tensors)
        extra += (raster_settings.viewmatrix, raster_settings.projmatrix, raster_settings.campos)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                     raster_settings, *extra)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        with torch.no_grad():
            rs = self.raster_settings
            return mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, features=None, feature_bg=None):
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        empty = torch.empty(0, dtype=torch.float32, device=means3D.device)
        shs = empty if shs is None else shs
        colors_precomp = empty if colors_precomp is None else colors_precomp
        scales = empty if scales is None else scales
        rotations = empty if rotations is None else rotations
        cov3D_precomp = empty if cov3D_precomp is None else cov3D_precomp
        if features is None and feature_bg is None:
            return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                       cov3D_precomp, rs)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, rs, features=features, feature_bg=feature_bg)
