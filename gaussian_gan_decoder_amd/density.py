"""The teacher's density field on the device: feature planes -> sigma (and rgb) at points or on the reference's lattice.

Step 2 of the reference's target loader (main/decoder_utils/target_dataloader.py:134-169): `G.sample_mixed` evaluates the
frozen generator's density on a 128^3 lattice (main/marching_cube/sample.py:5-26, create_samples) -- sample_from_planes, then
OSGDecoder (mean over the three planes, FullyConnectedLayer 32 -> 64, softplus, FullyConnectedLayer 64 -> 1 + 32; eg3d /
PanoHead training/triplane.py) -- and hands the grid to marching cubes.  Here that is ONE HIP launch without intermediate
tensors (csrc/ggd_density.hip; C ABI: ggd_density_points / ggd_density_grid / ggd_density_lattice), and
target_sampler.sample_target_points chains it with the iso-surface sampler.

Three quirks of the reference decide where the iso-surface lands, and all three are part of this module's contract:
  * the lattice is SHEARED: create_samples divides without flooring, so sample i has the y index (i / n) mod n and the x index
    (i / n / n) mod n with their fractional parts (x and y reach 0.5079 at n = 128, past the box, where the zero padding
    applies).  lattice="reference" repeats that arithmetic op for op in fp32; lattice="regular" floors the indices;
  * FullyConnectedLayer applies weight * (lr_mul / sqrt(in)) and bias * lr_mul in fp32: osg_weights() forms those products;
  * softplus is torch's (threshold 20); the rgb activation is "sigmoid" (x * 1.002 - 0.001; EG3D always), "lrelu"
    (leaky_relu 0.2, * sqrt 2) or "none" (PanoHead's decoder_activation option).

No autograd (the teacher runs under no_grad in the reference).  CUDA tensors take the HIP kernel; CPU tensors take the plain
torch form (sample_field_torch), which exists for tests, as the decoder's CPU paths do.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch
import torch.nn.functional as F

from . import _capi
from .decoder import planes_gather, sample_from_planes

PLANE_CHANNELS, HIDDEN, RGB_CHANNELS = 32, 64, 32
MAX_LATTICE = 1024
ACTIVATIONS = {"sigmoid": 0, "lrelu": 1, "none": 2}
LATTICES = {"reference": 0, "regular": 1}
_AXES = {"eg3d": 0, "panohead": 1}


class OSGWeights(namedtuple("OSGWeights", "w1 b1 w2 b2 activation")):
    """effective fp32 weights w1 [64, 32], b1 [64], w2 [33, 64], b2 [33] (row 0 of the second layer: sigma) and the name of
    the rgb activation"""
    __slots__ = ()

    def to(self, device):
        return OSGWeights(*(t.to(device) for t in self[:4]), self.activation)


def _effective(layer):
    """FullyConnectedLayer.forward's own products (networks_stylegan2.py:114-120): weight * weight_gain, bias * bias_gain, the
    gain a Python / numpy scalar that torch's scalar multiply rounds to fp32 first"""
    w = layer.weight.detach().float() * float(getattr(layer, "weight_gain", 1.0))
    b = layer.bias.detach().float() if getattr(layer, "bias", None) is not None else torch.zeros(w.shape[0], device=w.device)
    gain = float(getattr(layer, "bias_gain", 1.0))
    if gain != 1.0:
        b = b * gain
    return w, b


def osg_weights(decoder, b1=None, w2=None, b2=None, activation=None) -> OSGWeights:
    """The effective fp32 weights of an OSGDecoder: osg_weights(decoder) reads .net[0] / .net[2] (.weight, .bias, .weight_gain,
    .bias_gain) and .activation if present (default "sigmoid": EG3D's decoder has no option); osg_weights(w1, b1, w2, b2,
    activation="sigmoid") takes the four effective tensors directly.  An OSGWeights passes through."""
    if isinstance(decoder, OSGWeights):
        return decoder
    if torch.is_tensor(decoder):
        if b1 is None or w2 is None or b2 is None:
            raise TypeError("osg_weights(w1, b1, w2, b2): four tensors expected")
        w1 = decoder
        act = activation or "sigmoid"
    else:
        (w1, b1), (w2, b2) = _effective(decoder.net[0]), _effective(decoder.net[2])
        act = activation or getattr(decoder, "activation", "sigmoid")
    if act not in ACTIVATIONS:
        raise ValueError(f"rgb activation {act!r}: one of {sorted(ACTIVATIONS)}")
    w1, b1, w2, b2 = (t.detach().float().contiguous() for t in (w1, b1, w2, b2))
    if tuple(w1.shape) != (HIDDEN, PLANE_CHANNELS) or tuple(b1.shape) != (HIDDEN,):
        raise ValueError(f"first layer: weight [{HIDDEN}, {PLANE_CHANNELS}] and bias [{HIDDEN}] expected, got "
                         f"{tuple(w1.shape)} and {tuple(b1.shape)}")
    if tuple(w2.shape) != (1 + RGB_CHANNELS, HIDDEN) or tuple(b2.shape) != (1 + RGB_CHANNELS,):
        raise ValueError(f"second layer: weight [{1 + RGB_CHANNELS}, {HIDDEN}] and bias [{1 + RGB_CHANNELS}] expected, got "
                         f"{tuple(w2.shape)} and {tuple(b2.shape)}")
    return OSGWeights(w1, b1, w2, b2, act)


def _check(planes_cl, weights, triplane_depth, plane_axes, others=()):
    """-> (weights, D, H, W); raises on anything the kernel does not take"""
    weights = osg_weights(weights)
    depth = 0 if triplane_depth is None else int(triplane_depth)
    if plane_axes not in _AXES:
        raise ValueError(f"plane_axes {plane_axes!r}: 'eg3d' or 'panohead'")
    if depth == 0 and plane_axes != "eg3d":
        raise ValueError("the 2-D tri-plane form has the EG3D plane axes only")
    want = 4 if depth == 0 else 5
    if planes_cl.dim() != want or planes_cl.shape[0] != 3 or (depth and planes_cl.shape[1] != depth):
        raise ValueError("planes_cl: channel-last [3, H, W, C] (triplane_depth=None) or [3, D, H, W, C] expected "
                         "(decoder.planes_channels_last)")
    if planes_cl.shape[-1] != PLANE_CHANNELS:
        raise ValueError(f"planes_cl has {planes_cl.shape[-1]} channels: the density field takes {PLANE_CHANNELS}")
    if planes_cl.dtype != torch.float32:
        raise TypeError("planes_cl must be float32")
    devs = {t.device for t in (planes_cl,) + tuple(weights[:4]) + tuple(others)}
    if len(devs) != 1:
        raise ValueError(f"planes, weights and coordinates must live on one device, got {sorted(str(d) for d in devs)}")
    return weights, depth, int(planes_cl.shape[-3]), int(planes_cl.shape[-2])


def _activate(x, activation):
    if activation == "sigmoid":
        return torch.sigmoid(x) * (1 + 2 * 0.001) - 0.001
    if activation == "lrelu":
        return F.leaky_relu(x, 0.2) * (2.0 ** 0.5)
    return x


def sample_field_torch(planes_cl, weights, coordinates, box_warp=1.0, plane_axes="eg3d", triplane_depth=None, want_rgb=False):
    """The field in plain torch ops: the plane-mean features, F.linear, F.softplus, F.linear, the activation.  On CUDA tensors the
    features come from the HIP gather (decoder.planes_gather) -- the composition available without the fused kernel, and the
    baseline it is timed against; on CPU tensors from sample_from_planes(...).mean(0)."""
    weights, depth, _, _ = _check(planes_cl, weights, triplane_depth, plane_axes, (coordinates,))
    with torch.no_grad():
        pos = coordinates.detach().reshape(-1, 3).float()
        if planes_cl.is_cuda:
            f = planes_gather(planes_cl.detach().contiguous(), pos, box_warp, plane_axes, triplane_depth)
        else:
            nchw = planes_cl.detach().permute(0, 3, 1, 2) if depth == 0 else \
                planes_cl.detach().permute(0, 4, 1, 2, 3).reshape(3, -1, planes_cl.shape[2], planes_cl.shape[3])
            f = sample_from_planes(nchw.contiguous(), pos, box_warp, plane_axes, triplane_depth).mean(0)
        h = F.softplus(F.linear(f, weights.w1, weights.b1))
        if not want_rgb:
            return F.linear(h, weights.w2[:1], weights.b2[:1])[:, 0]
        o = F.linear(h, weights.w2, weights.b2)
        return o[:, 0].contiguous(), _activate(o[:, 1:], weights.activation).contiguous()


def _plane_args(planes_cl, weights, depth, H, W, plane_axes, box_warp):
    vp = C.c_void_p
    return [vp(planes_cl.data_ptr()), PLANE_CHANNELS, depth, H, W, _AXES[plane_axes], float(box_warp), vp(weights.w1.data_ptr()),
            vp(weights.b1.data_ptr()), vp(weights.w2.data_ptr()), vp(weights.b2.data_ptr()), ACTIVATIONS[weights.activation]]


def sample_field(planes_cl, weights, coordinates, box_warp=1.0, plane_axes="eg3d", triplane_depth=None, want_rgb=False):
    """planes_cl: channel-last planes (decoder.planes_channels_last), weights: osg_weights(...), coordinates [..., 3] ->
    sigma [M] (want_rgb: (sigma [M], rgb [M, 32])), M the number of points.  One HIP launch on CUDA tensors."""
    weights, depth, H, W = _check(planes_cl, weights, triplane_depth, plane_axes, (coordinates,))
    if not planes_cl.is_cuda:
        return sample_field_torch(planes_cl, weights, coordinates, box_warp, plane_axes, triplane_depth, want_rgb)
    dev = planes_cl.device
    planes_cl = planes_cl.detach().contiguous()
    pos = coordinates.detach().reshape(-1, 3).float().contiguous()
    M = int(pos.shape[0])
    if M >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 points per call")
    sigma = torch.empty((M,), dtype=torch.float32, device=dev)
    rgb = torch.empty((M, RGB_CHANNELS), dtype=torch.float32, device=dev) if want_rgb else None
    cx, stream = _capi.context_and_stream(dev)
    with torch.cuda.device(dev):
        cx.check(cx.lib.ggd_density_points(cx.handle, C.c_void_p(stream), *_plane_args(planes_cl, weights, depth, H, W, plane_axes, box_warp),
                                           C.c_void_p(pos.data_ptr()), M, C.c_void_p(sigma.data_ptr()),
                                           C.c_void_p(rgb.data_ptr()) if want_rgb else None))
    return (sigma, rgb) if want_rgb else sigma


def _lattice_args(n, cube_length, lattice):
    n = int(n)
    if not 2 <= n <= MAX_LATTICE:
        raise ValueError(f"n = {n}: 2 <= n <= {MAX_LATTICE}")
    if lattice not in LATTICES:
        raise ValueError(f"lattice {lattice!r}: 'reference' or 'regular'")
    if not float(cube_length) > 0.0:
        raise ValueError("cube_length must be positive")
    return n, float(cube_length), LATTICES[lattice]


def lattice_points(n, cube_length=1.0, lattice="reference", device="cpu"):
    """The n^3 sample positions [n^3, 3] (x, y, z; sample i -> [x][y][z] of the grid, z fastest).  "reference": create_samples'
    arithmetic in fp32 -- z index i mod n, y index fmod(float(i) / n, n), x index fmod((float(i) / n) / n, n), un-floored;
    "regular": floored indices.  Coordinate = fl(fl(index * voxel) + origin) with voxel = cube_length / (n - 1) and origin =
    -cube_length / 2 formed in double and rounded to fp32.  The CPU form is torch ops, the CUDA form one HIP launch; the two are
    bit-identical."""
    n, cube_length, mode = _lattice_args(n, cube_length, lattice)
    dev = torch.device(device)
    if dev.type == "cuda":
        pos = torch.empty((n ** 3, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            cx, stream = _capi.context_and_stream(pos.device)
            cx.check(cx.lib.ggd_density_lattice(cx.handle, C.c_void_p(stream), n, cube_length, mode, C.c_void_p(pos.data_ptr())))
        return pos
    i = torch.arange(n ** 3, dtype=torch.int64)
    fn = torch.tensor(float(n), dtype=torch.float32)
    if mode == 0:
        q = i.to(torch.float32) / fn
        idx = torch.stack([torch.fmod(q / fn, fn), torch.fmod(q, fn), (i % n).to(torch.float32)], 1)
    else:
        idx = torch.stack([i // (n * n), (i // n) % n, i % n], 1).to(torch.float32)
    voxel = torch.tensor(cube_length / (n - 1), dtype=torch.float64).to(torch.float32)
    origin = torch.tensor(-cube_length / 2.0, dtype=torch.float64).to(torch.float32)
    return idx * voxel + origin


def density_grid(planes_cl, weights, n=128, cube_length=None, box_warp=1.0, plane_axes="eg3d", triplane_depth=None,
                 lattice="reference", want_rgb=False):
    """The field on the n^3 lattice -> sigma [n, n, n] ([x][y][z], what sample_surface_points reads; want_rgb: plus rgb
    [n, n, n, 32]).  cube_length defaults to box_warp (target_dataloader.py:135).  On CUDA tensors the coordinates are generated
    inside the kernel; bit-identical to sample_field(lattice_points(...))."""
    cube_length = float(box_warp if cube_length is None else cube_length)
    n, cube_length, mode = _lattice_args(n, cube_length, lattice)
    weights, depth, H, W = _check(planes_cl, weights, triplane_depth, plane_axes)
    if not planes_cl.is_cuda:
        out = sample_field_torch(planes_cl, weights, lattice_points(n, cube_length, lattice), box_warp, plane_axes, triplane_depth,
                                 want_rgb)
        return (out[0].view(n, n, n), out[1].view(n, n, n, RGB_CHANNELS)) if want_rgb else out.view(n, n, n)
    dev = planes_cl.device
    planes_cl = planes_cl.detach().contiguous()
    sigma = torch.empty((n, n, n), dtype=torch.float32, device=dev)
    rgb = torch.empty((n, n, n, RGB_CHANNELS), dtype=torch.float32, device=dev) if want_rgb else None
    cx, stream = _capi.context_and_stream(dev)
    with torch.cuda.device(dev):
        cx.check(cx.lib.ggd_density_grid(cx.handle, C.c_void_p(stream), *_plane_args(planes_cl, weights, depth, H, W, plane_axes, box_warp),
                                         n, cube_length, mode, C.c_void_p(sigma.data_ptr()),
                                         C.c_void_p(rgb.data_ptr()) if want_rgb else None))
    return (sigma, rgb) if want_rgb else sigma
