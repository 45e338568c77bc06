"""Generate tests/golden/teacher_render_fixture.npz: the teacher's rendered feature / depth / weight maps from the REFERENCE's own
code, imported from /root/reference on the CPU:

  PanoHead/training/volumetric_rendering/ray_sampler.py:24-63   RaySampler.forward
  PanoHead/training/volumetric_rendering/renderer.py:100-323    ImportanceRenderer.forward (sample_stratified, run_model, the crop,
                                         sample_importance / sample_pdf, unify_samples)
  PanoHead/training/volumetric_rendering/ray_marcher.py:27-57   MipRayMarcher2.run_forward
  PanoHead/training/triplane.py:300-332  OSGDecoder;  eg3d/training/volumetric_rendering/renderer.py:88-140 and eg3d/training/
                                         triplane.py:116-139 for the EG3D case (its own renderer, no crop)

Run in the build container:  python tests/golden/make_teacher_render_golden.py
Only arrays travel.  torch.rand_like and torch.rand are wrapped while the renderer runs, so the two draws (renderer.py:260 and
:307) are recorded; sample_stratified, sample_importance and run_model are wrapped to record the depths and the per-sample sigma
(after the crop, which the renderer applies in place) and rgb.  Planes are 12 x 10, fp16-valued; raw weights likewise, one set.
Cameras sit at radius 2.7 and look at the origin, fields of view 12-18 degrees, ray limits 2.25 / 3.3.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
H, W = 12, 10
RAY_START, RAY_END, RADIUS = 2.25, 3.3, 2.7
RGB_SPLIT = 2000
NEAR = 1e-5     # a fine sample this close to the crop limit could flip with an ulp of depth: the fixture has none

# (name, teacher, depth (0 = 2-D tri-planes), activation, lr_mul, box_warp, crop, white_back, Nc, Ni, resolution (0: hand-placed))
CASES = [("pano_d3_sigmoid_48_48", "PanoHead", 3, "sigmoid", 1.0, 1.0, 0.1, False, 48, 48, 6),
         ("pano_d1_lrelu_white_8_5", "PanoHead", 1, "lrelu", 2.0, 0.7, 0.05, True, 8, 5, 5),
         ("pano_d3_none_48_0", "PanoHead", 3, "none", 1.0, 1.0, 0.1, False, 48, 0, 4),
         ("eg3d_64_64", "eg3d", 0, "sigmoid", 1.0, 1.0, None, False, 64, 64, 4),
         ("pano_d3_sigmoid_misses_33_64", "PanoHead", 3, "sigmoid", 1.0, 1.0, 0.1, False, 33, 64, 0)]


def fp16_valued(*shape, g, scale=1.0):
    return (scale * torch.randn(*shape, generator=g)).half().float()


def use_teacher(name):
    """put one teacher's `training` / `torch_utils` / `dnnlib` packages first (both trees use the same package names)"""
    for m in [m for m in sys.modules if m.split(".")[0] in ("training", "torch_utils", "dnnlib")]:
        del sys.modules[m]
    sys.path[:] = [p for p in sys.path if not p.startswith(REF)]
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, name))


def look_at_origin(azimuth, elevation, roll=0.0):
    """cam2world [4, 4] of a camera at RADIUS looking at the origin (x right, y down, z forward)"""
    eye = RADIUS * np.array([math.cos(elevation) * math.sin(azimuth), math.sin(elevation), math.cos(elevation) * math.cos(azimuth)])
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    right, up = math.cos(roll) * right + math.sin(roll) * up, -math.sin(roll) * right + math.cos(roll) * up
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, fwd, eye
    return torch.from_numpy(m).float()


def intrinsics(fov_degrees, skew=0.0):
    f = 1.0 / (2.0 * math.tan(math.radians(fov_degrees) / 2.0))
    return torch.tensor([[f, skew, 0.5], [0.0, f, 0.5], [0.0, 0.0, 1.0]])


def hand_placed_rays():
    """16 rays: 8 from a camera through the box (two graze the crop limit), 4 that cross only part of the cropped region, and 4
    that never enter |x| <= lim and |z| <= lim (every sample cropped: zero weight)"""
    eye = torch.tensor([0.0, 0.0, RADIUS])
    targets = torch.tensor([[0.0, 0.0, 0.0], [0.2, 0.1, 0.0], [-0.3, 0.2, 0.1], [0.1, -0.35, -0.1], [0.39, 0.0, 0.0], [-0.41, 0.1, 0.0],
                            [0.05, 0.45, 0.2], [-0.15, -0.2, -0.3]])
    o = [eye] * 8
    d = [t - eye for t in targets]
    o += [torch.tensor([0.5, 0.0, RADIUS]), torch.tensor([-0.6, 0.2, RADIUS]), torch.tensor([-RADIUS, 0.1, 0.3]),
          torch.tensor([0.3, RADIUS, 0.2])]
    d += [torch.tensor([-0.1, 0.0, -1.0]), torch.tensor([0.15, 0.0, -1.0]), torch.tensor([1.0, 0.0, 0.05]),
          torch.tensor([0.0, -1.0, 0.0])]
    o += [torch.tensor([1.5, 0.0, RADIUS]), torch.tensor([-1.2, 0.3, RADIUS]), torch.tensor([-RADIUS, 0.0, 2.0]),
          torch.tensor([0.0, 0.2, RADIUS + 1.5])]                                # the misses
    d += [torch.tensor([0.0, 0.0, -1.0]), torch.tensor([0.0, 0.1, -1.0]), torch.tensor([1.0, 0.0, 0.0]), torch.tensor([0.0, 0.0, -1.0])]
    return torch.stack(o), torch.nn.functional.normalize(torch.stack(d), dim=1)


class Recorder:
    """wraps the two rand draws and three methods of one renderer while it runs"""

    def __init__(self, renderer):
        self.renderer, self.draws, self.fields, self.depths_coarse, self.depths_fine = renderer, [], [], None, None

    def __enter__(self):
        self.rand, self.rand_like = torch.rand, torch.rand_like
        r = self.renderer
        self.methods = (r.sample_stratified, r.sample_importance, r.run_model)

        def rand(*a, **k):
            v = self.rand(*a, **k)
            self.draws.append(v.clone())
            return v

        def rand_like(*a, **k):
            v = self.rand_like(*a, **k)
            self.draws.append(v.clone())
            return v

        def stratified(*a, **k):
            self.depths_coarse = self.methods[0](*a, **k)
            return self.depths_coarse

        def importance(*a, **k):
            self.depths_fine = self.methods[1](*a, **k)
            return self.depths_fine

        def run_model(*a, **k):
            out = self.methods[2](*a, **k)
            self.fields.append(out)          # the renderer writes the crop into out['sigma'] afterwards, in place
            return out

        torch.rand, torch.rand_like = rand, rand_like
        r.sample_stratified, r.sample_importance, r.run_model = stratified, importance, run_model
        return self

    def __exit__(self, *exc):
        torch.rand, torch.rand_like = self.rand, self.rand_like
        r = self.renderer
        r.sample_stratified, r.sample_importance, r.run_model = self.methods


def main():
    g = torch.Generator().manual_seed(31)
    torch.manual_seed(31)
    out = {}
    raw = dict(w1=fp16_valued(64, 32, g=g), w2=fp16_valued(33, 64, g=g))
    planes = {D: fp16_valued(3, 32 * max(D, 1), H, W, g=g) for D in (0, 1, 3)}
    out.update(w1_raw=raw["w1"].numpy().astype(np.float16), w2_raw=raw["w2"].numpy().astype(np.float16))
    for D, p in planes.items():
        out[f"planes_d{D}"] = p.numpy().astype(np.float16)
    names = []
    for ci, (name, teacher, D, act, lr_mul, box_warp, crop, white_back, Nc, Ni, res) in enumerate(CASES):
        use_teacher(teacher)
        from training.triplane import OSGDecoder
        from training.volumetric_rendering.ray_sampler import RaySampler
        from training.volumetric_rendering.renderer import ImportanceRenderer
        dec = OSGDecoder(32, {"decoder_lr_mul": lr_mul, "decoder_output_dim": 32, "decoder_activation": act})
        b1, b2 = 0.5 * torch.randn(64, generator=g), 0.5 * torch.randn(33, generator=g)
        with torch.no_grad():
            dec.net[0].weight.copy_(raw["w1"]); dec.net[0].bias.copy_(b1)
            dec.net[2].weight.copy_(raw["w2"]); dec.net[2].bias.copy_(b2)
        if res:
            cam = look_at_origin(0.4 + 0.9 * ci, 0.15 * (ci - 1), 0.1 * ci)
            with torch.no_grad():
                origins, dirs = RaySampler()(cam[None], intrinsics(12.0 + 2.0 * ci if ci < 3 else 18.0)[None], res)
        else:
            origins, dirs = (t[None] for t in hand_placed_rays())
        opts = {"box_warp": box_warp, "ray_start": RAY_START, "ray_end": RAY_END, "depth_resolution": Nc,
                "depth_resolution_importance": Ni, "disparity_space_sampling": False, "clamp_mode": "softplus",
                "white_back": white_back}
        R = ImportanceRenderer()
        with torch.no_grad(), Recorder(R) as rec:
            if teacher == "PanoHead":
                opts["triplane_depth"] = D
                features, depth, weights = R(planes[D][None], dec, origins, dirs, opts, triplane_crop=crop)
            else:
                assert not hasattr(dec, "activation") and crop is None
                features, depth, weights = R(planes[D][None], dec, origins, dirs, opts)
        M = origins.shape[1]
        assert len(rec.draws) == (2 if Ni else 1) and len(rec.fields) == (2 if Ni else 1)
        u_coarse = rec.draws[0].reshape(M, Nc)
        u_fine = rec.draws[1].reshape(M, Ni) if Ni else torch.zeros(M, 0)
        depths_fine = rec.depths_fine.reshape(M, Ni) if Ni else torch.zeros(M, 0)
        sigma = torch.cat([f["sigma"].reshape(M, -1) for f in rec.fields], 1)          # [M, Nc + Ni]: coarse, then fine
        rgb = torch.cat([f["rgb"].reshape(M, -1, 32) for f in rec.fields], 1)
        if crop is not None and Ni:
            lim = np.float32(box_warp / 2 - crop)
            xyz = origins[0][:, None, :] + depths_fine[:, :, None] * dirs[0][:, None, :]
            gap = (xyz[..., [0, 2]].abs() - float(lim)).abs().min()
            assert float(gap) >= NEAR, f"{name}: a fine sample lies {float(gap):.2e} from the crop limit: change the seed"
        zero = int((weights[0, :, 0] == 0).sum())
        if not res:
            assert zero >= 4 and bool((depth[0, :, 0][weights[0, :, 0] == 0] == rec_max(rec, Ni)).all())
            assert bool((features[0][weights[0, :, 0] == 0] == 0).all())
        names.append(name)
        out.update({f"{name}.b1_raw": b1.numpy(), f"{name}.b2_raw": b2.numpy(), f"{name}.origins": origins[0].numpy(),
                    f"{name}.dirs": dirs[0].numpy(), f"{name}.u_coarse": u_coarse.numpy(), f"{name}.u_fine": u_fine.numpy(),
                    f"{name}.depths_coarse": rec.depths_coarse.reshape(M, Nc).numpy(), f"{name}.depths_fine": depths_fine.numpy(),
                    f"{name}.sigma": sigma.numpy(), f"{name}.rgb": rgb.numpy(), f"{name}.features": features[0].numpy(),
                    f"{name}.depth": depth[0, :, 0].numpy(), f"{name}.weights": weights[0, :, 0].numpy(),
                    f"{name}.gains": np.asarray([dec.net[0].weight_gain, dec.net[0].bias_gain, dec.net[2].weight_gain,
                                                 dec.net[2].bias_gain], np.float64),
                    f"{name}.meta": np.asarray([D, lr_mul, box_warp, -1.0 if crop is None else crop, float(white_back), Nc, Ni, res],
                                               np.float64),
                    f"{name}.activation": np.asarray(act), f"{name}.teacher": np.asarray(teacher)})
        print(name, "rays", M, "weights", float(weights.min()), float(weights.max()), "zero-weight rays", zero, "depth",
              float(depth.min()), float(depth.max()))
    out["cases"] = np.asarray(names)
    # RaySampler alone: two batched cameras, non-zero skew
    cams = torch.stack([look_at_origin(0.7, 0.2, 0.3), look_at_origin(-2.1, -0.4, -0.2)])
    intr = torch.stack([intrinsics(14.0, 0.07), intrinsics(17.0, -0.11)])
    with torch.no_grad():
        o, d = RaySampler()(cams, intr, 5)
    out.update(rays_cam2world=cams.numpy(), rays_intrinsics=intr.numpy(), rays_origins=o.numpy(), rays_dirs=d.numpy())
    # fp32 rgb rows do not compress: the per-sample rgb of the cases with more than RGB_SPLIT samples goes to a second file, so
    # that each stays well inside the size limit of a committed file
    big = {k: out.pop(k) for k in [k for k in out if k.endswith(".rgb") and out[k].shape[0] * out[k].shape[1] > RGB_SPLIT]}
    for fname, arrays in (("teacher_render_fixture.npz", out), ("teacher_render_fixture_rgb.npz", big)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrays)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 800 * 1024


def rec_max(rec, Ni):
    both = [rec.depths_coarse.reshape(-1)] + ([rec.depths_fine.reshape(-1)] if Ni else [])
    return torch.cat(both).max()


if __name__ == "__main__":
    main()
