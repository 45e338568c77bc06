"""Generate tests/golden/density_fixture.npz: the teacher's density / colour field from the REFERENCE's own code, imported from
/root/reference on the CPU:

  PanoHead/training/volumetric_rendering/renderer.py:198-205   ImportanceRenderer.run_model = sample_from_planes (3-D grid_sample
                                         over the C x D tri-grid, PanoHead plane axes) -> decoder
  PanoHead/training/triplane.py:300-332  OSGDecoder (FullyConnectedLayer 32 -> 64, Softplus, 64 -> 33; decoder_activation)
  eg3d/training/volumetric_rendering/renderer.py:142-148, eg3d/training/triplane.py:116-139   the same with the 2-D sampler, EG3D
                                         plane axes and the sigmoid always
  main/marching_cube/sample.py:5-26      create_samples (the lattice G.sample_mixed is evaluated on)

Run in the build container:  python tests/golden/make_density_golden.py
Only arrays travel.  Planes are 12 x 10 (H x W: a swap of the two shows), drawn as fp16-representable values and stored as fp16;
the raw (pre-gain) weights likewise, one set for every case -- the cases differ in depth, activation, lr multiplier (which
changes the gains, networks_stylegan2.py:111-112), biases and box_warp.  Coordinates are drawn from 1.2 x the box.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
H, W, NPTS = 12, 10, 256

# (name, teacher, depth (0 = 2-D tri-planes), activation, decoder_lr_mul, box_warp)
CASES = [("pano_d1_sigmoid_lr1", "PanoHead", 1, "sigmoid", 1.0, 1.0),
         ("pano_d1_lrelu_lr2", "PanoHead", 1, "lrelu", 2.0, 1.0),
         ("pano_d1_none_lr2", "PanoHead", 1, "none", 2.0, 0.7),
         ("pano_d3_none_lr1", "PanoHead", 3, "none", 1.0, 0.7),
         ("pano_d3_sigmoid_lr2", "PanoHead", 3, "sigmoid", 2.0, 0.7),
         ("pano_d3_lrelu_lr1", "PanoHead", 3, "lrelu", 1.0, 1.0),
         ("eg3d_sigmoid_lr1", "eg3d", 0, "sigmoid", 1.0, 1.0)]
LATTICES = [(5, 1.0), (8, 1.0), (6, 1.6)]


def fp16_valued(*shape, g, scale=1.0):
    return (scale * torch.randn(*shape, generator=g)).half().float()


def use_teacher(name):
    """put one teacher's `training` / `torch_utils` / `dnnlib` packages first (both trees use the same package names)"""
    for m in [m for m in sys.modules if m.split(".")[0] in ("training", "torch_utils", "dnnlib")]:
        del sys.modules[m]
    sys.path[:] = [p for p in sys.path if not p.startswith(REF)]
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, name))


def main():
    g = torch.Generator().manual_seed(20)
    out = {}
    raw = dict(w1=fp16_valued(64, 32, g=g), w2=fp16_valued(33, 64, g=g))
    planes = {D: fp16_valued(3, 32 * max(D, 1), H, W, g=g) for D in (0, 1, 3)}
    out.update(w1_raw=raw["w1"].numpy().astype(np.float16), w2_raw=raw["w2"].numpy().astype(np.float16))
    for D, p in planes.items():
        out[f"planes_d{D}"] = p.numpy().astype(np.float16)
    names = []
    for name, teacher, D, act, lr_mul, box_warp in CASES:
        use_teacher(teacher)
        from training.triplane import OSGDecoder
        from training.volumetric_rendering.renderer import ImportanceRenderer
        dec = OSGDecoder(32, {"decoder_lr_mul": lr_mul, "decoder_output_dim": 32, "decoder_activation": act})
        b1, b2 = 0.5 * torch.randn(64, generator=g), 0.5 * torch.randn(33, generator=g)
        with torch.no_grad():
            dec.net[0].weight.copy_(raw["w1"]); dec.net[0].bias.copy_(b1)
            dec.net[2].weight.copy_(raw["w2"]); dec.net[2].bias.copy_(b2)
        coords = (torch.rand(1, NPTS, 3, generator=g) - 0.5) * 1.2 * box_warp
        opts = {"box_warp": box_warp}
        if teacher == "PanoHead":
            opts["triplane_depth"] = D
        R = ImportanceRenderer()
        with torch.no_grad():
            res = R.run_model(planes[D][None], dec, coords, torch.zeros_like(coords), opts)
        if teacher == "eg3d":
            assert not hasattr(dec, "activation")
        names.append(name)
        out.update({f"{name}.b1_raw": b1.numpy(), f"{name}.b2_raw": b2.numpy(), f"{name}.coords": coords[0].numpy(),
                    f"{name}.sigma": res["sigma"][0, :, 0].numpy(), f"{name}.rgb": res["rgb"][0].numpy(),
                    f"{name}.plane_axes": R.plane_axes.numpy(),
                    f"{name}.gains": np.asarray([dec.net[0].weight_gain, dec.net[0].bias_gain, dec.net[2].weight_gain,
                                                 dec.net[2].bias_gain], np.float64),
                    f"{name}.meta": np.asarray([D, lr_mul, box_warp], np.float64), f"{name}.activation": np.asarray(act),
                    f"{name}.teacher": np.asarray(teacher)})
        print(name, "sigma", float(res["sigma"].min()), float(res["sigma"].max()), "rgb", float(res["rgb"].min()),
              float(res["rgb"].max()))
    out["cases"] = np.asarray(names)
    from main.marching_cube.sample import create_samples
    for n, cube in LATTICES:
        s, num = create_samples(samples_per_axis=n, voxel_origin=[0, 0, 0], cube_length=cube)
        assert num == n ** 3
        out[f"lattice_{n}_{cube}"] = s[0].numpy()
    out["lattices"] = np.asarray(LATTICES, np.float64)
    path = os.path.join(HERE, "density_fixture.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
