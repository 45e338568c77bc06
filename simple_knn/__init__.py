"""Drop-in shim: makes the reference's import line
    from simple_knn._C import distCUDA2
(gaussian_splatting/scene/gaussian_model.py:20) resolve to the gfx950 3-nearest-neighbour kernel when this repository
root is on sys.path.  See INTEGRATION.md."""
from gaussian_gan_decoder_amd.knn import dist_cuda2 as distCUDA2  # noqa: F401
