"""Drop-in shim: makes the reference's import line
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
(gaussian_splatting/gaussian_renderer/__init__.py:14) resolve to the gfx950 rasterizer when this repository root is
on sys.path, upstream's `from diff_gaussian_rasterization import SparseGaussianAdam` to the HIP optimizer step, and the
3DGS-MCMC fork's `from diff_gaussian_rasterization import compute_relocation` to the HIP relocation op.
See INTEGRATION.md."""
from gaussian_gan_decoder_amd.rasterizer import (  # noqa: F401
    GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians, _RasterizeGaussians, mark_visible,
    rasterize_gaussians_native, rasterize_gaussians_backward_native)
from gaussian_gan_decoder_amd.sparse_adam import SparseGaussianAdam  # noqa: F401
from gaussian_gan_decoder_amd.mcmc import compute_relocation  # noqa: F401
from gaussian_gan_decoder_amd.contribution import ContributionStats  # noqa: F401
