"""`simple_knn._C` of the reference is a compiled extension with one function; here it is this module."""
from gaussian_gan_decoder_amd.knn import dist_cuda2 as distCUDA2  # noqa: F401
