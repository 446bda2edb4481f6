"""Drop-in for the `diff_surfel_rasterization` extension (2D Gaussian splatting;
reference import: gaussian_splatting/gaussian_renderer/__init__.py:89)."""
from pings_amd.rasterizer import Surfel2DGaussianRasterizer as GaussianRasterizer
from pings_amd.rasterizer import Surfel2DRasterizationSettings as GaussianRasterizationSettings

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer"]
