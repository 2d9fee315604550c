"""Pieces of the reference's trainer wrappers that run on this package's kernels."""
from .crop3d import sample_3d_crop

__all__ = ["sample_3d_crop"]
