"""Writes tests/golden/msc_gt.npz: the reference's MultiScaleCropGT_kornia and InterpolatedGT
(scenedino/models/backbones/dino/upsampler.py) in float64 on the CPU, on the inputs of
tests/_msc_inputs.py.

    SCENEDINO_REF=<reference checkout> python tests/golden/make_golden_msc.py

The reference module is imported with make_golden.py's stubs plus stub ``kornia`` /
``torchvision`` modules, the way make_golden_recon.py stubs kornia.  The stub's
``kornia.geometry.warp_perspective`` is this package's restatement
(scenedino_amd/models/backbones/dino/upsampler.py warp_perspective), and torchvision's ``Resize``
is the antialiased ``F.interpolate`` it is on tensors.  ``_get_augmentations`` is replaced on the
instance by the injected views, and the gt encoder is a stub returning fixed grids.  So the
fixture pins the reference's control flow -- view order, flip reversal, mask padding, NaN
handling, channel chunking, normalisation -- and everything else except kornia's warp itself.
Arrays: ``forward_chunk`` (B, C, H, W), ``accumulate`` (_accumulate_predictions on 3-channel
features, (B, 3, H, W)), ``interpolated`` (InterpolatedGT("bilinear"), (B V, C, H, W)).
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
import _msc_inputs as mi  # noqa: E402


def _stub_modules():
    from scenedino_amd.models.backbones.dino import upsampler as up

    class _Aug:
        def __init__(self, *a, **k):
            pass

    kornia = types.ModuleType("kornia")
    kornia.augmentation = types.ModuleType("kornia.augmentation")
    for n in ("RandomHorizontalFlip", "RandomResizedCrop", "VideoSequential"):
        setattr(kornia.augmentation, n, _Aug)
    kornia.geometry = types.ModuleType("kornia.geometry")
    kornia.geometry.warp_perspective = up.warp_perspective
    sys.modules["kornia"] = kornia

    class InterpolationMode:
        NEAREST, BILINEAR, BICUBIC = "nearest", "bilinear", "bicubic"

    class Resize:
        def __init__(self, size, interpolation):
            self.size, self.mode = tuple(size), interpolation

        def __call__(self, x):
            kw = {} if self.mode == "nearest" else {"align_corners": False, "antialias": True}
            return F.interpolate(x, size=self.size, mode=self.mode, **kw)

    tvt = sys.modules["torchvision.transforms"]
    tvt.InterpolationMode, tvt.Resize = InterpolationMode, Resize
    for sub in ("scenedino.models.backbones", "scenedino.models.backbones.dino"):
        m = types.ModuleType(sub)
        m.__path__ = [os.path.join(mg.REF, *sub.split("."))]
        sys.modules[sub] = m
    mono = types.ModuleType("scenedino.models.backbones.monodepth2")
    mono.Decoder = object
    sys.modules["scenedino.models.backbones.monodepth2"] = mono


def main():
    mg._install_stubs()
    _stub_modules()
    from scenedino.models.backbones.dino.upsampler import InterpolatedGT, MultiScaleCropGT_kornia
    from scenedino_amd.models.backbones.dino.upsampler import view_transforms
    c, inp = mi.GOLDEN, mi.golden_inputs()
    H, W = c["H"], c["W"]
    T = view_transforms(inp["boxes"], inp["flips"], (H, W)).double()
    ref = MultiScaleCropGT_kornia(mi.FixedGrids(inp["grids"]), num_views=c["V"], image_size=(H, W))
    views = inp["images"][:, None].repeat(1, c["V"], 1, 1, 1)
    ref._get_augmentations = lambda images: (views, T.clone())
    out = {"forward_chunk": ref.forward_chunk(inp["images"]).numpy(),
           "accumulate": ref._accumulate_predictions(inp["acc"].clone(), T.clone()).numpy(),
           "interpolated": InterpolatedGT("bilinear", mi.FixedGrids(inp["grids"]), (H, W))(
               views.flatten(0, 1))[0].numpy()}
    for k, v in out.items():
        assert v.dtype == np.float64 and np.isfinite(v).all(), k
    path = os.path.join(HERE, "msc_gt.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
