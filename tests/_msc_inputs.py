"""Seeded inputs shared by tests/golden/make_golden_msc.py and the multi-scale-crop target
tests (tests/test_msc_gt.py, tests/test_msc_gt_gpu.py): the fixture holds results only."""
import torch
from torch import nn

GOLDEN = dict(B=2, V=4, C=8, hp=3, wp=5, H=24, W=40)
# [x0, y0, w, h] per image and augmented view, and the flips
GOLDEN_BOXES = [[[4, 3, 28, 16], [10, 6, 24, 14]], [[0, 0, 40, 24], [7, 2, 30, 20]]]
GOLDEN_FLIPS = [[False, True], [True, False]]


class FixedGrids(nn.Module):
    """A gt encoder that returns fixed final token grids whatever the images are."""

    def __init__(self, grids):
        super().__init__()
        self.grids = grids
        self.calls = []

    def forward(self, x):
        self.calls.append(tuple(x.shape))
        return [self.grids[: x.shape[0]]]


def golden_inputs():
    g = torch.Generator().manual_seed(2024)
    c = GOLDEN
    grids = torch.randn(c["B"] * c["V"], c["C"], c["hp"], c["wp"], generator=g, dtype=torch.float64)
    images = torch.rand(c["B"], 3, c["H"], c["W"], generator=g, dtype=torch.float64) * 2 - 1
    # _accumulate_predictions on its own: already-upsampled features of 3 channels
    acc = torch.randn(c["B"], c["V"], 3, c["H"], c["W"], generator=g, dtype=torch.float64)
    return dict(grids=grids, images=images, acc=acc,
                boxes=torch.tensor(GOLDEN_BOXES), flips=torch.tensor(GOLDEN_FLIPS))
