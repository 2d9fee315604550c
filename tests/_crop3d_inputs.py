"""Seeded inputs of the 3-D crop sampler's fixture (tests/golden/make_golden_crop3d.py writes
crop3d.npz from them, tests/test_crop3d.py reads it back) and the analytic stand-in net the
generator and the tests share: sigma and 64-d codes as closed-form functions of xyz,
``expand_dim`` the identity."""
from __future__ import annotations

import math

import numpy as np
import torch

Z_FAR = 100.0
N_CROPS = 5
N_SAMPLES = 16
OVERSAMPLING = 4
S = OVERSAMPLING * N_SAMPLES
RADIUS = 0.5
THR = 0.5
# no sample's sigma this close to THR: 2e-5 m of position moves sigma by 2e-5 * 0.45 * 5.2 < 5e-5
SIGMA_MARGIN = 1e-4

# name -> (n, h, w, share of the map on the far plateau, edge case)
CASES = {
    "full": (1, 8, 16, 0.0, False),
    "plateau": (1, 37, 83, 0.3, False),
    "batch2": (2, 8, 16, 0.0, False),
    "edge": (1, 8, 16, 0.0, True),
}
KITTI_K = [[0.7849, 0.0, -0.0312], [0.0, 2.9391, 0.2701], [0.0, 0.0, 1.0]]


class _Encoder:
    @staticmethod
    def expand_dim(x):
        return x


class StandInNet(torch.nn.Module):
    """sigma (n, P, 1) = 0.5 + 0.45 sin(3.9 x + 2.1 y - 2.7 z) and codes (n, P, 64) with
    codes[k] = cos(a_k x + b_k y + c_k z + k), evaluated in f64 on the f32 points and rounded
    once.  Called as the reference calls its net: a 5-tuple with sigma third and the codes under
    ``dino_features`` in the fifth."""

    D = 64

    def __init__(self):
        super().__init__()
        self.encoder = _Encoder()

    @classmethod
    def field(cls, xyz):
        p = xyz.double()
        x, y, z = p[..., 0], p[..., 1], p[..., 2]
        sigma = 0.5 + 0.45 * torch.sin(3.9 * x + 2.1 * y - 2.7 * z)
        k = torch.arange(cls.D, dtype=torch.float64, device=xyz.device)
        phase = (x[..., None] * (0.11 * (k + 1)) + y[..., None] * (0.07 * (k + 3))
                 + z[..., None] * (0.05 * (k + 2)) + k)
        return sigma.float(), torch.cos(phase).float()

    def forward(self, xyz, **kwargs):
        sigma, codes = self.field(xyz)
        return None, None, sigma.unsqueeze(-1), None, {"dino_features": codes}


def shift_of(unit, rad, radius=RADIUS):
    """The reference's ball offsets from its randn / rand draws (trainer_downstream.py:259-266)."""
    unit = unit / torch.norm(unit, dim=-1, keepdim=True)
    return unit * (radius * rad ** (1 / 3))


def make_case(name, seed):
    """The seeded inputs of case ``name``: poses (n, 2, 4, 4), projs (n, 2, 3, 3), depth
    (n, 2, h, w) (view 0 is the one read; view 1 is different data), pick (n, N_CROPS), unit
    (n, N_CROPS, S, 3) and rad (n, N_CROPS, S, 1) (the raw randn / rand draws)."""
    n, h, w, plateau, _ = CASES[name]
    g = torch.Generator().manual_seed(seed)
    depth = 3.0 + 77.0 * torch.rand(n, 2, h, w, generator=g)
    depth = depth.clamp_max(79.99)
    if plateau:
        k = int(round(plateau * h * w))
        for f in range(n):
            idx = torch.randperm(h * w, generator=g)[:k]
            depth[f, 0].view(-1)[idx] = 80.0
    poses = torch.eye(4).repeat(n, 2, 1, 1)
    for f in range(n):
        for v in range(2):
            ang = 0.3 * (torch.rand(3, generator=g) - 0.5)
            cx, cy, cz = (math.cos(float(t)) for t in ang)
            sx, sy, sz = (math.sin(float(t)) for t in ang)
            rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
            ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
            poses[f, v, :3, :3] = rz @ ry @ rx
            poses[f, v, :3, 3] = 2.0 * (torch.rand(3, generator=g) - 0.5)
    projs = torch.tensor(KITTI_K).repeat(n, 2, 1, 1)
    projs[:, :, :2] *= 1.0 + 0.05 * (torch.rand(n, 2, 2, 1, generator=g) - 0.5)
    pick = torch.rand(n, N_CROPS, generator=g)
    unit = torch.randn(n, N_CROPS, S, 3, generator=g)
    rad = torch.rand(n, N_CROPS, S, 1, generator=g)
    return {"poses": poses, "projs": projs, "depth": depth, "pick": pick, "unit": unit, "rad": rad}


def shape_edge_case(case, centre, seed):
    """Redraw single samples of crops 0 and 1 of frame 0 until crop 0 has exactly N_SAMPLES
    occupied samples (dropped: the test is strict) and crop 1 exactly N_SAMPLES + 1 (kept).
    centre (n, N_CROPS, 3): the crop centres of these inputs.  None when it cannot be done."""
    g = torch.Generator().manual_seed(seed + 1000)
    for crop, n_occ in ((0, N_SAMPLES), (1, N_SAMPLES + 1)):
        want = torch.zeros(S, dtype=torch.bool)
        want[torch.randperm(S, generator=g)[:n_occ]] = True
        for s in range(S):
            for _ in range(1000):
                sh = shift_of(case["unit"][0, crop, s], case["rad"][0, crop, s])
                sg = StandInNet.field(centre[0, crop] + sh)[0]
                if bool(sg > THR) == bool(want[s]) and abs(float(sg) - THR) > 1e-2:
                    break
                case["unit"][0, crop, s] = torch.randn(3, generator=g)
                case["rad"][0, crop, s] = torch.rand(1, generator=g)
            else:
                return None  # a ball wholly on one side of the threshold: another seed
    return case


def limits_are_robust(depth0, limits, z_far=Z_FAR):
    """True when moving any interpolated limit by one ulp either way changes no pixel's bin.
    A limit interpolated between the order statistics a < b at floor / ceil of its rank has no
    other depth in [a, b], so the condition is a < prev(limit) and next(limit) < b.  A limit
    whose two order statistics are equal (the minimum, the maximum, a plateau) must be that
    value exactly and is not moved."""
    depth0 = np.asarray(depth0, dtype=np.float32)
    limits = np.asarray(limits, dtype=np.float32)
    n_crops = limits.shape[1] - 1
    for f in range(depth0.shape[0]):
        sel = np.sort(depth0[f][depth0[f] < z_far].ravel())
        for i, L in enumerate(limits[f]):
            rank = np.float32(i / n_crops) * np.float32(len(sel) - 1)
            a, b = sel[int(np.floor(rank))], sel[int(np.ceil(rank))]
            if a == b:
                if L != a:
                    return False
                continue
            lo, hi = np.nextafter(L, np.float32(-np.inf)), np.nextafter(L, np.float32(np.inf))
            if not (a < lo and hi < b):
                return False
    return True
