"""Golden vectors of the supersampled SSCBench query (tests/golden/ssc_pool.npz,
tests/golden/voxel_points_fine.json), from the reference's own ``downsample_and_predict``
(sscbench/evaluate_model_sscbench.py:660-758) run on the CPU.

Run ONLY where the read-only reference is available (see make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ssc_pool.py

The evaluator module cannot be imported here (hydra, matplotlib, ...), so its
``downsample_and_predict`` and ``predict_grid`` definitions are executed with
make_golden.py's ``_ref_functions``; nothing of the reference is copied, the fixtures are
arrays.  The function's ``torch.cuda.synchronize()`` / ``empty_cache()`` calls (timing only)
meet a ``torch`` whose ``cuda`` namespace does nothing; ``device`` is the CPU.

The stub ``net``: ``forward(points)`` decodes the fine voxel index from the points (the
"points" handed to the reference are the int16 index triples of the fine grid -- the function
only slices and reshapes them) and returns a closed-form, integer-hashed sigma >= 0 and one-hot
segs, non-zero only under the coarse corner block [:8, :8, :]:

  * a quarter of the children of every coarse voxel (which quarter depends on the voxel) carry
    the voxel's "heavy" class with sigma in [2, 4);
  * the others carry one of two distractor classes with sigma = 0 (40 % of them: 30 % of all
    fine voxels) or sigma in [0.05, 0.5).

So the alpha-weighted winner is a class that loses the head count, and the winner's mean score
leads by more than 5e-3 for any exp() within a few ulp: the generator asserts a top-two margin
above 1e-3 for every recorded coarse voxel (for the per-point ``vis`` labels: alpha is exactly 0,
from sigma == 0, or above 1e-3), so the recorded labels do not depend on one machine's exp.

Recorded for factor 2 and 4, and for vis=True at factor 2 (same inputs as factor 2):
  f{2,4}_sigma_in / f{2,4}_label_in   the stub's values on the fine corner (8 f, 8 f, 32 f)
  f{2,4}_sigmas   sigmas[:9, :9, :]   (one plane more than the corner: the grow spreads by one)
  f{2,4}_segs     segs[:8, :8, :]
  vis2_sigmas     sigmas[:17, :17, :],  vis2_segs  segs[:16, :16, :]
  *_rest          the sum of every output element outside those blocks (all zero)

voxel_points_fine.json: generate_point_grid's centres at voxel_size 0.1 (SHA-256 of all
512 x 512 x 64 float32 triples) and a strided slice at 0.05, by the numpy restatement of
make_golden.py::fx_voxel_points.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _ref_functions  # noqa: E402

N_CLASSES = 19
CORNER = 8


class _Torch:
    """``torch`` with a do-nothing ``cuda`` namespace."""
    cuda = types.SimpleNamespace(synchronize=lambda: None, empty_cache=lambda: None)

    def __getattr__(self, name):
        return getattr(torch, name)


def _mix(n):
    """A 32-bit integer hash of int64 ``n`` (exact integer arithmetic: the same everywhere)."""
    n = (n * 2654435761 + 40503) % (1 << 32)
    n = (n ^ (n >> 15)) * 2246822519 % (1 << 32)
    n = (n ^ (n >> 13)) * 3266489917 % (1 << 32)
    return n ^ (n >> 16)


def stub_values(ix, iy, iz, f):
    """sigma (f32) and label (int64) of the fine voxels (ix, iy, iz) (int64 tensors)."""
    I, J, K = ix // f, iy // f, iz // f
    inside = (I < CORNER) & (J < CORNER)
    coarse = (I * 256 + J) * 32 + K
    hc = _mix(coarse)
    heavy_cls = hc % N_CLASSES
    child = ((ix % f) * f + (iy % f)) * f + (iz % f)
    heavy = (child + (hc >> 8)) % 4 == 0
    hp = _mix(((ix * (256 * f) + iy) * (32 * f) + iz) + (1 << 31))
    u = (hp & 0xFF).to(torch.float32) / 256.0
    light_cls = (heavy_cls + 1 + ((hp >> 8) % 2) * 6) % N_CLASSES
    light_zero = (hp >> 12) % 10 < 4
    sigma = torch.where(heavy, 2.0 + 2.0 * u,
                        torch.where(light_zero, torch.zeros_like(u), 0.05 + 0.45 * u))
    label = torch.where(heavy, heavy_cls, light_cls)
    zero = torch.zeros_like(sigma)
    return torch.where(inside, sigma, zero), torch.where(inside, label, torch.zeros_like(label)), inside


class StubNet:
    def __init__(self, f):
        self.f = f

    def compute_grid_transforms(self, *a, **k):
        pass

    def encode(self, *a, **k):
        pass

    def set_scale(self, *a, **k):
        pass

    def forward(self, points, predict_segmentation=True, prediction_mode=None):
        p = points.reshape(-1, 3).to(torch.int64)
        sigma, label, inside = stub_values(p[:, 0], p[:, 1], p[:, 2], self.f)
        segs = F.one_hot(label, N_CLASSES).to(torch.float32) * inside.unsqueeze(-1)
        return None, None, sigma.reshape(1, -1, 1), segs.reshape(1, -1, N_CLASSES)


def index_points(f):
    """The (256 f, 256 f, 32 f, 3) int16 fine-grid index triples standing in for the centres."""
    X, Y, Z = 256 * f, 256 * f, 32 * f
    pts = torch.empty(X, Y, Z, 3, dtype=torch.int16)
    pts[..., 0] = torch.arange(X, dtype=torch.int16).view(X, 1, 1)
    pts[..., 1] = torch.arange(Y, dtype=torch.int16).view(1, Y, 1)
    pts[..., 2] = torch.arange(Z, dtype=torch.int16).view(1, 1, Z)
    return pts


def corner_inputs(f):
    n = CORNER * f
    ix, iy, iz = torch.meshgrid(torch.arange(n), torch.arange(n), torch.arange(32 * f), indexing="ij")
    sigma, label, _ = stub_values(ix, iy, iz, f)
    return sigma, label


def check_margins(sigma, label, f):
    """Top-two margin of the mean-scale scores of every coarse voxel of the corner, in f64."""
    alpha = 1 - torch.exp(-(0.2 / f) * sigma.double())
    votes = F.one_hot(label, N_CLASSES).double() * alpha.unsqueeze(-1)
    n = CORNER
    scores = votes.reshape(n, f, n, f, 32, f, N_CLASSES).mean(dim=(1, 3, 5))
    top = scores.topk(2, dim=-1).values
    margin = float((top[..., 0] - top[..., 1]).min())
    assert margin > 1e-3, margin
    counts = F.one_hot(label, N_CLASSES).reshape(n, f, n, f, 32, f, N_CLASSES).sum(dim=(1, 3, 5))
    assert (counts.argmax(-1) != scores.argmax(-1)).float().mean() > 0.9  # weights decide
    return margin


def fx_ssc_pool():
    ev = _ref_functions(os.path.join(REF, "sscbench", "evaluate_model_sscbench.py"),
                        ["downsample_and_predict", "predict_grid"],
                        {"torch": _Torch(), "np": np, "F": F, "time": time, "device": "cpu",
                         "USE_ALPHA_WEIGHTING": True, "USE_GROW": True})
    data = {"imgs": [torch.zeros(3, 4, 4)], "poses": [np.eye(4, dtype=np.float32)],
            "projs": [np.eye(3, dtype=np.float32)]}
    out = {}
    margins = {}
    for f in (2, 4):
        ev["VOXEL_SIZE"] = 0.2 / f  # the evaluator's constant: downsample_factor = int(0.2 // it)
        sigma_in, label_in = corner_inputs(f)
        margins[f] = check_margins(sigma_in, label_in, f)
        out[f"f{f}_sigma_in"] = sigma_in.numpy()
        out[f"f{f}_label_in"] = label_in.numpy().astype(np.uint8)
        pts = index_points(f)
        runs = [("f%d" % f, False, CORNER)] + ([("vis2", True, CORNER * f)] if f == 2 else [])
        for name, vis, n in runs:
            with torch.no_grad():
                sigmas, segs, dino = ev["downsample_and_predict"](data, StubNet(f), pts, f,
                                                                  "stego_kmeans", vis=vis)
            assert dino is None
            if vis:  # per-point labels: alpha exactly 0 (sigma == 0) or clear of 0
                a = 1 - np.exp(-(0.2 / f) * sigma_in.double().numpy())
                assert ((sigma_in.numpy() == 0) | (a > 1e-3)).all()
            sigmas, segs = np.asarray(sigmas), np.asarray(segs)
            out[name + "_sigmas"] = sigmas[:n + 1, :n + 1, :].astype(np.float32)
            out[name + "_segs"] = segs[:n, :n, :].astype(np.uint8)
            assert (segs[:n, :n, :] == out[name + "_segs"]).all()
            out[name + "_sigmas_rest"] = np.float64(sigmas.sum(dtype=np.float64)
                                                    - sigmas[:n + 1, :n + 1, :].sum(dtype=np.float64))
            out[name + "_segs_rest"] = np.float64(segs.sum(dtype=np.float64)
                                                  - segs[:n, :n, :].sum(dtype=np.float64))
            assert out[name + "_sigmas_rest"] == 0 and out[name + "_segs_rest"] == 0
        del pts
    out["margin"] = np.array([margins[2], margins[4]])
    np.savez_compressed(os.path.join(HERE, "ssc_pool.npz"), **out)


def _centres(flat, dims, vox, T, origin):
    """fx_voxel_points' arithmetic for the flat voxel indices ``flat`` of a ``dims`` grid."""
    iz = flat % dims[2]
    iy = (flat // dims[2]) % dims[1]
    ix = flat // (dims[2] * dims[1])
    coords = np.stack([ix, iy, iz], 1).astype(np.float32)
    o32 = origin.astype(np.float32).astype(np.float64)
    cam = ((o32[None] + vox * coords.astype(np.float64)) + vox * 0.5).astype(np.float32)
    xyz_h = np.hstack([cam, np.ones((len(cam), 1), dtype=np.float32)])
    return torch.tensor(np.dot(T, xyz_h.T).T[:, :3]).float().numpy()


def fx_voxel_points_fine():
    cam2velo = np.array([0.04307104361, -0.08829286498, 0.995162929, 0.8043914418,
                         -0.999004371, 0.007784614041, 0.04392796942, 0.2993489574,
                         -0.01162548558, -0.9960641394, -0.08786966659, -0.1770225824]).reshape(3, 4)
    C2V = np.concatenate([cam2velo, np.array([0, 0, 0, 1]).reshape(1, 4)], axis=0)
    T = np.identity(4)
    T[:3, :4] = np.linalg.inv(C2V)[:3, :]
    origin = np.array([0, -25.6, -2])
    rec = {"origin": origin.tolist(), "T": T.tolist()}
    d1 = np.ceil(np.array([51.2, 51.2, 6.4]) / 0.1).astype(int)
    assert d1.tolist() == [512, 512, 64]
    pts = _centres(np.arange(int(np.prod(d1)), dtype=np.int64), d1, 0.1, T, origin)
    rec["0.1"] = {"dims": d1.tolist(), "sha256": hashlib.sha256(pts.tobytes()).hexdigest()}
    d2 = np.ceil(np.array([51.2, 51.2, 6.4]) / 0.05).astype(int)
    assert d2.tolist() == [1024, 1024, 128]
    stride = 65537 * 3 + 2
    sel = np.arange(0, int(np.prod(d2)), stride, dtype=np.int64)
    rec["0.05"] = {"dims": d2.tolist(), "slice_stride": stride,
                   "slice": _centres(sel, d2, 0.05, T, origin).tolist()}
    with open(os.path.join(HERE, "voxel_points_fine.json"), "w") as fh:
        json.dump(rec, fh)


if __name__ == "__main__":
    torch.set_num_threads(8)
    fx_voxel_points_fine()
    fx_ssc_pool()
    print("ssc pool fixtures written to", HERE)
