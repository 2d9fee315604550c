"""Writes tests/golden/recon_loss.npz: the reference's ReconstructionLoss
(scenedino/losses/reconstruction_loss.py) in float64 on the CPU, per case of
tests/_recon_inputs.py CASES.

    SCENEDINO_REF=<reference checkout> python tests/golden/make_golden_recon.py

The reference is imported as tests/golden/make_golden_stego.py imports it (make_golden.py's
stubs, a bare ``scenedino.losses`` package module) plus an empty ``kornia`` module, which the
reference's loss imports and never uses.  Inputs come from tests/_recon_inputs.py's seeded
generators, which the tests call too, so the file holds results only.  Per case: the metric
names in order, every metric, and per leaf (rgb, depth, dino_features,
dino_features_downsampled of every part) the float64 gradient's L2 norm and its dot with
_recon_inputs.projection (which pin the whole tensor) and a strided subset of at most 512
elements as float32.  For the three shipped shapes also the smallest top-2 view margin and the
smallest distance of a policy sum from 0.9, measured on the reference's own tensors.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402
import _recon_inputs as ri  # noqa: E402


def main():
    mg._install_stubs()
    sys.modules["kornia"] = types.ModuleType("kornia")
    losses = types.ModuleType("scenedino.losses")
    losses.__path__ = [os.path.join(mg.REF, "scenedino", "losses")]
    sys.modules["scenedino.losses"] = losses
    from scenedino.losses.reconstruction_loss import ReconstructionLoss, compute_l1ssim
    out = {}
    for name in ri.CASES:
        cfg, raw = ri.case(name)
        data = ri.convert(raw)
        loss = ReconstructionLoss(cfg)
        res = loss(data)
        names = loss.get_loss_metric_names()
        assert list(res) == names
        out[name + "/names"] = np.array(names)
        for k, v in res.items():
            out[f"{name}/metric/{k}"] = np.float64(v.item())
        res["rec_loss"].backward()
        lv = ri.leaves(data) + (ri.leaves(data, "fine") if "fine" in data else [])
        for lname, t in lv:
            if t.grad is None:
                continue
            g = t.grad.detach().double().reshape(-1)
            out[f"{name}/norm/{lname}"] = np.float64(g.norm().item())
            out[f"{name}/dot/{lname}"] = np.float64((g * ri.projection(g)).sum().item())
            out[f"{name}/sub/{lname}"] = ri.subset(g).float().numpy().copy()
        if name.startswith("shipped_"):
            c0 = data["coarse"][0]
            rgb = c0["rgb"].detach()
            b, pc, h, w, nv, ch = rgb.shape
            gt = data["rgb_gt"].unsqueeze(-2).expand(rgb.shape)
            e = compute_l1ssim(rgb.permute(0, 1, 4, 5, 2, 3).reshape(-1, ch, h, w),
                               gt.permute(0, 1, 4, 5, 2, 3).reshape(-1, ch, h, w))
            top = e.view(b, pc, nv, h, w).topk(2, dim=2, largest=False).values
            out[name + "/view_margin"] = np.float64((top[:, :, 1] - top[:, :, 0]).min().item())
            s = (c0["invalid"] * c0["weights"].unsqueeze(-1)).sum(-2)
            out[name + "/policy_margin"] = np.float64((s - 0.9).abs().min().item())
            out[name + "/masked"] = np.float64((s > 0.9).all(-1).double().mean().item())
    path = os.path.join(HERE, "recon_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    for name in ri.CASES:
        if name.startswith("shipped_"):
            print(name, "view margin", out[name + "/view_margin"], "policy margin",
                  out[name + "/policy_margin"], "masked", out[name + "/masked"])


if __name__ == "__main__":
    main()
