#!/usr/bin/env python3
"""Diagnostic: one ``sample_3d_crop`` call at the downstream recipe's shape: 4 frames of
192 x 640 depth, 5 crops per frame, 576 samples per crop kept out of 2304 drawn, on the C1 field
(192 x 640 x 256 grid, ResnetFC 128, 64 DINO codes, bf16) with an MlpDimReduction to 768.

  native:  sd_crop3d_centres -> net.query -> sd_crop3d_compact -> expand_dim, one host read;
  torch:   the same function with crop3d._NATIVE = False: the torch-op route of the same
           arithmetic on the same device (sort, cumsum, searchsorted, gather), the same
           net.query and expand_dim kernels, the same one host read.
Milliseconds per call, host clock around ITERS back-to-back calls that each end in their host
read, after warm-up; RUNS runs of each variant, alternated (native, torch, native, ...); every
run is reported, with the median and the spread (max - min) per variant.  Both variants draw on
the device RNG.  This is eager call time on a shared host, not kernel time.  The parts of the
native call are also timed alone (HIP events around ITERS calls).  Writes
profiles/crop3d/bench.json and prints it as one JSON line."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scenedino_amd import _lib  # noqa: E402
from scenedino_amd.training import crop3d  # noqa: E402

dev = "cuda"
ITERS, RUNS, WARM = 5, 6, 3
N_, H_, W_, C_GRID = 4, 192, 640, 256
N_CROPS, N_SAMPLES, OVERSAMPLING = 5, 576, 4
KITTI_K = [[0.7849, 0.0, -0.0312], [0.0, 2.9391, 0.2701], [0.0, 0.0, 1.0]]


class FixedGridEncoder(torch.nn.Module):
    def __init__(self, grid):
        super().__init__()
        self.register_buffer("grid", grid)
        self.latent_size = grid.shape[1]
        self.extra_outs = 0

    def forward(self, x, ground_truth=False):
        return [self.grid]


def make_net():
    from scenedino_amd.common.positional_encoding import PositionalEncoding
    from scenedino_amd.models import BTSNet
    from scenedino_amd.models.backbones.dino import MlpDimReduction
    from scenedino_amd.models.prediction_heads import ResnetFC
    g = torch.Generator().manual_seed(0)
    images = (torch.rand(N_, 1, 3, H_, W_, generator=g) * 2 - 1).to(dev)
    grid = torch.randn(N_, C_GRID, H_, W_, generator=g).contiguous(memory_format=torch.channels_last)
    torch.manual_seed(2)
    head = ResnetFC(d_in=C_GRID + 39, d_out=65, n_blocks=0, d_hidden=128)
    with torch.no_grad():
        head.lin_out.bias[0] = 0.5  # sigma = softplus(.) around the 0.5 threshold
    conf = {"predict_dino": True, "dino_dims": 64, "learn_empty": False, "code_mode": "z",
            "inv_z": True, "z_near": 3, "z_far": 80, "sample_color": True, "precision": "bf16"}
    enc = FixedGridEncoder(grid)
    enc.dim_reduction = MlpDimReduction(768, 64, 128)
    enc.expand_dim = enc.dim_reduction.transform_expand
    net = BTSNet(conf, enc, PositionalEncoding(6, 3, 1.5, True), {"normal_head": head},
                 final_pred_head="normal_head").to(dev).eval()
    Ks = torch.tensor(KITTI_K, device=dev).view(1, 1, 3, 3).repeat(N_, 1, 1, 1)
    poses = torch.eye(4, device=dev).view(1, 1, 4, 4).repeat(N_, 1, 1, 1)
    net.encode(images, Ks, poses, ids_encoder=[0], ids_render=[0])
    depth = 3.0 + 77.0 * torch.rand(N_, 1, H_, W_, generator=g)
    depth[:, :, :40] = torch.where(torch.rand(N_, 1, 40, W_, generator=g) < 0.5,
                                   torch.full_like(depth[:, :, :40], 80.0), depth[:, :, :40])
    return net, poses, Ks, depth.to(dev)


def wall(fn, iters=ITERS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def events(fn, iters=ITERS):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / iters


def main():
    if not torch.cuda.is_available():
        raise SystemExit("crop3d_bench: needs a ROCm device")
    _lib.load()
    net, poses, Ks, depth = make_net()
    kept = []

    def call(native):
        crop3d._NATIVE = native
        try:
            dino, _ = crop3d.sample_3d_crop(net, poses, Ks, depth, z_far=100, n_crops=N_CROPS,
                                            n_samples=N_SAMPLES, oversampling=OVERSAMPLING)
        finally:
            crop3d._NATIVE = True
        kept.append(0 if dino is None else dino.shape[1])

    variants = (("native", lambda: call(True)), ("torch", lambda: call(False)))
    for _, fn in variants:
        for _ in range(WARM):
            fn()
    times = {name: [] for name, _ in variants}
    for _ in range(RUNS):
        for name, fn in variants:
            times[name].append(wall(fn))
    out = {"iters": ITERS, "runs": RUNS, "frames": N_, "map": [H_, W_], "n_crops": N_CROPS,
           "n_samples": N_SAMPLES, "oversampling": OVERSAMPLING,
           "kept_crops_mean": round(sum(kept) / len(kept), 2), "call_ms": {}}
    for name, ts in times.items():
        out["call_ms"][name] = {"runs": [round(t, 3) for t in ts],
                                "median": round(statistics.median(ts), 3),
                                "spread": round(max(ts) - min(ts), 3)}
    n, t = out["call_ms"]["native"], out["call_ms"]["torch"]
    out["native_faster_beyond_spreads"] = bool(n["median"] < t["median"] - (n["spread"] + t["spread"]))

    # the parts of the native call alone
    S = OVERSAMPLING * N_SAMPLES
    pick, shift = crop3d._draw(N_, N_CROPS, S, 0.5, dev, None)
    _, count, _, _, points = _lib.crop3d_centres(depth, poses, Ks, 100.0, pick, shift)
    pts = points.view(N_, -1, 3)
    sigma, codes = net.query(pts, colors=False)[:2]
    sigma, codes = sigma.reshape(-1, S).contiguous(), codes.reshape(N_ * N_CROPS, S, -1).contiguous()
    ok = count.reshape(-1)
    rows = _lib.crop3d_compact(sigma, codes, ok, 0.5, N_SAMPLES)[0]
    parts = {"draws": lambda: crop3d._draw(N_, N_CROPS, S, 0.5, dev, None),
             "sd_crop3d_centres": lambda: _lib.crop3d_centres(depth, poses, Ks, 100.0, pick, shift),
             "centres_torch": lambda: crop3d.centres_torch(depth, poses, Ks, 100.0, pick, shift),
             "net_query": lambda: net.query(pts, colors=False),
             "sd_crop3d_compact": lambda: _lib.crop3d_compact(sigma, codes, ok, 0.5, N_SAMPLES),
             "compact_torch": lambda: crop3d.compact_torch(sigma, codes, ok, 0.5, N_SAMPLES),
             "expand_dim": lambda: net.encoder.expand_dim(rows)}
    out["part_ms"] = {}
    with torch.no_grad():
        for name, fn in parts.items():
            fn()
            torch.cuda.synchronize()
            ts = [events(fn, 20) for _ in range(3)]
            out["part_ms"][name] = {"runs": [round(x, 4) for x in ts],
                                    "median": round(statistics.median(ts), 4)}
    path = os.path.join(ROOT, "profiles", "crop3d")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
