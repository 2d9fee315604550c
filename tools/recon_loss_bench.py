#!/usr/bin/env python3
"""Diagnostic: forward + backward of the first stage's ReconstructionLoss (the shipped
training/loss/scenedino.yaml options) at the recipe's shapes: n = 4 images, nv = 4 views, K = 32
samples, 16 x 16 patches with pc = 8 and 8 x 8 patches with pc = 32, C = 384 / 768.

  native:   scenedino_amd.losses.ReconstructionLoss on its native route (sd_recon_loss_fwd /
            sd_recon_loss_bwd, one autograd node), eager;
  baseline: the path it replaces -- the same class's torch route on the device, which is the
            reference's op sequence with torch autograd.
Milliseconds per forward + backward with rgb, depth, dino_features and
dino_features_downsampled requiring grad: HIP events around 200 back-to-back steps after
warm-up, three runs of each, alternated (native, baseline, native, ...), every run reported and
the median.  This is eager step time -- it holds the host's launch and allocation cost of every
op, which at these sizes is most of it -- not kernel time.  Device-side launches (kernels and
memory operations) of one forward + backward of each route are counted with torch.profiler.
Writes profiles/recon_loss/bench.json and prints it as one JSON line."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scenedino_amd import _lib  # noqa: E402
from scenedino_amd.losses import make_loss  # noqa: E402

dev = "cuda"
ITERS, RUNS, WARM = 200, 3, 20
CONFIG = {"type": "reconstruction", "coarse": {"criterion": "l1+ssim", "dino_criterion": "cosine"},
          "invalid_policy": "weight_guided", "reconstruct_dino": True, "lambda_dino_coarse": 0.2,
          "temperature_dino": 5,
          "regularizations": [{"type": "edge_aware_smoothness", "lambda": 0.001},
                              {"type": "dino_edge_aware_smoothness", "lambda": 0.25}]}
LEAVES = ("rgb", "depth", "dino_features", "dino_features_downsampled")


def timed(fn):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / ITERS


def launches(fn):
    from torch.autograd import DeviceType
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU,
                                            torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)


def make_data(n, pc, hw, nv, K, C):
    g = torch.Generator().manual_seed(1000 * hw + C)

    def rand(*s):
        return torch.rand(*s, generator=g)

    gt = 0.2 + 0.45 * rand(n, pc, 1, 1, 3) + 0.3 * rand(n, pc, hw, hw, 3)
    amp = 0.1 * torch.arange(1, nv + 1, dtype=torch.float32).view(nv, 1)
    part = {"rgb": gt.unsqueeze(-2) + amp * (2 * rand(n, pc, hw, hw, nv, 3) - 1),
            "weights": torch.softmax(3 * rand(n, pc, hw, hw, K), dim=-1),
            "invalid": (rand(n, pc, hw, hw, K, nv) > 0.03).float(),
            "depth": 3 + 40 * rand(n, pc, hw, hw),
            "dino_features": torch.randn(n, pc, hw, hw, 1, C, generator=g),
            "dino_features_downsampled": torch.randn(n, pc, 1, C, generator=g)}
    part = {k: v.to(dev) for k, v in part.items()}
    for k in LEAVES:
        part[k].requires_grad_(True)
    return {"coarse": [part], "rgb_gt": gt.to(dev),
            "dino_gt": torch.randn(n, pc, C, generator=g).to(dev)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("recon_loss_bench: needs a ROCm device")
    _lib.load()
    out = {"iters": ITERS, "runs": RUNS, "n": 4, "nv": 4, "K": 32, "shapes": []}
    for hw, pc in ((16, 8), (8, 32)):
        for C in (384, 768):
            data = make_data(4, pc, hw, 4, 32, C)
            part = data["coarse"][0]
            loss_n, loss_t = make_loss(CONFIG), make_loss(CONFIG)
            loss_t.native = False

            def step(loss):
                for k in LEAVES:
                    part[k].grad = None
                loss(data)["rec_loss"].backward()

            def native():
                step(loss_n)

            def baseline():
                step(loss_t)

            for fn in (native, baseline):
                for _ in range(WARM):
                    fn()
            torch.cuda.synchronize()
            assert loss_n.last_route == "native" and loss_t.last_route == "torch"
            tn, tb = [], []
            for _ in range(RUNS):
                tn.append(timed(native))
                tb.append(timed(baseline))
            out["shapes"].append({
                "patch": hw, "pc": pc, "C": C,
                "native_fwd_bwd_ms": [round(t, 4) for t in tn],
                "torch_route_fwd_bwd_ms": [round(t, 4) for t in tb],
                "native_median_ms": round(statistics.median(tn), 4),
                "torch_median_ms": round(statistics.median(tb), 4),
                "native_launches": launches(native), "torch_route_launches": launches(baseline),
                "native_faster_in_every_run": all(a < b for a, b in zip(tn, tb))})
    path = os.path.join(ROOT, "profiles", "recon_loss")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
