#!/usr/bin/env python3
"""Diagnostic: the multi-scale-crop DINO targets of mode "upsample-gt" per loss image, after the
gt encoder: V = 4 views (two crops, the flip, the image), 12 x 40 token grids, 192 x 640 pixels,
C = 768 (ViT-B) and C = 384 (ViT-S).

  native:   sd_msc_gt (csrc/sdhip_msc.hip), one launch that writes the (1, C, H, W) result once;
  baseline: the path it replaces -- MultiScaleCropGT's torch route on the device, the reference's
            op sequence (upsample every view, warp_perspective, validity warp, NaN mask, nanmean
            in four channel chunks, normalise).
Milliseconds per image: HIP events around ITERS back-to-back calls after warm-up, three runs of
each, alternated, every run reported and the median.  GB/s is the result's bytes (C H W 4: 377 MB
at C = 768) over the time, beside the store floor of those bytes at 6 TB/s.  Peak transient
memory is torch's peak allocation during one call above what was allocated before it (the result
included).  Writes --out (default profiles/msc_gt/bench.json) and prints it as one JSON line."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scenedino_amd import _lib  # noqa: E402
from scenedino_amd.models.backbones.dino.upsampler import MultiScaleCropGT, view_transforms  # noqa: E402

dev = "cuda"
RUNS, WARM = 3, 3
ITERS = {"native": 20, "torch": 5}
H, W, HP, WP, V = 192, 640, 12, 40, 4
BOXES = [[[61, 17, 470, 141], [140, 30, 420, 126]]]
FLIPS = [[False, True]]
FLOOR_BPS = 6e12


def timed(fn, iters):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / iters


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def main():
    if not torch.cuda.is_available():
        raise SystemExit("msc_gt_bench: needs a ROCm device")
    out_path = os.path.join(ROOT, "profiles", "msc_gt", "bench.json")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
    _lib.load()
    out = {"runs": RUNS, "iters": ITERS, "V": V, "tokens": [HP, WP], "pixels": [H, W],
           "store_floor_GBps": FLOOR_BPS / 1e9, "shapes": []}
    T = view_transforms(torch.tensor(BOXES), torch.tensor(FLIPS), (H, W)).to(dev)
    for C in (768, 384):
        g = torch.Generator().manual_seed(C)
        feat = torch.nn.functional.normalize(torch.randn(1, V, C, HP, WP, generator=g), dim=2).to(dev)
        wn, wt = MultiScaleCropGT(None, V, (H, W)), MultiScaleCropGT(None, V, (H, W))
        wt.native = False

        def native():
            return wn.combine(feat, T, H, W)

        def baseline():
            return wt.combine(feat, T, H, W)

        for fn in (native, baseline):
            for _ in range(WARM):
                fn()
        torch.cuda.synchronize()
        assert wn.last_route == "native" and wt.last_route == "torch"
        diff = (native() - baseline()).abs().max().item()
        tn, tb = [], []
        for _ in range(RUNS):
            tn.append(timed(native, ITERS["native"]))
            tb.append(timed(baseline, ITERS["torch"]))
        nbytes = C * H * W * 4
        mn, mb = statistics.median(tn), statistics.median(tb)
        out["shapes"].append({
            "C": C, "result_MB": round(nbytes / 1e6, 1),
            "floor_ms": round(nbytes / FLOOR_BPS * 1e3, 4),
            "native_ms": [round(t, 4) for t in tn], "torch_route_ms": [round(t, 4) for t in tb],
            "native_median_ms": round(mn, 4), "torch_median_ms": round(mb, 4),
            "native_GBps": round(nbytes / mn / 1e6, 1), "torch_GBps": round(nbytes / mb / 1e6, 1),
            "native_peak_MB": round(peak_mb(native), 1), "torch_peak_MB": round(peak_mb(baseline), 1),
            "max_abs_diff": diff,
            "native_faster_in_every_run": all(a < b for a, b in zip(tn, tb))})
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
