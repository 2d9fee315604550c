#!/usr/bin/env python3
"""Diagnostic: the evaluation metrics of scenedino_amd/common/metrics.py, native kernels against
the same module's torch route, both on the GPU, at the validation shapes of one 192 x 640 frame:

  depth         compute_depth_metrics on (1, 1, 192, 640), the prediction as view 0 of two views;
  dino_patch    compute_dino_metrics at the patch grid, (1, 2, 24 * 80, 768);
  dino_full     compute_dino_metrics at full resolution (mode "upsample-gt"), (1, 2, 192 * 640,
                768): 755 MB per tensor, past the 256 MiB last-level cache, so this row is the
                HBM row.  ``bytes_per_s`` is rows * C * (pred element size + 4) over the median
                time, next to 6.3e12, the achievable HBM figure of a float4 copy on this part;
  seg_19x19,    compute_seg_metrics with 4 results (two with pseudo_segs_pred) on (1, 2, 192,
  seg_19x27     640) int64 labels, about 10 % of the targets -1.

The torch route is not the reference's code: it has the reference's operation order but none of
its ``torch.tensor([x.mean()])`` host reads, so the gap to the reference itself is larger than
the one reported here.  Timed with tools/stego_train_bench.py's protocol (HIP events around ITERS
back-to-back calls after warm-up, RUNS runs of each route, alternated in one process; every run is
reported, with the median and the spread max - min).  ``faster_than`` is True where the torch
median exceeds native's by more than the two spreads together.  This is eager time on a shared
host, not kernel time.  Writes profiles/eval_metrics/bench.json and prints it as one JSON line."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scenedino_amd import _lib  # noqa: E402
from scenedino_amd.common import metrics as M  # noqa: E402
from stego_train_bench import ITERS, RUNS, WARM, timed  # noqa: E402

dev = "cuda"
H_, W_, C_ = 192, 640, 768
HBM_ACHIEVABLE = 6.3e12


def _stats(ts):
    return {"runs": [round(t, 4) for t in ts], "median": round(statistics.median(ts), 4),
            "spread": round(max(ts) - min(ts), 4)}


def _compare(fn):
    variants = (("native", lambda: fn(True)), ("torch", lambda: fn(False)))
    for _, f in variants:
        for _ in range(WARM):
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(RUNS):
        for name, f in variants:
            times[name].append(timed(f))
    out = {name: _stats(ts) for name, ts in times.items()}
    n, t = out["native"], out["torch"]
    out["faster_than"] = {"torch": bool(t["median"] - n["median"] > n["spread"] + t["spread"])}
    return out


def _dino_row(P_hw, dtype=torch.float32):
    h, w = P_hw
    pred = torch.randn(1, 2, h, w, 1, C_, device=dev).to(dtype)
    gt = torch.randn(1, 2, h, w, C_, device=dev)
    data = {"dino_gt": gt, "coarse": [{"dino_features": pred}]}
    row = _compare(lambda native: M.compute_dino_metrics(data, native=native))
    nbytes = 2 * h * w * C_ * (pred.element_size() + 4)
    row["bytes"] = nbytes
    row["bytes_per_s"] = {k: round(nbytes / (row[k]["median"] * 1e-3)) for k in ("native", "torch")}
    return row


def _seg_row(n_classes):
    g = torch.Generator().manual_seed(n_classes)
    target = torch.randint(-1, 19, (1, H_, W_), generator=g)
    target[torch.rand(1, H_, W_, generator=g) < 0.1] = -1
    results = {}
    for r in range(4):
        pred, other = (torch.randint(0, n_classes, (1, 2, H_, W_), generator=g).to(dev) for _ in range(2))
        results[f"r{r}"] = {"segs_pred": other, "pseudo_segs_pred": pred} if r % 2 else {"segs_pred": pred}
    data = {"segmentation": {"target": target.to(dev), "results": results}}
    return _compare(lambda native: M.compute_seg_metrics(data, n_classes, 19, native=native))


def main():
    if not torch.cuda.is_available():
        raise SystemExit("eval_metrics_bench: needs a ROCm device")
    _lib.load()
    torch.manual_seed(0)
    out = {"iters": ITERS, "runs": RUNS, "unit": "ms per call", "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE}

    gt = torch.rand(1, 1, H_, W_, device=dev) * 70 + 1
    gt[torch.rand(1, 1, H_, W_, device=dev) < 0.7] = 0
    depth = (gt + 1).expand(1, 2, H_, W_) * (0.5 + torch.rand(1, 2, H_, W_, device=dev))
    out["depth"] = _compare(lambda native: M.compute_depth_metrics(gt, depth[:, :1], None, native=native))
    out["dino_patch"] = _dino_row((24, 80))
    out["dino_full"] = _dino_row((H_, W_))
    out["dino_full_bf16"] = _dino_row((H_, W_), torch.bfloat16)
    out["seg_19x19"] = _seg_row(19)
    out["seg_19x27"] = _seg_row(27)

    path = os.path.join(ROOT, "profiles", "eval_metrics")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
