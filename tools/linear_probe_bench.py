#!/usr/bin/env python3
"""Diagnostic: the linear probes of the downstream stage (direct_linear_head on 491 520 rows of
768 floats with the Dropout2d scale and targets, stego_linear_head on 491 520 rows of 64) at the
recipe's shape, 4 frames of 192 x 640.

  native:        sd_linear_probe (normalisation, scale, logits, argmax, cross-entropy, gW and gb
                 in one pass; the backward scales the saved gradients);
  torch_probes:  semantic_head._NATIVE_PROBES = False: _norm, the scale, nn.Linear, argmax and
                 F.cross_entropy as torch ops with autograd, the rest of the head native: the
                 route every step with ``segs`` took before the kernel existed;
  torch:         semantic_head._NATIVE = False: the whole head in torch ops.
Timed (tools/stego_train_bench.py's protocol: HIP events around ITERS back-to-back calls after
warm-up, RUNS runs of each variant, alternated in one process; every run is reported, with the
median and the spread max - min):
  * the two probe calls alone, forward + backward;
  * the whole step with ``segs``: forward_training + StegoLoss + backward (20 crops of 576
    points, mode "3d", dropout on, kNN buffer filled);
  * the peak allocated memory of one step of each.
``faster_than`` is True per baseline where its median exceeds native's by more than the two
spreads together.
This is eager time on a shared host, not kernel time.  The label table is the dataset
package's when it is importable, else a 20-entry stand-in (ids 0..18 -> trainIds 0..18, id 19 ->
255).  Writes profiles/linear_probe/bench.json and prints it as one JSON line."""
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scenedino_amd import _lib  # noqa: E402
from scenedino_amd.downstream_head import semantic_head as sh  # noqa: E402
from scenedino_amd.losses import StegoLoss  # noqa: E402
from stego_train_bench import CROPS, C_, H_, ITERS, LOSS, N_, POINTS, RUNS, V_, W_, WARM, timed  # noqa: E402

dev = "cuda"


def _stand_in_labels():
    if sh._kitti_labels() is not None:
        return
    lab = lambda i, t: types.SimpleNamespace(name=f"c{i}", id=i, trainId=t, color=(i, i, i))  # noqa: E731
    mod = types.ModuleType("datasets.kitti_360.labels")
    mod.labels = [lab(i, i) for i in range(19)] + [lab(19, 255)]
    mod.trainId2label = {l.trainId: l for l in mod.labels}
    pkg, sub = types.ModuleType("datasets"), types.ModuleType("datasets.kitti_360")
    pkg.__path__, sub.__path__ = [], []
    pkg.kitti_360, sub.labels = sub, mod
    sys.modules.update({"datasets": pkg, "datasets.kitti_360": sub, "datasets.kitti_360.labels": mod})


def _stats(ts):
    return {"runs": [round(t, 3) for t in ts], "median": round(statistics.median(ts), 3),
            "spread": round(max(ts) - min(ts), 3)}


def _compare(variants, warm=WARM):
    for _, fn in variants:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(RUNS):
        for name, fn in variants:
            times[name].append(timed(fn))
    out = {name: _stats(ts) for name, ts in times.items()}
    n = out["native"]
    out["faster_than"] = {name: bool(t["median"] - n["median"] > n["spread"] + t["spread"])
                          for name, t in list(out.items()) if name != "native"}
    return out


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    if not torch.cuda.is_available():
        raise SystemExit("linear_probe_bench: needs a ROCm device")
    _lib.load()
    _stand_in_labels()
    torch.manual_seed(0)
    head = sh.SemanticHead(19, 19, C_, 64, buffer_size=256, patch_sample_size=POINTS,
                           knn_neighbors=7, mode="3d").to(dev).train()
    loss_fn = StegoLoss(LOSS)
    img = torch.randn(N_, V_, H_, W_, 1, C_, device=dev)
    crops = torch.randn(1, CROPS, POINTS, C_, device=dev)
    sigma = torch.rand(1, CROPS, POINTS, device=dev)
    segs = torch.randint(0, 20, (N_, H_, W_), device=dev)
    target = head._train_id_lut(dev)[segs + 1]
    mask = (torch.rand(N_ * V_, C_, device=dev) >= 0.1).float() / 0.9
    codes = torch.nn.functional.normalize(torch.randn(N_, V_, H_, W_, 1, 64, device=dev), dim=-1)

    def probes():
        head.zero_grad(set_to_none=True)
        a = head.direct_linear_head(img, target, _mask=mask, _rows_per_group=H_ * W_, _normalize=True)
        b = head.stego_linear_head(codes, target)
        (a["loss"] + b["loss"]).backward()

    def step():
        data = {"coarse": [{"rgb": img[..., :3], "dino_features": img}], "sample_surface_sigma": sigma,
                "sample_surface_dino_features": crops, "segs": [segs]}
        head.zero_grad(set_to_none=True)
        loss_fn(head.forward_training(data))["total_loss"].backward()

    def route(fn, native, probes_native=True):
        def run():
            sh._NATIVE, sh._NATIVE_PROBES = native, probes_native
            try:
                fn()
            finally:
                sh._NATIVE = sh._NATIVE_PROBES = True
        return run

    out = {"iters": ITERS, "runs": RUNS, "image_rows": N_ * V_ * H_ * W_, "d_in": C_, "d_code": 64,
           "classes": 19, "crop_rows": CROPS * POINTS}
    out["probes_fwd_bwd_ms"] = _compare((("native", route(probes, True)),
                                         ("torch_probes", route(probes, True, False))))
    for _ in range(13):  # fill the kNN buffer (256 entries, 20 per step)
        step()
    variants = (("native", route(step, True)), ("torch_probes", route(step, True, False)),
                ("torch", route(step, False)))
    out["step_with_segs_ms"] = _compare(variants)
    out["peak_step_bytes"] = {name: _peak(fn) for name, fn in variants}
    out["peak_probes_bytes"] = {"native": _peak(route(probes, True)),
                                "torch_probes": _peak(route(probes, True, False))}
    out["direct_rows_bytes"] = N_ * V_ * H_ * W_ * C_ * 4
    path = os.path.join(ROOT, "profiles", "linear_probe")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
