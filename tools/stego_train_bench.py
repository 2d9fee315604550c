#!/usr/bin/env python3
"""Diagnostic: one training step of SemanticHead (forward_training + StegoLoss + backward) at the
downstream recipe's shape: 4 frames of 192 x 640 (491 520 image rows of 768 floats), 20 crops
of 576 points, mode "3d", dropout on, kNN buffer filled.

  native:   sd_stego_train_fwd on the image rows, sd_cluster_probe for both cluster heads, one
            _StegoTrainFn (sd_stego_train_fwd / _bwd + sd_conv_wgrad) for the crop rows;
  torch:    the same head with semantic_head._NATIVE = False: the torch-op fallback of the same
            math on the same device, in fp32 and under bf16 autocast.
Milliseconds per step: HIP events around ITERS back-to-back steps after warm-up, RUNS runs of
each variant, alternated (native, torch fp32, torch bf16, native, ...); every run is reported,
with the median and the spread (max - min) per variant.  The three heavy native calls are also
timed alone (events around ITERS calls).  This is eager step time on a shared host, not kernel
time.  Writes profiles/stego_train/bench.json and prints it as one JSON line.

``--loss`` measures the correlation loss instead and writes profiles/stego_loss/bench.json:
  * the native step with the eager correlation tensors (``lazy_corr = False``) against the step
    on StegoLoss's fused route (``lazy_corr = True``: sd_stego_corr_fwd / _bwd), same protocol,
    variants alternated, with the peak allocated memory of one step of each;
  * the parts of the native step after its three heavy forward calls, each timed alone as a
    forward + backward from leaf tensors: the six correlations + StegoLoss (eager and fused),
    _StegoTrainFn on the crop rows (forward, backward kernel, three sd_conv_wgrad), and what is
    left of the step (top-k, buffer update, cluster-loss autograd, host)."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scenedino_amd import _lib  # noqa: E402
from scenedino_amd.downstream_head import semantic_head as sh  # noqa: E402
from scenedino_amd.losses import StegoLoss  # noqa: E402

dev = "cuda"
ITERS, RUNS, WARM = 10, 3, 3
N_, V_, H_, W_, C_ = 4, 1, 192, 640, 768
CROPS, POINTS = 20, 576
LOSS = dict(random_weight=0.6702352279261414, knn_weight=0.4156436438453117,
            self_weight=0.08146997886146659, random_shift=0.8709334888837256,
            knn_shift=0.18458300726748128, self_shift=0.43610463774158115, pointwise=False)


def timed(fn, iters=ITERS):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / iters


def main():
    if not torch.cuda.is_available():
        raise SystemExit("stego_train_bench: needs a ROCm device")
    _lib.load()
    torch.manual_seed(0)
    head = sh.SemanticHead(19, 19, C_, 64, buffer_size=256, patch_sample_size=POINTS,
                           knn_neighbors=7, mode="3d").to(dev).train()
    loss_fn = StegoLoss(LOSS)
    img = torch.randn(N_, V_, H_, W_, 1, C_, device=dev)
    crops = torch.randn(1, CROPS, POINTS, C_, device=dev)
    sigma = torch.rand(1, CROPS, POINTS, device=dev)

    def step():
        data = {"coarse": [{"rgb": None, "dino_features": img}], "sample_surface_sigma": sigma,
                "sample_surface_dino_features": crops}
        data["coarse"][0]["rgb"] = img[..., :3]
        head.zero_grad(set_to_none=True)
        loss_fn(head.forward_training(data))["total_loss"].backward()

    def native():
        sh._NATIVE = True
        step()

    def torch32():
        sh._NATIVE = False
        step()
        sh._NATIVE = True

    def torch16():
        sh._NATIVE = False
        with torch.autocast("cuda", dtype=torch.bfloat16):
            step()
        sh._NATIVE = True

    variants = (("native", native), ("torch_fp32", torch32), ("torch_bf16_autocast", torch16))
    for _ in range(13):  # fill the kNN buffer (256 entries, 20 per step)
        native()
    for _, fn in variants:
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(RUNS):
        for name, fn in variants:
            times[name].append(timed(fn))
    out = {"iters": ITERS, "runs": RUNS, "image_rows": N_ * V_ * H_ * W_, "crop_rows": CROPS * POINTS,
           "d_in": C_, "step_ms": {}}
    for name, ts in times.items():
        out["step_ms"][name] = {"runs": [round(t, 3) for t in ts],
                                "median": round(statistics.median(ts), 3),
                                "spread": round(max(ts) - min(ts), 3)}

    # the heavy native calls alone
    rows = img.reshape(-1, C_)
    pack = head.stego_head._train_pack()
    mask = (torch.rand(N_ * V_, C_, device=dev) >= 0.1).float() / 0.9
    m64 = (torch.rand(N_ * V_, 64, device=dev) >= 0.1).float() / 0.9
    c768 = F.normalize(head.direct_cluster_head.cluster_centers.detach(), dim=1).contiguous()
    c64 = F.normalize(head.stego_cluster_head.cluster_centers.detach(), dim=1).contiguous()
    y, _ = _lib.stego_train_fwd(rows, pack, m64, m64, H_ * W_)
    x3 = torch.randn(3 * CROPS * POINTS, C_, device=dev)
    calls = {"sd_stego_train_fwd_image_rows": lambda: _lib.stego_train_fwd(rows, pack, m64, m64, H_ * W_),
             "sd_cluster_probe_768": lambda: _lib.cluster_probe(rows, c768, mask, H_ * W_),
             "sd_cluster_probe_64": lambda: _lib.cluster_probe(y, c64),
             "sd_stego_train_fwd_crop_rows_saving": lambda: _lib.stego_train_fwd(x3, pack, save=True,
                                                                                normalize=False)}
    out["call_ms"] = {}
    for name, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        ts = [timed(fn) for _ in range(RUNS)]
        out["call_ms"][name] = {"runs": [round(t, 3) for t in ts], "median": round(statistics.median(ts), 3)}
    flop = 2 * N_ * V_ * H_ * W_ * (C_ * C_ + 2 * 64 * C_)
    out["image_rows_stego_tflop"] = round(flop / 1e12, 3)
    path = os.path.join(ROOT, "profiles", "stego_train")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def loss_main():
    if not torch.cuda.is_available():
        raise SystemExit("stego_train_bench: needs a ROCm device")
    _lib.load()
    torch.manual_seed(0)
    head = sh.SemanticHead(19, 19, C_, 64, buffer_size=256, patch_sample_size=POINTS,
                           knn_neighbors=7, mode="3d").to(dev).train()
    loss_fn = StegoLoss(LOSS)
    img = torch.randn(N_, V_, H_, W_, 1, C_, device=dev)
    crops = torch.randn(1, CROPS, POINTS, C_, device=dev)
    sigma = torch.rand(1, CROPS, POINTS, device=dev)

    def step(lazy):
        head.lazy_corr = lazy
        data = {"coarse": [{"rgb": img[..., :3], "dino_features": img}], "sample_surface_sigma": sigma,
                "sample_surface_dino_features": crops}
        head.zero_grad(set_to_none=True)
        loss_fn(head.forward_training(data))["total_loss"].backward()

    variants = (("native_eager_corr", lambda: step(False)), ("native_fused_loss", lambda: step(True)))
    for _ in range(13):  # fill the kNN buffer (256 entries, 20 per step)
        step(False)
    for _, fn in variants:
        for _ in range(WARM):
            fn()
    assert loss_fn.last_route == "fused"
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(RUNS):
        for name, fn in variants:
            times[name].append(timed(fn))
    out = {"iters": ITERS, "runs": RUNS, "image_rows": N_ * V_ * H_ * W_, "crops": CROPS, "points": POINTS,
           "d_in": C_, "pointwise": LOSS["pointwise"], "step_ms": {}, "peak_step_bytes": {}}
    for name, ts in times.items():
        out["step_ms"][name] = {"runs": [round(t, 3) for t in ts],
                                "median": round(statistics.median(ts), 3),
                                "spread": round(max(ts) - min(ts), 3)}
    for name, fn in variants:
        head.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        out["peak_step_bytes"][name] = torch.cuda.max_memory_allocated() - base
    out["six_corr_tensors_bytes"] = 6 * CROPS * POINTS * POINTS * 4

    # the parts, each from leaf tensors
    dino = [F.normalize(torch.randn(CROPS, POINTS, C_, device=dev), dim=-1) for _ in range(3)]
    y3 = F.normalize(torch.randn(3, CROPS, POINTS, 64, device=dev), dim=-1).requires_grad_(True)
    x3 = torch.cat([t.reshape(-1, C_) for t in dino])
    dy = torch.randn(3 * CROPS * POINTS, 64, device=dev)

    def corr_loss(lazy):
        y3.grad = None
        corr = head._compute_stego_correlation
        rows = (y3[0], y3[1], y3[2])
        c = sh.StegoCorrMap(dino, rows, corr) if lazy else {
            f"{k}_{p}_corr": corr(r[0], r[i]) for k, r in (("dino", dino), ("stego", rows))
            for i, p in enumerate(("self", "nn", "random"))}
        zero = {"loss": torch.zeros((), device=dev)}
        data = {"segmentation": {"stego_corr": c, "results": {"direct_cluster": zero, "stego_cluster": zero}}}
        loss_fn(data)["total_loss"].backward()

    def stego_fn():
        head.zero_grad(set_to_none=True)
        head.stego_head.train_rows(x3, rows_per_group=POINTS, normalize=False).backward(dy)

    pack = head.stego_head._train_pack()
    parts = {"corr_and_loss_fwd_bwd_eager": lambda: corr_loss(False),
             "corr_and_loss_fwd_bwd_fused": lambda: corr_loss(True),
             "stego_train_fn_fwd_bwd_wgrad": stego_fn,
             "stego_train_fn_fwd_only": lambda: _lib.stego_train_fwd(x3, pack, save=True, normalize=False)}
    out["part_ms"] = {}
    for name, fn in parts.items():
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        ts = [timed(fn) for _ in range(RUNS)]
        out["part_ms"][name] = {"runs": [round(t, 3) for t in ts], "median": round(statistics.median(ts), 3)}
    assert loss_fn.last_route == "fused"
    path = os.path.join(ROOT, "profiles", "stego_loss")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    loss_main() if "--loss" in sys.argv[1:] else main()
