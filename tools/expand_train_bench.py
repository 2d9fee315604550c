#!/usr/bin/env python3
"""Diagnostic: forward + backward of MlpDimReduction.transform_expand in training, P rows of
64-d codes -> d_full, P = 2048 / 8192 (a training batch's rendered rays), d_full = 384 / 768.

  native:   the module's transform_expand (sd_seg_query forward; sd_expand_bwd + two
            sd_conv_wgrad calls backward), eager;
  baseline: the path it replaces -- the same module's parameters through
            F.normalize(linear_out(relu(linear_in(x))), dim=-1) with torch autograd on the
            device under bf16 autocast.
Milliseconds per forward + backward, input and all four parameters requiring grad: HIP events
around 200 back-to-back steps after warm-up, three runs of each, alternated (native, baseline,
native, ...), every run reported and the median.  This is eager step time -- it holds the
host's launch and allocation cost of every op, which at these sizes is most of it -- not
kernel time.  Writes profiles/expand_train/bench.json and prints it as one JSON line."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scenedino_amd import _lib  # noqa: E402
from scenedino_amd.models.backbones.dino.dim_reduction import MlpDimReduction  # noqa: E402

dev = "cuda"
ITERS, RUNS, WARM = 200, 3, 20


def timed(fn):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / ITERS


def main():
    if not torch.cuda.is_available():
        raise SystemExit("expand_train_bench: needs a ROCm device")
    _lib.load()
    out = {"iters": ITERS, "runs": RUNS, "shapes": []}
    for DF in (384, 768):
        for P in (2048, 8192):
            torch.manual_seed(DF + P)
            m = MlpDimReduction(DF, 64, 128).to(dev).train()
            x = torch.randn(P, 64, device=dev, requires_grad=True)
            go = torch.randn(P, DF, device=dev)

            def native():
                m.zero_grad(set_to_none=True)
                x.grad = None
                m.transform_expand(x).backward(go)

            def baseline():
                m.zero_grad(set_to_none=True)
                x.grad = None
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    y = F.normalize(m.linear_out(F.relu(m.linear_in(x))), dim=-1)
                y.backward(go.to(y.dtype))

            for fn in (native, baseline):
                for _ in range(WARM):
                    fn()
            torch.cuda.synchronize()
            tn, tb = [], []
            for _ in range(RUNS):
                tn.append(timed(native))
                tb.append(timed(baseline))
            out["shapes"].append({
                "P": P, "d_full": DF,
                "native_fwd_bwd_ms": [round(t, 4) for t in tn],
                "torch_autocast_fwd_bwd_ms": [round(t, 4) for t in tb],
                "native_median_ms": round(statistics.median(tn), 4),
                "torch_median_ms": round(statistics.median(tb), 4)})
    path = os.path.join(ROOT, "profiles", "expand_train")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
