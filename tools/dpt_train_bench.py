#!/usr/bin/env python3
"""Diagnostic: DPT decoder forward + backward at the shipped shape (B = 1, 12x40 token grids
of a ViT-S, channels [64, 64, 128, 256] -> 256, 192x640 output grid).

  native:   DPTHead.train() through dpt_autograd (forward GEMMs for the data gradients,
            sd_conv_wgrad for the weight gradients), eager;
  baseline: what a user ran in its place before -- oracle.dpt_oracle.dpt_forward with torch
            autograd on the GPU under bf16 autocast.
Milliseconds per forward + backward (HIP events around 50 back-to-back steps after warm-up,
median of 7 rounds, native and baseline rounds interleaved), then the conv_wgrad call per
layer shape: microseconds per eager call between HIP events (200 calls, 7 rounds).  That is
call time, not kernel time: it holds the workspace allocation, the two launches
(k_conv_wgrad, k_cw_reduce) and, for the small layers, the host's launch cost; call_tflops is
the layer's FLOPs over it.  Prints one JSON line."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import dpt_oracle as DO  # noqa: E402
from scenedino_amd import _lib  # noqa: E402
from scenedino_amd.models.backbones.dino.dpt_head import DPTHead  # noqa: E402

dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)


def timeit(fns, iters, rounds=7, warm=5):
    """Median device time per call (ms) of each callable in fns, their rounds interleaved
    (a, b, a, b, ...) so that clock and thermal drift fall on all alike."""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(e) / iters)
    return [statistics.median(t) for t in ts]


_lib.load()
torch.manual_seed(0)
head = DPTHead(embed_dims=384, post_process_channels=[64, 64, 128, 256], d_out=256).to(dev).train()
xs = [torch.randn(1, 12, 40, 384, device=dev, generator=g).to(torch.bfloat16) for _ in range(4)]
xs_nchw = [x.float().permute(0, 3, 1, 2).contiguous() for x in xs]
go = torch.randn(1, 256, 192, 640, device=dev, generator=g)


def native_step():
    head.zero_grad(set_to_none=True)
    out = head.forward_nhwc(xs)[0]
    out.backward(go)


def native_fwd():
    with torch.no_grad():
        head.forward_nhwc(xs)


def torch_step():
    head.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = DO.dpt_forward(head, xs_nchw)
    out.backward(go.to(out.dtype))


t_native, t_torch, t_fwd = timeit([native_step, torch_step, native_fwd], 50)
res = {"native_fwd_bwd_ms": round(t_native, 3), "native_fwd_nograd_ms": round(t_fwd, 3),
       "torch_autocast_fwd_bwd_ms": round(t_torch, 3), "iters": 50, "rounds": 7}

layers = {}
for name, (H, W, Cin, Cout, taps, stride, relu) in {
        "proj_1x1_12x40_384to256": (12, 40, 384, 256, 1, 1, False),
        "up0_convT4_12x40_64to64": (12, 40, 64, 1024, 1, 1, False),
        "down3_3x3s2_12x40_256": (12, 40, 256, 256, 9, 2, False),
        "convs0_3x3_48x160_64to256": (48, 160, 64, 256, 9, 1, False),
        "rcu_3x3_6x20_256": (6, 20, 256, 256, 9, 1, True),
        "rcu_3x3_12x40_256": (12, 40, 256, 256, 9, 1, True),
        "rcu_3x3_24x80_256": (24, 80, 256, 256, 9, 1, True),
        "rcu_3x3_48x160_256": (48, 160, 256, 256, 9, 1, True),
        "fusion_project_1x1_48x160_256": (48, 160, 256, 256, 1, 1, False),
        "project_head0_3x3_96x320_256": (96, 320, 256, 256, 9, 1, False),
        "head1_convT2_96x320_256": (96, 320, 256, 1024, 1, 1, False),
        "head2_3x3_192x640_256": (192, 640, 256, 256, 9, 1, False)}.items():
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(1, H, W, Cin, device=dev, generator=g).to(torch.bfloat16)
    dy = torch.randn(1, OH, OW, Cout, device=dev, generator=g).to(torch.bfloat16)
    ms, = timeit([lambda: _lib.conv_wgrad(x, dy, taps=taps, stride=stride, relu_in=relu)], 200)
    layers[name] = {"call_us": round(ms * 1e3, 1),
                    "parts": _lib.conv_wgrad_parts(1, H, W, Cin, Cout, taps, stride),
                    "call_tflops": round(2 * OH * OW * Cout * taps * Cin / ms / 1e9, 1)}
print(json.dumps({"lib": os.environ.get("SDHIP_LIB") or "main", "step": res,
                  "conv_wgrad_call": layers}))
