#!/usr/bin/env python3
"""Diagnostic: one forward + backward of the ViT encoder alone (12 blocks, intermediate grids
of blocks 3 / 6 / 9 and the final grid, bf16 NHWC as the DPT decoder takes them).

  native:   vit_autograd.vit_forward_train (the forward kernels eager, sd_attention_bwd /
            sd_layernorm_bwd / sd_gelu_bwd, sd_gemm on transposed packs, sd_conv_wgrad);
  baseline: how the reference trains it -- torch autograd of the oracle block
            (oracle.vit_oracle) on the GPU under bf16 autocast.
Shapes: ViT-S/16 at 192x640 (481 tokens) with B = 1 and B = 4, DINOv2-B/14 at 168x560 (481
tokens, layer scale) with B = 1.  Milliseconds per forward + backward (HIP events around 20
back-to-back steps after warm-up, median of 7 rounds, native and baseline rounds interleaved),
the native no_grad forward for scale, then a per-kernel split of one block's backward:
microseconds per eager call between HIP events (100 calls, 7 rounds) -- call time (workspace
allocation, launches, host launch cost), not kernel time.  Prints one JSON line and writes it
to --out (default profiles/vit_train/bench.json)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import vit_oracle as VO  # noqa: E402
from scenedino_amd import _lib  # noqa: E402
from scenedino_amd.models.backbones.dino import vit as V  # noqa: E402
from scenedino_amd.models.backbones.dino import vit_autograd as VA  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit_train", "bench.json"))
opt = ap.parse_args()

dev = "cuda"
bf = torch.bfloat16
INTER = [3, 6, 9]


def timeit(fns, iters, rounds=7, warm=3):
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


def oracle_forward(vit, images, intermediate):
    """oracle.vit_oracle.encoder_forward's loop with grad enabled."""
    mean = VO.MEAN.to(images.device).view(1, 3, 1, 1)
    std = VO.STD.to(images.device).view(1, 3, 1, 1)
    x = ((images.float() / 2 + 0.5) - mean) / std
    B = x.shape[0]
    C, nh, p = vit.embed_dim, vit.num_heads, vit.patch_size
    gh, gw = x.shape[-2] // p, x.shape[-1] // p
    t = F.conv2d(x, vit.patch_embed.proj.weight, vit.patch_embed.proj.bias, stride=p)
    t = t.flatten(2).transpose(1, 2)
    t = torch.cat([vit.cls_token.expand(B, -1, -1), t], 1) + vit.pos_embed
    grids = []
    for i, b in enumerate(vit.blocks):
        t = VO.block(t, b, nh)
        if i in intermediate:
            grids.append(t[:, 1:].reshape(B, gh, gw, C))
    f = F.layer_norm(t, (C,), vit.norm.weight, vit.norm.bias, 1e-6)
    f = F.normalize(f[:, 1:], p=2, dim=2).reshape(B, gh, gw, C)
    return grids + [f]


def case(name, dim, heads, patch, img, B, ls):
    torch.manual_seed(0)
    g = torch.Generator(device=dev).manual_seed(0)
    vit = V.VisionTransformer(img, patch, dim, 12, heads, layer_scale=ls).to(dev).train()
    if ls:
        with torch.no_grad():
            for b in vit.blocks:
                b.ls1.gamma.fill_(1.0)
                b.ls2.gamma.fill_(1.0)
    images = torch.rand(B, 3, *img, device=dev, generator=g) * 2 - 1
    gh, gw = img[0] // patch, img[1] // patch
    gos = [torch.randn(B, gh, gw, dim, device=dev, generator=g) for _ in range(4)]
    gos_bf = [t.to(bf) for t in gos]
    packed = V._Packed(vit)

    def native_step():
        vit.zero_grad(set_to_none=True)
        grids, final = VA.vit_forward_train(vit, images, packed, INTER, nhwc=True)
        torch.autograd.backward(grids + [final], gos_bf)

    def native_fwd():
        with torch.no_grad():
            V.vit_forward(vit, images, packed, INTER, nhwc=True)

    def torch_step():
        vit.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=bf):
            outs = oracle_forward(vit, images, INTER)
        torch.autograd.backward(outs, [t.to(o.dtype) for t, o in zip(gos, outs)])

    t_native, t_torch, t_fwd = timeit([native_step, torch_step, native_fwd], 20)
    res = {"native_fwd_bwd_ms": round(t_native, 3), "torch_autocast_fwd_bwd_ms": round(t_torch, 3),
           "native_fwd_nograd_ms": round(t_fwd, 3), "tokens": gh * gw + 1, "batch": B}

    # per-kernel split of one block's backward at this shape
    T = gh * gw + 1
    M, C, Tp = B * T, dim, (T + 63) // 64 * 64
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    q = rnd(B, heads, T, 64).to(bf)
    k = torch.zeros(B, heads, Tp, 64, device=dev, dtype=bf)
    vt = torch.zeros(B, heads, 64, Tp, device=dev, dtype=bf)
    k[:, :, :T] = rnd(B, heads, T, 64).to(bf)
    vt[..., :T] = rnd(B, heads, 64, T).to(bf)
    ao = torch.empty(M, C, device=dev, dtype=bf)
    _lib.attention(q, k, vt, 0.125, ao)
    d_ao = rnd(M, C).to(bf)
    x, w = rnd(M, C), 1 + 0.1 * rnd(C)
    b0 = torch.zeros(C, device=dev)
    d = rnd(M, C)
    xn, dxn = rnd(M, C).to(bf), rnd(M, C).to(bf)
    u, dh = rnd(M, 4 * C).to(bf), rnd(M, 4 * C).to(bf)
    dqkv = rnd(M, 3 * C).to(bf)
    tpk = packed.train_packs()["blocks"][0]
    blk = packed.blocks[0]
    out_xn = torch.empty(M, C, device=dev, dtype=bf)
    split = {
        "attention_fwd": lambda: _lib.attention(q, k, vt, 0.125, ao),
        "attention_bwd": lambda: _lib.attention_bwd(q, k, vt, ao, d_ao, 0.125),
        "layernorm_bwd": lambda: _lib.layernorm_bwd(x, w, dxn, 1e-6, dx=d, accumulate=True),
        "layernorm_recompute": lambda: _lib.layernorm(x, w, b0, 1e-6, out_xn),
        "gelu_bwd": lambda: _lib.gelu_bwd(u, dh),
        "fc1_recompute_gemm": lambda: _lib.gemm(xn, blk["fc1_w"], blk["fc1_b"], _lib.SD_EPI_BF16, out=u),
        "dgrad_qkv": lambda: VA._dgrad(dqkv, tpk["qkv_wt"]),
        "dgrad_proj": lambda: VA._dgrad(dxn, tpk["proj_wt"]),
        "dgrad_fc1": lambda: VA._dgrad(dh, tpk["fc1_wt"]),
        "dgrad_fc2": lambda: VA._dgrad(dxn, tpk["fc2_wt"]),
        "wgrad_qkv": lambda: VA._wgrad(xn, dqkv),
        "wgrad_proj": lambda: VA._wgrad(ao, dxn),
        "wgrad_fc1": lambda: VA._wgrad(xn, dh),
        "wgrad_fc2": lambda: VA._wgrad(u, dxn),
    }
    names = list(split)
    ts = timeit([split[n] for n in names], 100)
    res["block_backward_call_us"] = {n: round(t * 1e3, 1) for n, t in zip(names, ts)}
    return res


_lib.load()
out = {"lib": os.environ.get("SDHIP_LIB") or "main", "iters": 20, "rounds": 7,
       "device": torch.cuda.get_device_name(0), "cases": {}}
for name, args in {"vit_s16_192x640_b1": (384, 6, 16, (192, 640), 1, False),
                   "vit_s16_192x640_b4": (384, 6, 16, (192, 640), 4, False),
                   "dinov2_b14_168x560_b1": (768, 12, 14, (168, 560), 1, True)}.items():
    out["cases"][name] = case(name, *args)
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
with open(opt.out, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
