"""Differentiable training path of the native ViT (the backward of vit.py's vit_forward).

The reference fine-tunes the ViT whenever ``encoder_freeze`` is false (scenedino/models/
backbones/dino/vit.py:112-189 under autograd, dinov2_module.py:176-183) in its own Adam
group at lr / 10 (scenedino/training/trainer.py:561-573).  ``vit_forward_train`` is one
``torch.autograd.Function`` over the whole encoder: its inputs are the parameters, its
forward is ``vit_forward`` itself with a tape (the default route's kernels, so the grids are
bit-equal to the inference pass on the same weights), eager, keeping what the backward needs;
its backward walks the blocks in reverse.

Saved per block: the two LayerNorm inputs (f32 copies of the residual stream before the
block and after its attention half), the block's own q / K / V^T (never the per-shape shared
buffers of ``_Packed._kv``), the attention output and the post-GELU hidden rows.  Recomputed
in the backward: the two normalised row sets (sd_layernorm), the pre-GELU fc1 output (one
SD_EPI_BF16 fc1 GEMM on the re-normalised rows) and the softmax (sd_attention_bwd's first
sweep recomputes the row statistics, its two main kernels recompute S and P per tile).

Backward pieces:
  * linear data gradients: sd_gemm on the transposed bf16 packs (``_Packed.train_packs``);
  * linear weight / bias gradients: sd_conv_wgrad with taps = 1 (token rows as pixels);
  * residual epilogue with layer scale x += gamma o (a W^T + b): ``layer_scale_grads`` from
    one sd_conv_wgrad on the unscaled gradient, the data gradient from bf16(gamma o d);
  * sd_attention_bwd, sd_layernorm_bwd (accumulating into the f32 residual gradient),
    sd_gelu_bwd (csrc/sdhip_vit_bwd.hip);
  * the tail's L2 normalisation, the layer-scale products, pos_embed / cls_token sums and
    bf16 casts: small torch tensor ops.
Gradients along the residual stream are f32 (B T, C); GEMM operand gradients are bf16;
weight and bias gradients are f32.  The LN-tail / fused-MLP A/B variants of vit_forward are
ignored: the training path always takes the default route.
"""
from __future__ import annotations

from typing import List

import torch
import torch.nn.functional as F

from .... import _lib
from .vit import vit_forward

EPS = 1e-6


def pack_t(w):
    """Forward GEMM pack (N, K) -> the sd_gemm operand of its data gradient, (K, N)
    contiguous: dX = dY W = sd_gemm(dY, pack_t(W)) (sd_gemm multiplies by its operand's
    transpose)."""
    return w.t().contiguous()


def layer_scale_grads(G, s, W, b, gamma):
    """Gradients of y = x + gamma o (a W^T + b) from G = d^T a (N, K) and s = colsum(d) (N),
    d the gradient of y: (dW, db, dgamma).  gamma None: plain residual (dgamma None)."""
    if gamma is None:
        return G, s, None
    return gamma[:, None] * G, gamma * s, (W * G).sum(1) + b * s


def vit_params(vit):
    """The ViT's parameters in the order _VitFn takes them, with their names."""
    names, params = [], []

    def add(n, p):
        names.append(n)
        params.append(p)

    add("cls_token", vit.cls_token)
    add("pos_embed", vit.pos_embed)
    add("patch_embed.proj.weight", vit.patch_embed.proj.weight)
    add("patch_embed.proj.bias", vit.patch_embed.proj.bias)
    for i, b in enumerate(vit.blocks):
        pre = f"blocks.{i}."
        add(pre + "norm1.weight", b.norm1.weight)
        add(pre + "norm1.bias", b.norm1.bias)
        add(pre + "attn.qkv.weight", b.attn.qkv.weight)
        add(pre + "attn.qkv.bias", b.attn.qkv.bias)
        add(pre + "attn.proj.weight", b.attn.proj.weight)
        add(pre + "attn.proj.bias", b.attn.proj.bias)
        if b.ls1 is not None:
            add(pre + "ls1.gamma", b.ls1.gamma)
        add(pre + "norm2.weight", b.norm2.weight)
        add(pre + "norm2.bias", b.norm2.bias)
        add(pre + "mlp.fc1.weight", b.mlp.fc1.weight)
        add(pre + "mlp.fc1.bias", b.mlp.fc1.bias)
        add(pre + "mlp.fc2.weight", b.mlp.fc2.weight)
        add(pre + "mlp.fc2.bias", b.mlp.fc2.bias)
        if b.ls2 is not None:
            add(pre + "ls2.gamma", b.ls2.gamma)
    add("norm.weight", vit.norm.weight)
    add("norm.bias", vit.norm.bias)
    return names, params


def _wgrad(a, dy):
    """G = dy^T a (N, K) and s = colsum(dy) (N), f32, from bf16 rows (sd_conv_wgrad, taps 1)."""
    rows, K = a.shape
    return _lib.conv_wgrad(a.view(1, 1, rows, K), dy.view(1, 1, rows, dy.shape[1]), taps=1)


def _dgrad(dy, wt):
    """dX = dY W as bf16 rows (sd_gemm on the transposed pack)."""
    out = torch.empty(dy.shape[0], wt.shape[0], device=dy.device, dtype=torch.bfloat16)
    _lib.gemm(dy, wt, None, _lib.SD_EPI_BF16, out=out)
    return out


def _l2_bwd(y, g):
    """Gradient of z = y / max(|y|, 1e-12) (rows of y) given g = dL/dz.  F.normalize applied
    twice (vit.py:188, dinov2_module.py:282) has the same gradient: the second pass divides a
    unit vector by its norm, and its Jacobian there is the projection the first one applies."""
    n = y.norm(dim=1, keepdim=True).clamp_min(1e-12)
    z = y / n
    return (g - z * (z * g).sum(1, keepdim=True)) / n


class _Cfg:
    """Non-tensor arguments of _VitFn (one object, so autograd sees a single non-tensor)."""

    def __init__(self, vit, images, packed, intermediate, nhwc, names):
        self.vit, self.images, self.packed = vit, images, packed
        self.intermediate, self.nhwc, self.names = list(intermediate), nhwc, names


class _VitFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, *params):
        vit, saved = cfg.vit, []
        grids, final = vit_forward(vit, cfg.images, cfg.packed, cfg.intermediate, cfg.nhwc,
                                   tape=saved)
        ctx.save_for_backward(*saved)
        ctx.cfg = cfg
        B, _, H, W = cfg.images.shape
        gh, gw = H // vit.patch_size, W // vit.patch_size
        ctx.dims = (B, gh * gw + 1, vit.embed_dim, vit.num_heads, gh, gw)
        return tuple(grids) + (final,)

    @staticmethod
    def backward(ctx, *gouts):
        cfg = ctx.cfg
        packed, names, nhwc = cfg.packed, cfg.names, cfg.nhwc
        tp = packed.train_packs()
        B, T, C, nh, gh, gw = ctx.dims
        Np = T - 1
        saved = ctx.saved_tensors
        patches, x_last = saved[0], saved[-1]
        need = dict(zip(names, ctx.needs_input_grad[1:]))
        grads = {}
        bf = torch.bfloat16
        scale = (C // nh) ** -0.5

        def rows_of(g):
            """Gradient of a token grid -> f32 (B, Np, C) rows."""
            if g is None:
                return None
            if nhwc:
                return g.reshape(B, Np, C).float()
            return g.reshape(B, C, Np).transpose(1, 2).float()

        # tail: final norm -> L2 normalisation -> grid
        d = torch.zeros(B * T, C, device=x_last.device)
        gf = rows_of(gouts[-1])
        if gf is not None:
            y = torch.empty(B * T, C, device=x_last.device)
            _lib.layernorm(x_last, packed.nw, packed.nb, EPS, y)
            dy = torch.zeros(B, T, C, device=x_last.device)
            dy[:, 1:] = _l2_bwd(y.view(B, T, C)[:, 1:].reshape(B * Np, C),
                                gf.reshape(B * Np, C)).view(B, Np, C)
            want = need["norm.weight"] or need["norm.bias"]
            _, dw, db = _lib.layernorm_bwd(x_last, packed.nw, dy.view(B * T, C), EPS, dx=d,
                                           accumulate=False, want_wb=want)
            if need["norm.weight"]:
                grads["norm.weight"] = dw
            if need["norm.bias"]:
                grads["norm.bias"] = db

        def residual(pre, wname, a, d, w_f, b_f, gamma, gname, wt):
            """Backward of x += gamma o (a W^T + b): parameter gradients into grads, returns
            the bf16 data gradient of a."""
            want_w = need[pre + wname + ".weight"] or need[pre + wname + ".bias"]
            want_g = gamma is not None and need[pre + gname]
            if want_w or want_g:
                G, s = _wgrad(a, d.to(bf))
                dW, db, dg = layer_scale_grads(G, s, w_f.float(), b_f, gamma)
                if need[pre + wname + ".weight"]:
                    grads[pre + wname + ".weight"] = dW
                if need[pre + wname + ".bias"]:
                    grads[pre + wname + ".bias"] = db
                if want_g:
                    grads[pre + gname] = dg
            dsc = (d if gamma is None else d * gamma).to(bf)
            return _dgrad(dsc, wt)

        def norm_bwd(pre, nname, x_ln, w, dxn, d):
            want = need[pre + nname + ".weight"] or need[pre + nname + ".bias"]
            _, dw, db = _lib.layernorm_bwd(x_ln, w, dxn, EPS, dx=d, accumulate=True, want_wb=want)
            if need[pre + nname + ".weight"]:
                grads[pre + nname + ".weight"] = dw
            if need[pre + nname + ".bias"]:
                grads[pre + nname + ".bias"] = db

        def linear_wb(pre, lname, a, dy):
            if need[pre + lname + ".weight"] or need[pre + lname + ".bias"]:
                G, s = _wgrad(a, dy)
                if need[pre + lname + ".weight"]:
                    grads[pre + lname + ".weight"] = G
                if need[pre + lname + ".bias"]:
                    grads[pre + lname + ".bias"] = s

        gi = len(cfg.intermediate)
        nblk = len(packed.blocks)
        xn = torch.empty(B * T, C, device=x_last.device, dtype=bf)
        for i in range(nblk - 1, -1, -1):
            blk, tblk = packed.blocks[i], tp["blocks"][i]
            x_in, q, k, vt, ao, x_mid, hid = saved[1 + 7 * i: 8 + 7 * i]
            pre = f"blocks.{i}."
            if i in cfg.intermediate:  # this block's output grid: rows 1 .. T - 1 of each image
                gi -= 1
                g = rows_of(gouts[gi])
                if g is not None:
                    d.view(B, T, C)[:, 1:] += g
            # MLP half: x_out = x_mid + ls2 o (gelu(LN2(x_mid) W1^T + b1) W2^T + b2)
            dh = residual(pre, "mlp.fc2", hid, d, blk["fc2_w"], blk["fc2_b"], blk["ls2"],
                          "ls2.gamma", tblk["fc2_wt"])
            _lib.layernorm(x_mid, blk["n2w"], blk["n2b"], EPS, xn)
            u = torch.empty_like(hid)
            _lib.gemm(xn, blk["fc1_w"], blk["fc1_b"], _lib.SD_EPI_BF16, out=u)
            du = _lib.gelu_bwd(u, dh)
            linear_wb(pre, "mlp.fc1", xn, du)
            norm_bwd(pre, "norm2", x_mid, blk["n2w"], _dgrad(du, tblk["fc1_wt"]), d)
            # attention half: x_mid = x_in + ls1 o (attn(LN1(x_in)) Wp^T + bp)
            d_ao = residual(pre, "attn.proj", ao, d, blk["proj_w"], blk["proj_b"], blk["ls1"],
                            "ls1.gamma", tblk["proj_wt"])
            d_qkv = _lib.attention_bwd(q, k, vt, ao, d_ao, scale)
            _lib.layernorm(x_in, blk["n1w"], blk["n1b"], EPS, xn)
            linear_wb(pre, "attn.qkv", xn, d_qkv)
            norm_bwd(pre, "norm1", x_in, blk["n1w"], _dgrad(d_qkv, tblk["qkv_wt"]), d)
        # embedding: x0[b, 0] = cls + pos[0], x0[b, 1 + n] = patches W^T + b + pos[1 + n]
        d3 = d.view(B, T, C)
        if need["pos_embed"]:
            grads["pos_embed"] = d3.sum(0, keepdim=True)
        if need["cls_token"]:
            grads["cls_token"] = d3[:, 0].sum(0).view(1, 1, C)
        if need["patch_embed.proj.weight"] or need["patch_embed.proj.bias"]:
            # sd_conv_wgrad wants Cin % 64 == 0: the patch rows (Kp a multiple of 32) padded
            # with zero columns here, the forward GEMM keeps its operands and its bits
            k_raw = 3 * cfg.vit.patch_size ** 2
            Kp64 = (k_raw + 63) // 64 * 64
            p64 = patches if Kp64 == packed.Kp else F.pad(patches, (0, Kp64 - packed.Kp))
            G, s = _wgrad(p64, d3[:, 1:].to(bf).reshape(B * Np, C))
            if need["patch_embed.proj.weight"]:
                grads["patch_embed.proj.weight"] = G[:, :k_raw].reshape(
                    cfg.vit.patch_embed.proj.weight.shape)
            if need["patch_embed.proj.bias"]:
                grads["patch_embed.proj.bias"] = s
        return (None,) + tuple(grads.get(n) if need[n] else None for n in names)


def vit_forward_train(vit, images: torch.Tensor, packed, intermediate: List[int],
                      nhwc: bool = False):
    """vit_forward with a backward: same arguments, returns (grids, final) in the same
    ``nhwc=True`` (bf16 NHWC) or f32 NCHW layouts, bit-equal to vit_forward under no_grad on
    the same weights, carrying a grad_fn that fills ``.grad`` of every ViT parameter that
    requires grad.  No image gradient is produced."""
    if images.requires_grad:
        raise NotImplementedError("scenedino_amd ViT training path: no gradient with respect to "
                                  "the input image; pass it detached")
    names, params = vit_params(vit)
    outs = _VitFn.apply(_Cfg(vit, images, packed, intermediate, nhwc, names), *params)
    return list(outs[:-1]), outs[-1]
