"""Differentiable ops of the DPT decoder: what the ops of ``DPTHead.forward_nhwc`` are in
train mode with grad enabled.

One ``torch.autograd.Function`` per decoder op.  Every Function takes the ``nn.Parameter``s
as inputs (autograd routes and accumulates their ``.grad``), makes the kernel call the
inference walk makes on the same packed operands (the head's ``_pack`` table; ``pack=None``
packs on the spot, for a single op), and saves the bf16 NHWC operands its backward needs.
  * data gradients reuse the forward GEMM (``sd_gemm``) on re-packed weights:
      - 3x3, stride 1: dX = conv3x3(dY, W') with W' the weight rotated by 180 degrees and
        Cin / Cout swapped, packed (Cin, ky, kx, co) (``pack_dgrad3``);
      - 3x3, stride 2: dY written into a zeroed (B, H, W, Cout) tensor at [::2, ::2], then
        the same stride-1 call (exact);
      - 1x1 and ConvTranspose2d(k, stride k): dX = dY W with dY un-shuffled to
        (B, H, W, k^2 Cout) rows for the transposed convolution (``pack_dgrad1``);
  * weight / bias gradients: ``sd_conv_wgrad`` (csrc/sdhip_dpt_bwd.hip), f32, permuted here
    from the packed (Cout, ky, kx, ci) order to the parameter's layout;
  * the pre-activation ReLU mask: ``sd_relu_bwd``; the bilinear x2: ``sd_upsample2x_bwd``.
Gradients that flow between layers are bf16 NHWC; weight and bias gradients stay f32.
"""
from __future__ import annotations

import torch

from .... import _lib


def pack_dgrad3(weight):
    """Conv2d weight (Cout, Cin, 3, 3) -> the conv3x3 operand of its data gradient:
    (Cin, 9 Cout) bf16, row ci, column (ky', kx', co) = weight[co, ci, 2 - ky', 2 - kx']."""
    w = weight.detach().flip(2, 3).permute(1, 2, 3, 0)
    return w.reshape(w.shape[0], -1).to(torch.bfloat16).contiguous()


def pack_dgrad1(packed_fwd):
    """The forward's packed (N, Cin) GEMM weight (1x1: N = Cout; ConvTranspose: N = k^2 Cout,
    _pack_convT's column order) -> (Cin, N) bf16 for dX = dY W."""
    return packed_fwd.t().contiguous()


def embed_stride2(dy, H, W):
    """dY (B, OH, OW, C) of a stride-2 convolution on an (H, W) input -> zeroed (B, H, W, C)
    with dY at [::2, ::2]: the stride-1 data gradient of that tensor is the stride-2 one."""
    z = torch.zeros(dy.shape[0], H, W, dy.shape[3], device=dy.device, dtype=dy.dtype)
    z[:, ::2, ::2] = dy
    return z


def _bf16_nhwc(g):
    return g.to(torch.bfloat16).contiguous()


class Conv3x3Fn(torch.autograd.Function):
    """y = conv3x3(relu?(x)) + bias (+ res) (+ res2) on NHWC bf16; ``f32_out``: the f32 NHWC
    grid of the decoder's last convolution.  wf / bf: the forward pack (_pack_conv3), wd:
    pack_dgrad3(weight)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, relu_in, res, res2, f32_out, wf, bf, wd):
        ctx.save_for_backward(x, wd)
        ctx.stride, ctx.relu_in, ctx.has_bias = stride, relu_in, bias is not None
        ctx.wshape = weight.shape
        return _lib.conv3x3(x, wf, bf, stride=stride, relu_in=relu_in, res=res, res2=res2,
                            epi=_lib.SD_EPI_F32 if f32_out else None)

    @staticmethod
    def backward(ctx, dy):
        x, wd = ctx.saved_tensors
        dy = _bf16_nhwc(dy)
        need = ctx.needs_input_grad
        dx = dw = db = None
        if need[1] or (ctx.has_bias and need[2]):
            dwp, db = _lib.conv_wgrad(x, dy, taps=9, stride=ctx.stride, relu_in=ctx.relu_in,
                                      bias=ctx.has_bias)
            cout, cin = ctx.wshape[0], ctx.wshape[1]
            dw = dwp.view(cout, 3, 3, cin).permute(0, 3, 1, 2)
        if need[0]:
            g = dy if ctx.stride == 1 else embed_stride2(dy, x.shape[1], x.shape[2])
            dx = _lib.conv3x3(g, wd, None)
            if ctx.relu_in:
                dx = _lib.relu_bwd(x, dx)
        return (dx, dw if need[1] else None, db if need[2] else None, None, None,
                dy if need[5] else None, dy if need[6] else None, None, None, None, None)


class LinearFn(torch.autograd.Function):
    """k = 0: 1x1 convolution (weight (N, Cin, 1, 1)); k > 0: ConvTranspose2d(k, stride k)
    (weight (Cin, Cout, k, k)) on NHWC bf16.  wf / bf: the forward pack (_pack_conv1 /
    _pack_convT), wt: pack_dgrad1(wf)."""

    @staticmethod
    def forward(ctx, x, weight, bias, k, wf, bf, wt):
        ctx.save_for_backward(x, wt)
        ctx.k, ctx.has_bias, ctx.wshape = k, bias is not None, weight.shape
        return _lib.linear_nhwc(x, wf, bf, shuf=k if k else None)

    @staticmethod
    def backward(ctx, dy):
        x, wt = ctx.saved_tensors
        k = ctx.k
        dy = _bf16_nhwc(dy)
        B, H, W, _ = x.shape
        if k:  # un-shuffle: (B, H k, W k, Cout) -> (B, H, W, (dy, dx, co))
            cout = dy.shape[3]
            dy = dy.view(B, H, k, W, k, cout).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, k * k * cout)
            dy = dy.contiguous()
        need = ctx.needs_input_grad
        dx = dw = db = None
        if need[1] or (ctx.has_bias and need[2]):
            dwp, db = _lib.conv_wgrad(x, dy, taps=1, bias=ctx.has_bias)
            if k:
                cin, cout = ctx.wshape[0], ctx.wshape[1]
                dw = dwp.view(k, k, cout, cin).permute(3, 2, 0, 1)
                db = db.view(k * k, cout).sum(0) if db is not None else None
            else:
                dw = dwp.view(ctx.wshape)
        if need[0]:
            dx = _lib.linear_nhwc(dy, wt, None)
        return dx, dw if need[1] else None, db if need[2] else None, None, None, None, None


class Upsample2xFn(torch.autograd.Function):
    """Bilinear x2, align_corners=True, on NHWC bf16."""

    @staticmethod
    def forward(ctx, x):
        return _lib.upsample2x(x)

    @staticmethod
    def backward(ctx, dy):
        return _lib.upsample2x_bwd(_bf16_nhwc(dy))


def conv3x3(x, conv, stride=1, relu_in=False, res=None, res2=None, f32_out=False, pack=None):
    """Differentiable 3x3 convolution of the module ``conv`` (nn.Conv2d, padding 1).
    pack: (wf, bf, wd) from the decoder's cache, or None to pack here."""
    if pack is None:
        from .dpt_head import _pack_conv3
        pack = _pack_conv3(conv) + (pack_dgrad3(conv.weight),)
    wf, bf, wd = pack
    return Conv3x3Fn.apply(x, conv.weight, conv.bias, stride, relu_in, res, res2, f32_out,
                           wf, bf, wd)


def linear(x, conv, pack=None):
    """Differentiable 1x1 convolution (nn.Conv2d) or ConvTranspose2d(k, stride k) of the
    module ``conv``.  pack: (wf, bf, k, wt) from the decoder's cache, or None."""
    if pack is None:
        from .dpt_head import _pack_conv1, _pack_convT
        if isinstance(conv, torch.nn.ConvTranspose2d):
            wf, bf, k = _pack_convT(conv)
        else:
            (wf, bf), k = _pack_conv1(conv), 0
        pack = (wf, bf, k, pack_dgrad1(wf))
    wf, bf, k, wt = pack
    return LinearFn.apply(x, conv.weight, conv.bias, k, wf, bf, wt)


def upsample2x(x):
    return Upsample2xFn.apply(x)
