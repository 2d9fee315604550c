"""DPT decoder, MI355X build.

Mirror of scenedino/models/backbones/dino/dpt_head.py:10-236 (``DPTHead``,
``ReassembleBlocks``, ``PreActResidualConvUnit``, ``FeatureFusionBlock``, ``OutputHead``):
same constructor arguments and parameter names (``reassemble_blocks.projects.{i}``,
``reassemble_blocks.resize_layers.{0,1,3}``, ``convs.{i}``,
``fusion_blocks.{i}.{project,res_conv_unit1,res_conv_unit2}.{conv1,conv2}``, ``project``,
``output_head.head_modules.{0,1,2}``), so the ``encoder.decoder.*`` keys of a SceneDINO
checkpoint load unchanged.  The forward pass runs on the gfx950 GEMM kernel of
csrc/sdhip_vit.hip with NHWC bf16 activations:
  * 1x1 convolutions: plain GEMMs over pixels;
  * ConvTranspose2d(k, stride k): one GEMM to k^2 Cout columns whose epilogue scatters
    every column block to its sub-pixel (SD_EPI_SHUF);
  * 3x3 convolutions (stride 1 / 2, padding 1): implicit GEMM, the im2col done by the
    A-tile loader (out-of-image taps read as zeros through the buffer bounds), the
    pre-activation ReLU of the residual units applied as the tile is loaded, the residual
    additions in the epilogue;
  * bilinear x2 (align_corners=True): sd_upsample2x;
  * the last convolution writes the NCHW f32 grid BTSNet samples (SD_EPI_NCHW).
Parity: tests/golden/dpt_head.npz, produced by the reference's own DPTHead on CPU.

One walk, ``forward_nhwc``, serves inference and training over one table of packed operands
(``_pack``, keyed by the convolution module).  In train mode with grad enabled every op of
the walk is the autograd Function of dpt_autograd.py around the same kernel call (data
gradients on the forward GEMM with rotated / transposed packs, weight gradients by
sd_conv_wgrad, csrc/sdhip_dpt_bwd.hip); the two modes differ only at levels 0 / 1 (folded for
inference, below), at the final convolution (``forward_last`` / the Function with the f32
output) and in what training refuses (``last=False``, fusion inputs of different sizes).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from .... import _lib
from ....pack_cache import module_key, track_steps
from . import dpt_autograd as A

# FeatureFusionBlock's 1x1 projection is applied before its x2 upsampling (the reference order,
# dpt_head.py:156-157, is upsample then project; exact in real arithmetic, one bf16 rounding
# moved).
# Inference, levels 0 / 1: the reassemble projection (1x1 conv) is folded into the
# ConvTranspose(k, stride k) behind it -- both linear, no padding, so W_t W_p x + (W_t b_p + b_t)
# is the same map in one GEMM (weights multiplied in fp32 on the host, one bf16 rounding of the
# product instead of one of the intermediate activations).  Training keeps the two GEMMs, so
# that every parameter gets its gradient.


class ReassembleBlocks(nn.Module):
    def __init__(self, in_channels=768, out_channels=None, readout_type="ignore", patch_size=16):
        super().__init__()
        out_channels = [96, 192, 384, 384] if out_channels is None else out_channels
        if readout_type != "ignore":
            raise NotImplementedError("readout_type 'ignore' only (dpt_head.py:41)")
        self.readout_type = readout_type
        self.patch_size = patch_size
        self.projects = nn.ModuleList([nn.Conv2d(in_channels, c, kernel_size=1) for c in out_channels])
        self.resize_layers = nn.ModuleList([
            nn.ConvTranspose2d(out_channels[0], out_channels[0], kernel_size=4, stride=4, padding=0),
            nn.ConvTranspose2d(out_channels[1], out_channels[1], kernel_size=2, stride=2, padding=0),
            nn.Identity(),
            nn.Conv2d(out_channels[3], out_channels[3], kernel_size=3, stride=2, padding=1),
        ])


class PreActResidualConvUnit(nn.Module):
    def __init__(self, in_channels, stride=1, dilation=1, bn=False):
        super().__init__()
        if bn or stride != 1 or dilation != 1:
            raise NotImplementedError("PreActResidualConvUnit(bn=False, stride 1, dilation 1) only")
        self.bn = bn
        self.act = nn.ReLU()
        self.conv1 = nn.Conv2d(in_channels, in_channels, 3, stride=stride, padding=dilation,
                               dilation=dilation, bias=True)
        self.conv2 = nn.Conv2d(in_channels, in_channels, 3, padding=1, bias=True)


class FeatureFusionBlock(nn.Module):
    def __init__(self, in_channels, expand=False, align_corners=True):
        super().__init__()
        self.in_channels = in_channels
        self.expand = expand
        self.align_corners = align_corners
        self.out_channels = in_channels // 2 if expand else in_channels
        self.project = nn.Conv2d(self.in_channels, self.out_channels, kernel_size=1)
        self.res_conv_unit1 = PreActResidualConvUnit(in_channels=self.in_channels)
        self.res_conv_unit2 = PreActResidualConvUnit(in_channels=self.in_channels)


class OutputHead(nn.Module):
    def __init__(self, latent_size=768):
        super().__init__()
        self.head_modules = nn.ModuleList([
            nn.Conv2d(latent_size, latent_size, kernel_size=3, stride=1, padding=1),
            nn.ConvTranspose2d(latent_size, latent_size, kernel_size=2, stride=2, padding=0),
            nn.Conv2d(latent_size, latent_size, kernel_size=3, stride=1, padding=1),
        ])


def _pack_conv3(conv):
    w = conv.weight.detach()  # (Cout, Cin, 3, 3) -> (Cout, ky, kx, ci)
    return (w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).to(torch.bfloat16).contiguous(),
            conv.bias.detach().float().contiguous() if conv.bias is not None else None)


def _pack_conv1(conv):
    w = conv.weight.detach()
    return (w.reshape(w.shape[0], -1).to(torch.bfloat16).contiguous(),
            conv.bias.detach().float().contiguous() if conv.bias is not None else None)


def _pack_proj_convT(proj, conv):
    """Conv2d(C, c, 1) followed by ConvTranspose2d(c, c', k, stride k) as one GEMM operand:
    (k k c', C) with column n = (dy k + dx) c' + co (_pack_convT's order), bias per column."""
    wp = proj.weight.detach().double().reshape(proj.weight.shape[0], -1)  # (c, C)
    bp = proj.bias.detach().double()
    w = conv.weight.detach().double()  # (c, c', k, k)
    cin, cout, k, _ = w.shape
    wt = w.permute(2, 3, 1, 0).reshape(k * k * cout, cin)  # (k k c', c)
    bt = conv.bias.detach().double().repeat(k * k)
    return ((wt @ wp).to(torch.bfloat16).contiguous(), (wt @ bp + bt).float().contiguous(), k)


def _pack_convT(conv):
    """ConvTranspose2d(k, stride k): weight (Cin, Cout, k, k) -> (k k Cout, Cin) with column
    n = (dy k + dx) Cout + co; bias repeated per sub-pixel."""
    w = conv.weight.detach()
    cin, cout, k, _ = w.shape
    wp = w.permute(2, 3, 1, 0).reshape(k * k * cout, cin)
    b = conv.bias.detach().float().repeat(k * k)
    return wp.to(torch.bfloat16).contiguous(), b.contiguous(), k


class DPTHead(nn.Module):
    """dpt_head.py:179-236.  ``forward(inputs)``: the reference contract (list of 4 NCHW
    feature grids -> [NCHW f32 grid]); ``forward_nhwc`` takes NHWC bf16 inputs directly
    (the ViT's token layout, no transposition)."""

    def __init__(self, embed_dims=768, post_process_channels=None, readout_type="ignore",
                 patch_size=16, d_out=384, expand_channels=False):
        super().__init__()
        post = list(post_process_channels) if post_process_channels else [96, 192, 384, 768]
        self.post_process_channels = [min(d_out, c) for c in post]
        self.d_out = d_out
        self.expand_channels = expand_channels
        self.reassemble_blocks = ReassembleBlocks(embed_dims, self.post_process_channels,
                                                  readout_type, patch_size)
        self.convs = nn.ModuleList([nn.Conv2d(c, d_out, kernel_size=3, padding=1, bias=False)
                                    for c in self.post_process_channels])
        self.fusion_blocks = nn.ModuleList([FeatureFusionBlock(d_out) for _ in self.convs])
        self.fusion_blocks[0].res_conv_unit1 = None
        self.project = nn.Conv2d(d_out, d_out, kernel_size=3, padding=1)
        self.output_head = OutputHead(d_out)
        self._packed = None

    def _pack(self, key=None, dgrad=False):
        """The packed operands per convolution module, re-packed when the parameters changed
        (``key``: this module's module_key if the caller has it already): 3x3 -> (wf, bf, wd),
        1x1 / ConvTranspose -> (wf, bf, k, wt), dpt_autograd's pack of each, and under the pair
        (projects[i], resize_layers[i]) of levels 0 / 1 their folded operand ("last": below).  The
        data-gradient operands (wd the rotated, wt the transposed weight) are None until a
        training pass asks for them (``dgrad``): an inference-only process never builds them
        (they double the bf16 weight footprint).  Adding them leaves the forward operands the
        tensors they were (a captured graph holds their pointers).  The cache entry is
        (module_key, table, whether the table holds the data-gradient operands)."""
        key = module_key(self) if key is None else key
        if self._packed is None or self._packed[0] != key:
            T = {}
            for m in self.modules():
                if isinstance(m, nn.ConvTranspose2d):
                    T[m] = _pack_convT(m) + (None,)
                elif isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3):
                    T[m] = _pack_conv3(m) + (None,)
                elif isinstance(m, nn.Conv2d):
                    assert m.kernel_size == (1, 1), m
                    T[m] = _pack_conv1(m) + (0, None)
            rb = self.reassemble_blocks
            for i in (0, 1):
                T[rb.projects[i], rb.resize_layers[i]] = _pack_proj_convT(rb.projects[i],
                                                                          rb.resize_layers[i])
            # forward_last's operands under a fixed key: the one launch behind every graph
            # replay then walks no submodule attributes (3 us of host time)
            T["last"] = T[self.output_head.head_modules[2]][:2]
            self._packed = (key, T, False)
        _, T, has_dgrad = self._packed
        if dgrad and not has_dgrad:  # the first training pass under this key
            for m, pk in list(T.items()):
                if isinstance(m, nn.Module):  # not the folded pairs: training runs them unfolded
                    # (wf, bf, wd): a 3x3 entry, from the weight; (wf, bf, k, wt): from wf
                    wd = A.pack_dgrad3(m.weight) if len(pk) == 3 else A.pack_dgrad1(pk[0])
                    T[m] = pk[:-1] + (wd,)
            self._packed = (key, T, True)
        return T

    def forward_nhwc(self, xs, last: bool = True):
        """xs: 4 NHWC bf16 tensors (B, h, w, embed) -> [f32 (B, d_out, H, W), channels-last].
        ``last=False`` stops before the final convolution and returns its NHWC bf16 input
        (``forward_last`` applies it: the graph-captured pass leaves that one launch out,
        so its output is a fresh tensor instead of a copy of a graph-owned buffer).
        In train mode with grad enabled every op goes through its dpt_autograd Function, in
        the unfolded form (every parameter its own operand, so every parameter gets its own
        gradient), eager, and the grid carries a grad_fn."""
        train = torch.is_grad_enabled() and self.training
        if train:
            if not last:
                raise NotImplementedError("scenedino_amd DPT: the training forward runs whole "
                                          "(no last=False)")
            track_steps(self)
        T = self._pack(dgrad=train)
        if train:
            def conv(x, m, **kw):
                return A.conv3x3(x, m, pack=T[m], **kw)

            def lin(x, m):
                return A.linear(x, m, pack=T[m])
            up = A.upsample2x
        else:
            def conv(x, m, **kw):
                wf, bf, _ = T[m]
                return _lib.conv3x3(x, wf, bf, **kw)

            def lin(x, m):
                wf, bf, k, _ = T[m]
                return _lib.linear_nhwc(x, wf, bf, shuf=k or None)
            up = _lib.upsample2x
        rb = self.reassemble_blocks
        def front(i, x):
            """The per-level front: the reassemble projection (+ its resize layer) and
            ``convs[i]`` (dpt_head.py:56-92, 226-229)."""
            if i < 2 and not train:  # the folded single GEMM (top of the file)
                wf, bf, k = T[rb.projects[i], rb.resize_layers[i]]
                y = _lib.linear_nhwc(x, wf, bf, shuf=k)
            else:
                y = lin(x, rb.projects[i])
                if i < 2:
                    y = lin(y, rb.resize_layers[i])
                elif i == 3:
                    y = conv(y, rb.resize_layers[3], stride=2)
            return conv(y, self.convs[i])

        def rcu(x, unit, extra=None):
            t = conv(x, unit.conv1, relu_in=True)
            return conv(t, unit.conv2, relu_in=True, res=x, res2=extra)  # conv2(..) + x (+ extra)

        def fusion(fb, x, res=None):
            if res is not None:
                if res.shape != x.shape:  # dpt_head.py:152-154 (not hit by 192x640 frames)
                    if train:
                        raise NotImplementedError("scenedino_amd DPT training: fusion inputs of "
                                                  "different sizes (dpt_head.py:152-154)")
                    res = F.interpolate(res.permute(0, 3, 1, 2).float(), size=x.shape[1:3],
                                        mode="bilinear", align_corners=False)
                    res = res.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()
                x = rcu(res, fb.res_conv_unit1, extra=x)            # x + rcu1(res)
            x = rcu(x, fb.res_conv_unit2)
            # project (1x1 conv) before the x2 upsampling: both are linear and the
            # align_corners bilinear weights sum to one (the bias passes through), so
            # upsample(project(x)) = project(upsample(x)) -- on a quarter of the pixels
            return up(lin(x, fb.project))

        f = [front(i, x) for i, x in enumerate(xs)]
        out = fusion(self.fusion_blocks[0], f[-1])
        for i in range(1, len(self.fusion_blocks)):
            out = fusion(self.fusion_blocks[i], out, f[-(i + 1)])
        hm = self.output_head.head_modules
        out = lin(conv(conv(out, self.project), hm[0]), hm[1])
        if train:  # the f32 grid through the Function: the permuted view carries the grad_fn
            return [conv(out, hm[2], f32_out=True).permute(0, 3, 1, 2)]
        return self.forward_last(out) if last else out

    def forward_last(self, x, key=None):
        """output_head.head_modules[2] (3x3 conv) on NHWC bf16 -> [(B, C, H, W) f32 grid].
        The grid is written channels-last (the GEMM's natural, coalesced output rows) and
        returned as its (B, C, H, W) permuted view: the reference's shape and values, and
        the layout every grid consumer here reads without a transposition
        (sd_project_grid_nhwc, sd_cast_grid, the training gather)."""
        w2, b2 = self._pack(key)["last"]
        return [_lib.conv3x3(x, w2, b2, epi=_lib.SD_EPI_F32).permute(0, 3, 1, 2)]

    def forward(self, inputs):
        """dpt_head.py:226-236: list of 4 NCHW grids -> [NCHW f32 grid]."""
        xs = [x.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous() for x in inputs]
        return self.forward_nhwc(xs)
