"""DINO feature dimension reduction, MI355X build.

Mirror of scenedino/models/backbones/dino/dim_reduction.py:6-25 (same class names,
constructor arguments and parameter names ``linear_in`` / ``linear_out``, so the
reference's ``encoder.dim_reduction.*`` checkpoint keys load unchanged).
``MlpDimReduction.transform_expand`` (64 -> 128 ReLU -> d_full, L2-normalised) runs in
the gfx950 kernel ``sd_seg_query`` (expand-only record, csrc/sdhip_seg.hip).

Training (the reference's step expands the rendered features right after the render,
scenedino/training/trainer.py:288,441-445, and optimises ``linear_in`` / ``linear_out`` in its
first Adam group, trainer.py:565-568): in train mode with grad enabled and either the input or
a parameter requiring grad, ``transform_expand`` runs ``_ExpandFn`` (eval mode, ``no_grad`` and
a frozen module on a detached input keep the plain kernel call).  Its forward is the same
``sd_seg_query`` call (the training output is bit-equal to the eval output); its backward is
``sd_expand_bwd`` (csrc/sdhip_expand_bwd.hip: dx, and the bf16 rows h, de, dh, x) plus two
``sd_conv_wgrad`` calls with taps = 1 for dW2 / db2 and dW1 / db1, as the ViT backward forms its
linear weight gradients (vit_autograd.py).  Nothing is saved but the input codes; the
backward reads the packs the forward read, so a step between forward and backward does not
mix weights.

Packed weights and optimizer steps: the record is cached on ``pack_cache.module_key`` (data
pointers, version counters and, because torch's fused Adam bumps no version counter, the steps
of optimizers holding one of the module's parameters, counted from its first differentiable
``transform_expand``).  A module that never trained is not tracked and keys as its raw tensors.
After an update no hook sees (a ``.data`` write, a replayed graph that captured the step) set
``module._packed = None``.
"""
from __future__ import annotations

import torch
from torch import nn

from .... import _lib  # noqa: F401  (fail loudly on a box without the HIP library)
from ....pack_cache import module_key, track_steps


class NoDimReduction(nn.Module):
    """dim_reduction.py:6-12: identity (full == reduced)."""

    def __init__(self, full_channels, reduced_channels):
        super().__init__()
        if full_channels != reduced_channels:
            raise ValueError("NoDimReduction needs full_channels == reduced_channels")

    def forward(self, features):
        return features

    def transform_expand(self, features):
        return features


def _wgrad(a, dy, bias):
    """dy^T a (N, K) and colsum(dy) (N) | None, f32, from bf16 rows (sd_conv_wgrad, taps 1)."""
    rows, K = a.shape
    return _lib.conv_wgrad(a.view(1, 1, rows, K), dy.view(1, 1, rows, dy.shape[1]), taps=1,
                           bias=bias)


class _ExpandFn(torch.autograd.Function):
    """x (P, 64) f32 -> F.normalize(linear_out(relu(linear_in(x))), dim=-1) (P, d_full) f32.
    The four parameters are inputs so that autograd routes their gradients; the kernels read
    the packed copies."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, module):
        packs = module._packs(train=True)
        _, _, full = _lib.seg_query(x, packs[0].rec, want_labels=False, want_full=True)
        ctx.save_for_backward(x)
        ctx.packs = packs
        return full

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        seg, bwd = ctx.packs
        need_x, need_w1, need_b1, need_w2, need_b2 = ctx.needs_input_grad[:5]
        if x.shape[0] == 0:
            z = lambda need, t: torch.zeros_like(t) if need else None  # noqa: E731
            return (z(need_x, x), z(need_w1, bwd.w1.float()), z(need_b1, bwd.b1),
                    z(need_w2, bwd.w2.float()), z(need_b2, bwd.b2), None)
        dy = dy.float().contiguous()
        want1, want2 = need_w1 or need_b1, need_w2 or need_b2
        dx, h, de, dh, xb = _lib.expand_bwd(x, seg.rec, bwd, dy, want_w1=want1, want_w2=want2)
        dw1 = db1 = dw2 = db2 = None
        if want2:
            dw2, db2 = _wgrad(h, de, need_b2)
        if want1:
            dw1, db1 = _wgrad(xb, dh, need_b1)
        return (dx if need_x else None, dw1 if need_w1 else None, db1 if need_b1 else None,
                dw2 if need_w2 else None, db2 if need_b2 else None, None)


class MlpDimReduction(nn.Module):
    """dim_reduction.py:15-25."""

    def __init__(self, full_channels, reduced_channels, latent_channels):
        super().__init__()
        self.linear_in = nn.Linear(reduced_channels, latent_channels)
        self.linear_out = nn.Linear(latent_channels, full_channels)
        self.relu = nn.ReLU()
        self._packed = None

    def _key(self):
        return module_key(self)

    def _packs(self, train=False):
        """(PackedSegHead, PackedExpandBwd | None) of the current weights; the backward's
        operands are packed on the first training call of a key."""
        from ....seg_pack import PackedExpandBwd, PackedSegHead
        key = self._key()
        if self._packed is None or self._packed[0] != key:
            self._packed = (key, PackedSegHead(self), None)
        if train and self._packed[2] is None:
            self._packed = (key, self._packed[1], PackedExpandBwd(self))
        return self._packed[1], self._packed[2]

    def _rec(self):
        return self._packs()[0]

    def transform_expand(self, features: torch.Tensor) -> torch.Tensor:
        """features (..., reduced) -> F.normalize(linear_out(relu(linear_in(x))), dim=-1)."""
        lead = features.shape[:-1]
        x = features.reshape(-1, features.shape[-1]).float().contiguous()
        params = (self.linear_in.weight, self.linear_in.bias, self.linear_out.weight,
                  self.linear_out.bias)
        if torch.is_grad_enabled() and self.training and (
                x.requires_grad or any(p.requires_grad for p in params)):
            track_steps(self)
            full = _ExpandFn.apply(x, *params, self)
            x = x.detach()
        else:
            _, _, full = _lib.seg_query(x, self._rec().rec, want_labels=False, want_full=True)
        out = full.view(*lead, -1)
        # provenance for SemanticHead.forward: the expanded features of these codes, so the
        # 2-D demo's head call on them (demo_utils/utils.py:228-232) runs the folded
        # stego / k-means kernel on the 64-d codes instead of library GEMMs on 768-d rows
        out._sd_expand = (x, self, module_key(self), out._version)
        return out
