"""STEGO correlation loss of the downstream stage.

Mirror of scenedino/losses/stego_loss.py:6-79 (same config keys, ``pointwise``,
``get_loss_metric_names`` and result keys), so ``train_semantic_kitti_360`` runs on this package
alone.  It reads ``data["segmentation"]["stego_corr"]`` and ``["results"]`` as
``SemanticHead.forward_training`` leaves them.

Two routes compute the three correlation losses:

* the torch route reduces the six (nc, P, P) correlation tensors with element-wise ops, as the
  reference does (in-place row-mean removal included); it takes the eager dict or, by indexing,
  a ``StegoCorrMap``, on any device;
* the fused route (``sd_stego_corr_fwd`` / ``_bwd``, csrc/sdhip_stego_corr.hip; one autograd node
  whose inputs are the three un-normalised code row sets) is taken when ``stego_corr`` is a
  ``StegoCorrMap`` (``SemanticHead.lazy_corr``) of GPU tensors inside ``fused_domain``: D and S
  tiles are recomputed on bf16 MFMA and no correlation tensor is ever written.  With
  ``pointwise`` the centring is the factored form D - A^ . mean_q B^ + mean of that, which equals
  the reference's op sequence in exact arithmetic.

The four cluster / probe losses are torch ops on either route.
"""
from __future__ import annotations

import torch


class _FusedStegoCorr(torch.autograd.Function):
    """One node: forward sd_stego_corr_fwd -> (3) = [self, knn, random] losses, backward
    sd_stego_corr_bwd -> gradients of the three code row sets."""

    @staticmethod
    def forward(ctx, stego_self, stego_nn, stego_random, dino, weights, shifts, pointwise):
        from .. import _lib
        partners = [(None, None), (dino[1], stego_nn), (dino[2], stego_random)]
        loss, work = _lib.stego_corr_fwd(dino[0], stego_self, partners, weights, shifts, pointwise)
        ctx.cfg = (weights, shifts, pointwise)
        n = ctx.needs_input_grad
        ctx.need = (n[0], False, n[1], n[2])  # stego_a, then one flag per pair
        ctx.save_for_backward(stego_self, stego_nn, stego_random, *dino, work)
        return loss

    @staticmethod
    def backward(ctx, up):
        from .. import _lib
        s_self, s_nn, s_rnd, d0, d1, d2, work = ctx.saved_tensors
        weights, shifts, pointwise = ctx.cfg
        up = up if up.dtype == torch.float32 and up.is_contiguous() else up.float().contiguous()
        partners = [(None, None), (d1, s_nn), (d2, s_rnd)]
        d_a, d_b = _lib.stego_corr_bwd(up, d0, s_self, partners, weights, shifts, pointwise, work,
                                       ctx.need)
        return d_a, d_b[1], d_b[2], None, None, None, None


class StegoLoss:
    def __init__(self, config) -> None:
        g = config.get
        self.random_weight = g("random_weight", 1.0)
        self.knn_weight = g("knn_weight", 1.0)
        self.self_weight = g("self_weight", 1.0)
        self.random_shift = g("random_shift", 0.0)
        self.knn_shift = g("knn_shift", 0.0)
        self.self_shift = g("self_shift", 0.0)
        self.pointwise = g("pointwise", True)
        self.fused = True         # False: always the torch route
        self.last_route = None    # "fused" / "torch": the route of the latest call with stego_corr

    def get_loss_metric_names(self) -> list[str]:
        return ["total_loss", "self_loss", "knn_loss", "random_loss", "direct_cluster_loss",
                "direct_linear_loss", "stego_cluster_loss", "stego_linear_loss"]

    def _compute_stego_loss(self, dino_corr, stego_corr, weight, shift):
        if self.pointwise:
            # stego_loss.py:72-75: the row means are removed in place, as the reference does
            old_mean = dino_corr.mean()
            dino_corr -= dino_corr.mean(dim=-1, keepdim=True)
            dino_corr = dino_corr - dino_corr.mean() + old_mean
        return (-weight * stego_corr.clamp(0) * (dino_corr - shift)).mean()

    @staticmethod
    def fused_domain(c):
        """None if the correlation entry ``c`` can take the fused route, else the reason."""
        from ..downstream_head.semantic_head import StegoCorrMap
        if not isinstance(c, StegoCorrMap):
            return "stego_corr is not a StegoCorrMap (SemanticHead.lazy_corr)"
        rows = c.dino + c.stego
        if any(not torch.is_tensor(t) or t.device.type != "cuda" or t.dim() != 3 for t in rows):
            return "operand rows are not (nc, P, c) device tensors"
        nc, P, d = c.dino[0].shape
        if d not in (384, 768) or not 1 <= P <= 4096 or nc < 1 or nc * P > 1 << 24:
            return "shape outside d in (384, 768), 1 <= P <= 4096"
        if any(t.dtype != c.dino[0].dtype or tuple(t.shape) != (nc, P, d) for t in c.dino) \
                or c.dino[0].dtype not in (torch.float32, torch.bfloat16):
            return "DINO rows are not f32 / bf16 of one shape"
        if any(t.dtype != torch.float32 or tuple(t.shape) != (nc, P, 64) for t in c.stego):
            return "code rows are not f32 (nc, P, 64)"
        return None

    def _fused(self, c):
        dino = tuple(t.detach().contiguous() for t in c.dino)
        stego = tuple(t.contiguous() for t in c.stego)
        loss = _FusedStegoCorr.apply(
            *stego, dino, (float(self.self_weight), float(self.knn_weight), float(self.random_weight)),
            (float(self.self_shift), float(self.knn_shift), float(self.random_shift)),
            bool(self.pointwise))
        return loss[0], loss[1], loss[2]

    def __call__(self, data) -> dict[str, torch.Tensor]:
        seg = data["segmentation"]
        if "stego_corr" not in seg:
            self_loss, knn_loss, random_loss, total = 0, 0, 0, 0
        elif self.fused and self.fused_domain(seg["stego_corr"]) is None:
            self.last_route = "fused"
            self_loss, knn_loss, random_loss = self._fused(seg["stego_corr"])
            total = self_loss + knn_loss + random_loss
        else:
            self.last_route = "torch"
            c = seg["stego_corr"]
            self_loss = self._compute_stego_loss(c["dino_self_corr"], c["stego_self_corr"],
                                                 self.self_weight, self.self_shift)
            knn_loss = self._compute_stego_loss(c["dino_nn_corr"], c["stego_nn_corr"],
                                                self.knn_weight, self.knn_shift)
            random_loss = self._compute_stego_loss(c["dino_random_corr"], c["stego_random_corr"],
                                                   self.random_weight, self.random_shift)
            total = self_loss + knn_loss + random_loss
        res = seg["results"]
        direct_cluster = res["direct_cluster"].get("loss", 0.0)
        stego_cluster = res["stego_cluster"].get("loss", 0.0)
        direct_linear = res.get("direct_linear", {}).get("loss", 0.0)
        stego_linear = res.get("stego_linear", {}).get("loss", 0.0)
        total = total + direct_cluster + direct_linear + stego_cluster + stego_linear
        return {"total_loss": total, "self_loss": self_loss, "knn_loss": knn_loss,
                "random_loss": random_loss, "direct_cluster_loss": direct_cluster,
                "direct_linear_loss": direct_linear, "stego_cluster_loss": stego_cluster,
                "stego_linear_loss": stego_linear}
