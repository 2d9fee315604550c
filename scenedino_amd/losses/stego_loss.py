"""STEGO correlation loss of the downstream stage.

Mirror of scenedino/losses/stego_loss.py:6-79 (same config keys, ``pointwise``,
``get_loss_metric_names`` and result keys), so ``train_semantic_kitti_360`` runs on this package
alone.  It reads ``data["segmentation"]["stego_corr"]`` and ``["results"]`` as
``SemanticHead.forward_training`` leaves them; the correlation tensors are small, so this is
torch ops.
"""
from __future__ import annotations

import torch


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

    def __call__(self, data) -> dict[str, torch.Tensor]:
        seg = data["segmentation"]
        if "stego_corr" not in seg:
            self_loss, knn_loss, random_loss, total = 0, 0, 0, 0
        else:
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
