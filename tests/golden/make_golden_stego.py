"""Writes tests/golden/stego_train.npz: two consecutive training steps of the reference's
SemanticHead.forward_training (scenedino/downstream_head/semantic_head.py:122-235) and
StegoLoss (scenedino/losses/stego_loss.py), on CPU, for modes "3d" and "2d".

    SCENEDINO_REF=<reference checkout> python tests/golden/make_golden_stego.py

The reference is imported as tests/golden/make_golden.py imports it (that file's stubs).  Its
SemanticHead.__init__ allocates on "cuda", so the head object is assembled here from the
reference's sub-modules and plain attributes, and the reference's own (unbound) methods run on
it.  Every dropout p is 0 and every randint draw is recorded.  Parameters and inputs come from
tests/_stego_oracle.py's seeded generators, which the tests call too, so the file holds results
only: the six correlations, both cluster losses, labels and their top-2 margins per step, the
reference StegoLoss total under the shipped weights and shifts (pointwise false and true), and
the gradients of the head parameters after the second step's backward (the three weight
matrices subsampled: rows [::16] of nonlinear_path.0, columns [::4] of the other two).
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402
import _stego_oracle as so  # noqa: E402

SUB = {"stego_head.linear_path.0.weight": (slice(None), slice(None, None, 4)),
       "stego_head.nonlinear_path.0.weight": (slice(None, None, 16), slice(None)),
       "stego_head.nonlinear_path.2.weight": (slice(None), slice(None, None, 4))}


def _assemble(sh, mode):
    a = so.HEAD_ARGS
    head = sh.SemanticHead.__new__(sh.SemanticHead)
    torch.nn.Module.__init__(head)
    head.n_classes, head.gt_classes = a["n_classes"], a["gt_classes"]
    head.input_dim, head.code_dim = a["input_dim"], a["code_dim"]
    head.knn_neighbors, head.mode, head.apply_crf = a["knn_neighbors"], mode, False
    head.buffer_size, head.buffer_idx, head.buffer_filled = a["buffer_size"], 0, 1
    head.dino_patch_buffer = torch.zeros(a["buffer_size"], a["patch_sample_size"], a["input_dim"])
    head.dino_gap_buffer = torch.zeros(a["buffer_size"], a["input_dim"])
    head.direct_cluster_head = sh.KMeansParamHead(a["n_classes"], a["gt_classes"], a["input_dim"])
    head.stego_head = sh.StegoClusterHead(a["input_dim"], a["code_dim"])
    head.stego_cluster_head = sh.KMeansParamHead(a["n_classes"], a["gt_classes"], a["code_dim"])
    head.direct_linear_head = sh.LinearHead(a["input_dim"], a["gt_classes"])
    head.stego_linear_head = sh.LinearHead(a["code_dim"], a["gt_classes"])
    head.label_colors = torch.zeros(a["gt_classes"] + 1, 3)
    head.dropout = torch.nn.Dropout2d(p=0.0)
    head.dropout1d = torch.nn.Dropout1d(p=0.0)
    for m in head.modules():
        if isinstance(m, (torch.nn.Dropout2d, torch.nn.Dropout1d)):
            m.p = 0.0
    head.load_state_dict(so.head_state(so.HEAD_SEEDS[mode]), strict=False)
    head.direct_cluster_head.centroids_initialized = True
    head.stego_cluster_head.centroids_initialized = True
    return head.train()


def _margins(x, centres):
    s = so.probe_xhat(x.reshape(-1, x.shape[-1])) @ torch.nn.functional.normalize(centres, dim=1).t()
    top = s.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]).detach()


def main():
    mg._install_stubs()
    _, sh = mg.load_reference_seg()
    # scenedino/losses/__init__.py imports the reconstruction loss (kornia): a bare package
    # module, as make_golden.py stubs scenedino.models
    losses = types.ModuleType("scenedino.losses")
    losses.__path__ = [os.path.join(mg.REF, "scenedino", "losses")]
    sys.modules["scenedino.losses"] = losses
    from scenedino.losses.stego_loss import StegoLoss
    out = {}
    for mode in ("3d", "2d"):
        seed = so.HEAD_SEEDS[mode]
        head = _assemble(sh, mode)
        draws = []
        orig = torch.randint

        def randint(*a, **kw):
            r = orig(*a, **kw)
            draws.append(r.clone())
            return r

        for step in range(2):
            data, nc = so.head_step_inputs(seed, step, mode)
            torch.manual_seed(100 * seed + step)
            del draws[:]
            torch.randint = randint
            try:
                data = head.forward_training(data, sample_factor=2 if mode == "2d" else 4)
            finally:
                torch.randint = orig
            assert len(draws) == 2 and draws[0].shape == (nc,)
            seg = data["segmentation"]
            t = f"{mode}_{step}_"
            out[t + "nn_pick"], out[t + "random_idx"] = draws[0].numpy(), draws[1].numpy()
            for k, c in seg["stego_corr"].items():
                out[t + k] = c.detach().numpy().copy()
            feats = torch.nn.functional.normalize(data["coarse"][0]["dino_features"], dim=-1, eps=1e-10)
            stego = head.stego_head(feats.squeeze(-2).flatten(0, 1)).detach()
            for name, x, ch in (("direct", feats, head.direct_cluster_head),
                                ("stego", stego, head.stego_cluster_head)):
                res = seg["results"][name + "_cluster"]
                mar = _margins(x, ch.cluster_centers)
                frac = float((mar > 2e-2).float().mean())
                assert frac >= 0.95, f"{mode} step {step} {name}: {frac:.3f} of the rows have a " \
                                     "margin over 2e-2; pick another seed"
                out[t + name + "_labels"] = res["pseudo_segs_pred"].numpy().astype(np.int16)
                out[t + name + "_margin"] = mar.numpy().astype(np.float32)
                out[t + name + "_loss"] = np.float32(res["loss"].item())
            total = StegoLoss(dict(so.STEGO_LOSS, pointwise=False))(data)["total_loss"]
            out[t + "total"] = np.float32(total.item())
            if step == 1:
                head.zero_grad(set_to_none=True)
                total.backward()
                for name, p in head.named_parameters():
                    if p.grad is not None:
                        g = p.grad.reshape(p.shape[0], -1) if p.dim() == 4 else p.grad
                        out[f"{mode}_grad_{name}"] = g[SUB[name]].numpy().copy() if name in SUB else g.numpy().copy()
            out[t + "total_pointwise"] = np.float32(
                StegoLoss(dict(so.STEGO_LOSS, pointwise=True))(data)["total_loss"].item())
    path = os.path.join(HERE, "stego_train.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
