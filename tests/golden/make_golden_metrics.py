"""Writes tests/golden/eval_metrics.npz: inputs and the reference's own outputs of
scenedino/common/metrics.py (compute_depth_metrics, compute_dino_metrics, compute_seg_metrics,
SegmentationMetric.compute), for tests/test_metrics.py.

    SCENEDINO_REF=<reference checkout> python tests/golden/make_golden_metrics.py

The reference module imports skimage, pulp and ignite at the top; none of the recorded functions
uses them, so stub modules stand in (a minimal ``Metric`` base class, identity decorators).  The
one pulp call, SegmentationMetric._calculate_pseudo_label_assignment, is replaced here by
``scipy.optimize.linear_sum_assignment`` on the square 19 x 19 case, where the program is a plain
assignment problem: that record pins the scatter and IoU arithmetic, not pulp's choice.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("SCENEDINO_REF", "")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_metrics.npz")


def _stub_modules():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class Metric:
        def __init__(self, output_transform=lambda x: x, device="cpu"):
            self._output_transform = output_transform
            self._device = torch.device(device)
            self.reset()

        def reset(self):
            pass

    class Engine:
        pass

    class NotComputableError(RuntimeError):
        pass

    def identity(fn):
        return fn

    sk = module("skimage")
    sk.metrics = module("skimage.metrics")
    module("pulp")
    ig = module("ignite")
    ig.engine = module("ignite.engine", Engine=Engine)
    ig.exceptions = module("ignite.exceptions", NotComputableError=NotComputableError)
    ig.metrics = module("ignite.metrics", Metric=Metric)
    ig.metrics.metric = module("ignite.metrics.metric", reinit__is_reduced=identity,
                               sync_all_reduce=lambda *names: identity)


def load_reference():
    _stub_modules()
    path = os.path.join(REF, "scenedino", "common", "metrics.py")
    spec = importlib.util.spec_from_file_location("_reference_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def depth_inputs(g):
    """(3, 1, 6, 10) f64: about 70 % of gt zero, predictions below 1e-3 and above 80, image 2 of
    gt all zero.  Values are float32-representable, so the f32 case reads the same numbers."""
    gt = torch.rand(3, 1, 6, 10, generator=g) * 60 + 2
    gt[torch.rand(3, 1, 6, 10, generator=g) < 0.7] = 0
    gt[2] = 0
    pred = gt * (0.6 + 0.9 * torch.rand(3, 1, 6, 10, generator=g)) + torch.rand(3, 1, 6, 10, generator=g)
    pred[0, 0, 0, :4] = torch.tensor([1e-5, 5e-4, 95.0, 300.0])
    pred[1, 0, 1, :2] = torch.tensor([-3.0, 81.0])
    gt[0, 0, 0, :4] = torch.tensor([0.5, 2.0, 70.0, 0.0])
    gt[1, 0, 1, :2] = torch.tensor([4.0, 79.0])
    return gt.float().double(), pred.float().double()


def dino_inputs(g):
    """n, v = 2, 3 on a 4 x 5 grid, C = 64, float32-representable; one prediction row zero."""
    pred = torch.randn(2, 3, 4, 5, 1, 64, generator=g)
    gt = torch.randn(2, 3, 4, 5, 64, generator=g) * 0.7 + 0.3 * pred.squeeze(-2)
    pred[1, 2, 3, 4] = 0
    down = 0.5 * pred + 0.1 * torch.randn(2, 3, 4, 5, 1, 64, generator=g)
    return pred.float(), gt.float(), down.float()


def seg_inputs(g, n_classes):
    """target (2, 12, 16) in -1..18, view-major predictions (2, 2, 12, 16) in 0..n_classes-1."""
    target = torch.randint(-1, 19, (2, 12, 16), generator=g)
    like = target.clamp_min(0).unsqueeze(1).expand(2, 2, 12, 16)
    out = {}
    for name in ("plain", "pseudo"):
        noise = torch.randint(0, n_classes, (2, 2, 12, 16), generator=g)
        keep = torch.rand(2, 2, 12, 16, generator=g) < 0.6
        out[name] = torch.where(keep, like % n_classes, noise)
    other = torch.randint(0, n_classes, (2, 2, 12, 16), generator=g)
    return target, out["plain"], out["pseudo"], other


def seg_data(target, plain, pseudo, other):
    return {"segmentation": {"target": target, "results": {
        "direct_cluster": {"segs_pred": plain},
        "stego_cluster": {"segs_pred": other, "pseudo_segs_pred": pseudo}}}}


def lsa_assignment(self, metric_matrix):
    from scipy.optimize import linear_sum_assignment
    costs = metric_matrix.cpu().numpy()
    assert costs.shape[0] == costs.shape[1]
    rows, cols = linear_sum_assignment(costs, maximize=True)
    assignment = torch.zeros(costs.shape[1], dtype=torch.int64)
    assignment[torch.as_tensor(cols)] = torch.as_tensor(rows)
    return assignment


def main():
    if not os.path.isdir(os.path.join(REF, "scenedino")):
        raise SystemExit("set SCENEDINO_REF to a checkout of the reference")
    ref = load_reference()
    g = torch.Generator().manual_seed(20240611)
    rec = {}

    gt, pred = depth_inputs(g)
    rec["depth_gt"], rec["depth_pred"] = gt.numpy(), pred.numpy()
    for tag, a, b, fn in (("depth64", gt, pred, None), ("depth32", gt.float(), pred.float(), None),
                          ("depthl2", gt[:2], pred[:2], ref.l2_scaling)):
        for k, val in ref.compute_depth_metrics(a.clone(), b.clone(), fn).items():
            rec[f"{tag}_{k}"] = val.numpy()

    dp, dg, dd = dino_inputs(g)
    rec["in_dino_pred"], rec["in_dino_gt"], rec["in_dino_down"] = dp.numpy(), dg.numpy(), dd.numpy()
    for tag, coarse in (("dino", {"dino_features": dp.double()}),
                        ("dinodown", {"dino_features": dp.double(),
                                      "dino_features_downsampled": dd.double()})):
        for k, val in ref.compute_dino_metrics({"dino_gt": dg.double(), "coarse": [coarse]}).items():
            rec[f"{tag}_{k}"] = val.numpy()

    for n_classes in (19, 27):
        for batch in (0, 1):
            tensors = seg_inputs(g, n_classes)
            for name, t in zip(("target", "plain", "pseudo", "other"), tensors):
                rec[f"seg{n_classes}_{batch}_{name}"] = t.numpy()
            for k, val in ref.compute_seg_metrics(seg_data(*tensors), n_classes, 19).items():
                rec[f"seg{n_classes}_{batch}_out_{k}"] = val.numpy()

    ref.SegmentationMetric._calculate_pseudo_label_assignment = lsa_assignment
    for tag, assign in (("agg0", False), ("agg1", True)):
        metric = ref.SegmentationMetric("seg", assign_pseudo=assign)
        for batch in (0, 1):
            metric.update({k: torch.from_numpy(rec[f"seg19_{batch}_out_{k}"])
                           for k in ("direct_cluster", "stego_cluster")})
        for k, val in metric.compute().items():
            rec[f"{tag}_{k}"] = val.numpy() if torch.is_tensor(val) else np.float64(val)

    np.savez_compressed(OUT, **rec)
    print(OUT, os.path.getsize(OUT), "bytes,", len(rec), "arrays")


if __name__ == "__main__":
    main()
