"""Evaluation metrics: the mirror of scenedino/common/metrics.py without ignite, skimage or pulp.

``compute_depth_metrics``, ``compute_dino_metrics`` and ``compute_seg_metrics`` each have two
routes.  The torch route works on any device and dtype and keeps the reference's operation
order; it is the oracle of the tests.  On a GPU, inside the domain stated per function, the
native route runs one fused kernel of include/sdhip_metrics.h (``sd_depth_metrics``,
``sd_dino_metrics``, ``sd_seg_confusion``) and reads nothing back to the host.

The aggregators (``DictMeanMetric``, ``SegmentationMetric``) are plain classes with ``reset()``,
``update(value)`` and ``compute()``; they accumulate on the device the values arrive on and read
the host in ``compute()`` only.  ``SegmentationMetric._calculate_pseudo_label_assignment`` solves
the reference's integer program with one ``scipy.optimize.linear_sum_assignment``.

Not mirrored: ``compute_occ_metrics``, ``compute_nvs_metrics``, ``FG_ARI``,
``ConcatenateMetric``.
"""
from __future__ import annotations

from typing import Callable

import torch
import torch.nn.functional as F

DEPTH_KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
_DEPTH_MAX_HW = 1 << 24
_MAX_GRID_Y = 65535


class NotComputableError(RuntimeError):
    """compute() before the first update() (ignite.exceptions.NotComputableError's role)."""


def _no_grad_needed(*tensors) -> bool:
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))


# ---------------------------------------------------------------------------
# depth
# ---------------------------------------------------------------------------
def median_scaling(depth_gt: torch.Tensor, depth_pred: torch.Tensor):
    """The reference's median_scaling (metrics.py:16-29) divides two ``torch.nanmedian`` named
    tuples and so raises TypeError on every call; there is no behaviour to mirror."""
    raise NotImplementedError(
        "scenedino_amd: median_scaling is not implemented: the reference's version raises "
        "TypeError (it divides two torch.nanmedian (values, indices) tuples); use l2_scaling")


def l2_scaling(depth_gt: torch.Tensor, depth_pred: torch.Tensor):
    """Least-squares scale and shift of the prediction onto the pixels with gt > 0
    (metrics.py:32-46), in torch ops (the mask compaction reads the host)."""
    valid = depth_gt > 0
    target = depth_gt[valid].unsqueeze(-1).to(torch.float32)
    picked = depth_pred[valid]
    basis = torch.stack((picked, torch.ones_like(picked)), dim=-1).to(torch.float32)
    coef = torch.linalg.lstsq(basis, target).solution.squeeze()
    return depth_pred * coef[0] + coef[1]


def _depth_metrics_torch(depth_gt, depth_pred):
    pred = torch.clamp(depth_pred, 1e-3, 80)
    valid = depth_gt != 0
    count = valid.to(torch.float).flatten(-2, -1).sum(dim=-1)

    def image_mean(term):
        return torch.where(valid, term, torch.zeros_like(term)).flatten(-2, -1).sum(dim=-1) / count

    ratio = torch.maximum(depth_gt / pred, pred / depth_gt)
    out = {}
    sq = (depth_gt - pred) ** 2
    out["abs_rel"] = image_mean(torch.abs(depth_gt - pred) / depth_gt) ** 0.5
    out["sq_rel"] = image_mean(sq / depth_gt) ** 0.5
    out["rmse"] = image_mean(sq) ** 0.5
    out["rmse_log"] = image_mean((torch.log(depth_gt) - torch.log(pred)) ** 2) ** 0.5
    for k, name in enumerate(("a1", "a2", "a3"), start=1):
        out[name] = image_mean((ratio < 1.25 ** k).to(torch.float))
    return out


def _row_view(t, rows):
    """t -> (rows, numel / rows) with contiguous, 16-byte aligned rows: a view where the strides
    allow it (the kernels take an image stride), else a copy."""
    hw = t.numel() // rows
    try:
        v = t.view(rows, hw)
    except RuntimeError:
        v = None
    if v is None or v.data_ptr() % 16 or (rows > 1 and v.stride(0) < hw) or \
            (hw > 1 and v.stride(1) != 1):
        v = t.reshape(rows, hw).clone(memory_format=torch.contiguous_format)
    return v


def _depth_native_ok(gt, pred) -> bool:
    if not (gt.is_cuda and pred.is_cuda and gt.device == pred.device):
        return False
    if gt.dtype != torch.float32 or pred.dtype != torch.float32 or gt.shape != pred.shape:
        return False
    if gt.dim() < 2 or gt.numel() == 0:
        return False
    hw = gt.shape[-2] * gt.shape[-1]
    return hw <= _DEPTH_MAX_HW and gt.numel() // hw <= _MAX_GRID_Y and _no_grad_needed(gt, pred)


def compute_depth_metrics(depth_gt: torch.Tensor, depth_pred: torch.Tensor,
                          scaling_fn: Callable[[torch.Tensor, torch.Tensor], torch.Tensor] | None = None,
                          native: bool | None = None):
    """The seven depth scores of metrics.py:49-113 per image: a dict of tensors of the leading
    shape, (n, 1) for (n, 1, h, w) inputs.  The prediction is clamped to [1e-3, 80], pixels with
    gt == 0 are left out, ``abs_rel`` and ``sq_rel`` are square roots of their means as the
    reference writes them, and an image without a valid pixel gives NaN.  ``scaling_fn`` runs in
    torch first.  native: None picks ``sd_depth_metrics`` for float32 tensors on a GPU (the
    prediction is taken as a strided view, e.g. ``depth[:, :1]``, without a copy); True demands
    it; False keeps the torch route."""
    if scaling_fn:
        depth_pred = scaling_fn(depth_gt, depth_pred)
    ok = _depth_native_ok(depth_gt, depth_pred)
    if native and not ok:
        raise ValueError("compute_depth_metrics: outside sd_depth_metrics's domain (float32 "
                         "(..., h, w) tensors of one shape on one GPU, h w <= 2^24)")
    if native is False or not ok:
        return _depth_metrics_torch(depth_gt, depth_pred)
    from .. import _lib
    lead = depth_gt.shape[:-2]
    rows = depth_gt.numel() // (depth_gt.shape[-2] * depth_gt.shape[-1])
    out = _lib.depth_metrics(_row_view(depth_gt, rows), _row_view(depth_pred, rows))
    return {k: out[:, i].reshape(lead) for i, k in enumerate(DEPTH_KEYS)}


# ---------------------------------------------------------------------------
# dino
# ---------------------------------------------------------------------------
def _dino_operands(data):
    gt = data["dino_gt"]
    coarse = data["coarse"][0]
    key = "dino_features_downsampled" if "dino_features_downsampled" in coarse else "dino_features"
    return coarse[key].squeeze(-2), gt


def _dino_keys(v):
    keys = ["l1", "l2", "cos_sim"]
    for i in range(v):
        keys += [f"l1_{i}", f"l2_{i}", f"cos_sim_{i}"]
    return keys


def _dino_metrics_torch(pred, gt):
    if pred.dtype != gt.dtype:
        common = torch.promote_types(pred.dtype, gt.dtype)
        pred, gt = pred.to(common), gt.to(common)
    l1 = F.l1_loss(pred, gt, reduction="none").mean(dim=(0, 2, 3, 4))
    l2 = F.mse_loss(pred, gt, reduction="none").mean(dim=(0, 2, 3, 4))
    cos = F.cosine_similarity(pred, gt, dim=-1).mean(dim=(0, 2, 3))
    out = {"l1": l1.mean().reshape(1), "l2": l2.mean().reshape(1), "cos_sim": cos.mean().reshape(1)}
    for i in range(l1.shape[0]):
        out[f"l1_{i}"], out[f"l2_{i}"], out[f"cos_sim_{i}"] = l1[i:i + 1], l2[i:i + 1], cos[i:i + 1]
    return out


def _dino_native_ok(pred, gt) -> bool:
    if not (pred.is_cuda and gt.is_cuda and pred.device == gt.device):
        return False
    if pred.dim() != 5 or pred.shape != gt.shape or gt.numel() == 0:
        return False
    if gt.dtype != torch.float32 or pred.dtype not in (torch.float32, torch.bfloat16):
        return False
    n, v, _, _, C = pred.shape
    if C % 64 or not 64 <= C <= 768 or v > 64 or n * v > _MAX_GRID_Y:
        return False
    return pred.is_contiguous() and gt.is_contiguous() and pred.data_ptr() % 16 == 0 and \
        gt.data_ptr() % 16 == 0 and _no_grad_needed(pred, gt)


def compute_dino_metrics(data, native: bool | None = None):
    """``l1``, ``l2``, ``cos_sim`` between ``data["coarse"][0]["dino_features"]`` (or
    ``dino_features_downsampled`` where present), (n, v, h, w, 1, C), and ``data["dino_gt"]``,
    (n, v, h, w, C), averaged per view (``l1_i`` ...) and over the views (metrics.py:195-215).
    Every value has shape (1,) on the data's device and keeps the operands' dtype (the
    reference's ``torch.tensor([x])`` gives the same through 3 + 3 v host reads).
    The native route (``sd_dino_metrics``: float32 or bfloat16 features against float32 targets,
    contiguous, C % 64 == 0, 64 <= C <= 768) returns views of one device result."""
    pred, gt = _dino_operands(data)
    ok = _dino_native_ok(pred, gt)
    if native and not ok:
        raise ValueError("compute_dino_metrics: outside sd_dino_metrics's domain (contiguous "
                         "(n, v, h, w, C) float32 / bfloat16 features and float32 targets on one "
                         "GPU, C % 64 == 0, 64 <= C <= 768)")
    if native is False or not ok:
        return _dino_metrics_torch(pred, gt)
    from .. import _lib
    n, v, h, w, C = pred.shape
    out = _lib.dino_metrics(pred.view(n, v, h * w, C), gt.view(n, v, h * w, C))
    res = {"l1": out[v, 0:1], "l2": out[v, 1:2], "cos_sim": out[v, 2:3]}
    for i in range(v):
        res[f"l1_{i}"], res[f"l2_{i}"], res[f"cos_sim_{i}"] = out[i, 0:1], out[i, 1:2], out[i, 2:3]
    return res


# ---------------------------------------------------------------------------
# stego, segmentation
# ---------------------------------------------------------------------------
def compute_stego_metrics(data):
    """The three mean-correlation entries of ``data["segmentation"]["stego_corr"]``, a dict or a
    ``StegoCorrMap`` (metrics.py:218-227)."""
    seg = data["segmentation"]
    if "stego_corr" not in seg:
        return {}
    corr = seg["stego_corr"]
    return {k: corr[k] for k in ("stego_self_corr", "stego_nn_corr", "stego_random_corr")}


class SegConfusion(dict):
    """compute_seg_metrics's result: result key -> (gt_classes, n_classes) int64 matrix.
    ``bad_labels`` is None (torch route: out-of-range labels fail inside bincount / reshape) or a
    0-dim int32 device tensor counting the pixels with a target >= gt_classes or a prediction
    outside [0, n_classes); ``SegmentationMetric.compute()`` raises on a non-zero count."""
    bad_labels = None


def _seg_prediction(result):
    return result["pseudo_segs_pred"] if "pseudo_segs_pred" in result else result["segs_pred"]


def _seg_metrics_torch(target, preds, n_classes, gt_classes):
    flat = target.flatten()
    keep = flat >= 0
    flat = flat[keep]
    out = SegConfusion()
    for key, pred in preds.items():
        picked = pred[:, 0].flatten()[keep]
        out[key] = torch.bincount(n_classes * flat + picked,
                                  minlength=n_classes * gt_classes).reshape(gt_classes, n_classes)
    return out


def _seg_native_ok(target, preds, n_classes, gt_classes) -> bool:
    from .._lib import SEG_MAX_BINS
    if not target.is_cuda or target.dtype != torch.int64 or target.numel() == 0 or not preds:
        return False
    if n_classes < 1 or gt_classes < 1 or n_classes * gt_classes > SEG_MAX_BINS:
        return False
    first = next(iter(preds.values()))
    if first.dim() < 3:
        return False
    n = first.shape[0]
    for p in preds.values():
        if p.dtype != torch.int64 or p.device != target.device or p.dim() < 3 or p.shape[0] != n:
            return False
        if p[:, 0].numel() != target.numel():
            return False
    return True


def compute_seg_metrics(data, n_classes, gt_classes, native: bool | None = None):
    """One (gt_classes, n_classes) int64 confusion matrix per key of
    ``data["segmentation"]["results"]`` (metrics.py:230-247): rows are the targets, columns the
    predictions (``pseudo_segs_pred`` where a result has it, else ``segs_pred``), view 0 only,
    pixels with a target < 0 dropped.  The native route (``sd_seg_confusion``: int64 labels on a
    GPU) reads the target once per 8 results, compacts nothing and returns the count of
    out-of-range labels on the device instead of failing (``SegConfusion.bad_labels``)."""
    seg = data["segmentation"]
    target = seg["target"]
    preds = {k: _seg_prediction(r) for k, r in seg["results"].items()}
    n_classes, gt_classes = int(n_classes), int(gt_classes)
    ok = _seg_native_ok(target, preds, n_classes, gt_classes)
    if native and not ok:
        raise ValueError("compute_seg_metrics: outside sd_seg_confusion's domain (int64 labels on "
                         "one GPU, gt_classes n_classes <= 8192)")
    if native is False or not ok:
        return _seg_metrics_torch(target, preds, n_classes, gt_classes)
    from .. import _lib
    keys = list(preds)
    n = preds[keys[0]].shape[0]
    tgt = _row_view(target.contiguous(), n)
    per = gt_classes * n_classes
    chunk = max(1, min(_lib.SEG_MAX_RESULTS, _lib.SEG_MAX_BINS // per))
    out = SegConfusion()
    bad = None
    for c0 in range(0, len(keys), chunk):
        part = keys[c0:c0 + chunk]
        views = [_row_view(preds[k][:, 0], n) for k in part]
        conf = _lib.seg_confusion(tgt, views, gt_classes, n_classes)
        mats = conf[:-1].view(len(part), gt_classes, n_classes).to(torch.int64)
        for i, k in enumerate(part):
            out[k] = mats[i]
        bad = conf[-1] if bad is None else bad + conf[-1]  # per launch: a bad target counts in each
    out.bad_labels = bad
    return out


# ---------------------------------------------------------------------------
# aggregators
# ---------------------------------------------------------------------------
class DictMeanMetric:
    """Mean over the updates of every entry of a dict of tensors (metrics.py:288-331): per key
    the running sum of ``metric.sum()``, kept on the metric's device; a value holding a NaN is
    left out by a device-side select (the reference tests it on the host and prints a warning).
    ``compute()`` returns ``{name_key: sum / updates}`` as Python floats."""

    def __init__(self, name: str, output_transform=lambda x: x["output"], device=None):
        self._name = name
        self._output_transform = output_transform
        self._device = device
        self.reset()

    def reset(self):
        self._sums = {}
        self._num_examples = 0

    def _place(self, t):
        return t if self._device is None else t.to(self._device)

    @torch.no_grad()
    def update(self, value):
        for key, metric in value.items():
            metric = self._place(torch.as_tensor(metric))
            total = metric.sum().to(torch.float32)
            if key not in self._sums:
                self._sums[key] = torch.zeros((), device=metric.device, dtype=torch.float32)
            acc = self._sums[key]
            self._sums[key] = torch.where(torch.isnan(metric).any(), acc, acc + total)
        self._num_examples += 1

    def compute(self):
        if self._num_examples == 0:
            raise NotComputableError(f"{type(self).__name__} {self._name}: compute() needs at "
                                     "least one update()")
        return {f"{self._name}_{key}": total.item() / self._num_examples
                for key, total in self._sums.items()}


# [road, sidewalk, building, wall, fence, pole, traffic light, traffic sign, vegetation, terrain,
#  sky, person, rider, car, truck, bus, train, motorcycle, bicycle]
_CLASS_WEIGHTS = (4, 2, 2, 1, 1, 1, 1, 1, 2, 2, 1, 1, 1, 2, 1, 1, 1, 1, 1)


def pseudo_label_assignment(metric_matrix):
    """The assignment of metrics.py:431-456 without pulp: every one of the n_classes columns of the
    (gt_classes, n_classes) matrix goes to exactly one row, every row gets at least one column,
    and the sum of the chosen entries is maximal.  One ``linear_sum_assignment`` on a square
    (n_classes, n_classes) matrix: the first gt_classes rows are the matrix (a column matched to
    row i takes i: the mandatory column of that row), the other n_classes - gt_classes rows each
    hold the column maxima (a column matched to one of them is free and takes its own argmax).
    Which of several optima comes out is SciPy's choice, not pulp's.  Returns (n_classes) int64."""
    import numpy as np
    from scipy.optimize import linear_sum_assignment

    costs = np.asarray(torch.as_tensor(metric_matrix).detach().cpu().numpy(), dtype=np.float64)
    gt_classes, n_classes = costs.shape
    if n_classes < gt_classes:
        raise ValueError(f"pseudo-label assignment: {n_classes} predicted classes cannot cover "
                         f"{gt_classes} target classes (the reference's program is infeasible)")
    best = costs.argmax(axis=0)
    square = np.concatenate([costs, np.broadcast_to(costs.max(axis=0), (n_classes - gt_classes,
                                                                        n_classes))], axis=0)
    rows, cols = linear_sum_assignment(square, maximize=True)
    assignment = torch.zeros(n_classes, dtype=torch.int64)
    for i, j in zip(rows.tolist(), cols.tolist()):
        assignment[j] = i if i < gt_classes else int(best[j])
    return assignment


class SegmentationMetric(DictMeanMetric):
    """Sum of the confusion matrices of ``compute_seg_metrics`` (int32, on their device) and the
    scores of metrics.py:398-429 per result key: ``_assignment`` (with ``assign_pseudo``),
    ``_per_class_iou``, ``_miou``, ``_weighted_miou`` (the 19 Cityscapes class weights; left out
    for any other number of target classes, where the reference's product does not broadcast),
    ``_acc`` and ``_confusion_matrix``."""

    def __init__(self, name: str, output_transform=lambda x: x["output"], device=None,
                 assign_pseudo=True):
        super().__init__(name, output_transform, device)
        self.assign_pseudo = assign_pseudo
        weights = torch.tensor(_CLASS_WEIGHTS, dtype=torch.float32)
        self.weights = weights / weights.mean()

    def reset(self):
        super().reset()
        self._bad_labels = None

    @torch.no_grad()
    def update(self, value):
        for key, metric in value.items():
            metric = self._place(metric)
            if key not in self._sums:
                self._sums[key] = torch.zeros(metric.shape, device=metric.device, dtype=torch.int32)
            self._sums[key] += metric
        bad = getattr(value, "bad_labels", None)
        if bad is not None:
            bad = self._place(bad)
            self._bad_labels = bad.clone() if self._bad_labels is None else self._bad_labels + bad
        self._num_examples += 1

    _calculate_pseudo_label_assignment = staticmethod(pseudo_label_assignment)

    def compute(self):
        if self._num_examples == 0:
            raise NotComputableError(f"SegmentationMetric {self._name}: compute() needs at least "
                                     "one update()")
        if self._bad_labels is not None and int(self._bad_labels.item()) != 0:
            raise ValueError(f"SegmentationMetric {self._name}: {int(self._bad_labels.item())} pixels "
                             "had a target >= gt_classes or a prediction outside [0, n_classes)")
        result = {}
        for key, total in self._sums.items():
            total = total.cpu()
            if self.assign_pseudo:
                assignment = self._calculate_pseudo_label_assignment(total)
                gt_classes = total.size(0)
                confusion = torch.zeros((gt_classes, gt_classes), dtype=total.dtype)
                confusion.scatter_add_(1, assignment.unsqueeze(0).expand(gt_classes, -1), total)
                result[key + "_assignment"] = assignment
            else:
                confusion = total
            hits = confusion.diag()
            union = confusion.sum(dim=1) + confusion.sum(dim=0) - hits
            iou = torch.where(union > 0, hits / union, torch.zeros_like(union))
            result[key + "_per_class_iou"] = iou
            result[key + "_miou"] = iou.mean().item()
            if iou.numel() == self.weights.numel():
                result[key + "_weighted_miou"] = (iou * self.weights).mean().item()
            result[key + "_acc"] = hits.sum().item() / confusion.sum().item()
            result[key + "_confusion_matrix"] = confusion
        return result
