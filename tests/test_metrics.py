"""CPU side of scenedino_amd/common/metrics.py: the torch route against the reference's own
outputs (tests/golden/eval_metrics.npz, written by tests/golden/make_golden_metrics.py), the
pulp-free pseudo-label assignment against brute force and against the LP bound of the reference's
constraints, the aggregators, the C ABI of include/sdhip_metrics.h and the drop-in switch."""
from __future__ import annotations

import ctypes
import importlib
import itertools
import os
import re
import sys
import textwrap

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

from scenedino_amd.common import metrics as M

F32_EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "eval_metrics.npz")) as z:
        return {k: z[k] for k in z.files}


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _close(got, want, rtol, what):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs"
    g, w = got[~nan].double(), want[~nan].double()
    assert bool(((g - w).abs() <= rtol * w.abs().clamp_min(1e-300)).all()), (what, g, w)


# ---------------------------------------------------------------------------------- golden
def test_depth_torch_route_matches_the_reference(golden):
    gt, pred = _t(golden["depth_gt"]), _t(golden["depth_pred"])
    assert gt.dtype == torch.float64 and float((gt == 0).float().mean()) > 0.6
    assert float(pred.min()) < 1e-3 and float(pred.max()) > 80 and not bool(gt[2].any())
    cases = (("depth64", gt, pred, None, 1e-12), ("depth32", gt.float(), pred.float(), None, 4 * F32_EPS),
             # l2_scaling solves its least-squares system in float32, as the reference does, and
             # LAPACK's last bits move with the thread count: float32 rounding of two
             # coefficients through a sum and a square root, not 1e-12
             ("depthl2", gt[:2], pred[:2], M.l2_scaling, 16 * F32_EPS))
    for tag, a, b, fn, rtol in cases:
        out = M.compute_depth_metrics(a.clone(), b.clone(), fn)
        assert tuple(out) == M.DEPTH_KEYS
        for k in M.DEPTH_KEYS:
            want = _t(golden[f"{tag}_{k}"])
            assert out[k].shape == a.shape[:2] and out[k].dtype == want.dtype, (tag, k)
            # the a-scores are float32 ratios of counts in the reference, for f64 inputs too
            _close(out[k], want, 0.0 if k in ("a1", "a2", "a3") else rtol, f"{tag} {k}")
    # the image without a valid pixel stays NaN in every score
    out = M.compute_depth_metrics(gt, pred, None)
    assert all(bool(torch.isnan(out[k][2]).all()) and not bool(torch.isnan(out[k][:2]).any())
               for k in M.DEPTH_KEYS)


def test_median_scaling_raises_and_says_why(golden):
    gt, pred = _t(golden["depth_gt"]), _t(golden["depth_pred"])
    with pytest.raises(NotImplementedError, match="TypeError"):
        M.compute_depth_metrics(gt, pred, M.median_scaling)


def test_dino_torch_route_matches_the_reference(golden):
    pred, gt, down = (_t(golden[k]).double() for k in ("in_dino_pred", "in_dino_gt", "in_dino_down"))
    assert pred.shape == (2, 3, 4, 5, 1, 64) and not bool(pred[1, 2, 3, 4].any())
    for tag, coarse in (("dino", {"dino_features": pred}),
                        ("dinodown", {"dino_features": pred, "dino_features_downsampled": down})):
        out = M.compute_dino_metrics({"dino_gt": gt, "coarse": [coarse]})
        want_keys = [k[len(tag) + 1:] for k in golden if k.startswith(tag + "_")]
        assert sorted(out) == sorted(want_keys) and len(out) == 3 + 3 * 3
        for k, val in out.items():
            assert val.shape == (1,) and val.dtype == torch.float64
            want = _t(golden[f"{tag}_{k}"])
            assert want.dtype == torch.float64
            _close(val, want, 1e-12, f"{tag} {k}")
    a = M.compute_dino_metrics({"dino_gt": gt, "coarse": [{"dino_features": pred}]})
    b = M.compute_dino_metrics({"dino_gt": gt, "coarse": [{"dino_features": pred,
                                                          "dino_features_downsampled": down}]})
    assert not torch.equal(a["l1"], b["l1"])


def _seg_data(golden, n_classes, batch, dev="cpu"):
    t = {k: _t(golden[f"seg{n_classes}_{batch}_{k}"]).to(dev) for k in ("target", "plain", "pseudo", "other")}
    return {"segmentation": {"target": t["target"], "results": {
        "direct_cluster": {"segs_pred": t["plain"]},
        "stego_cluster": {"segs_pred": t["other"], "pseudo_segs_pred": t["pseudo"]}}}}


def test_seg_torch_route_matches_the_reference(golden):
    for n_classes in (19, 27):
        for batch in (0, 1):
            data = _seg_data(golden, n_classes, batch)
            assert int(data["segmentation"]["target"].min()) == -1
            out = M.compute_seg_metrics(data, n_classes, 19)
            assert list(out) == ["direct_cluster", "stego_cluster"] and out.bad_labels is None
            for k, mat in out.items():
                want = _t(golden[f"seg{n_classes}_{batch}_out_{k}"])
                assert mat.dtype == torch.int64 and mat.shape == (19, n_classes)
                assert torch.equal(mat, want)
            # pseudo_segs_pred is preferred, and view 1 is not scored
            data["segmentation"]["results"]["stego_cluster"]["segs_pred"] = \
                torch.zeros_like(data["segmentation"]["results"]["stego_cluster"]["segs_pred"])
            data["segmentation"]["results"]["direct_cluster"]["segs_pred"][:, 1] = 0
            again = M.compute_seg_metrics(data, n_classes, 19)
            assert all(torch.equal(again[k], out[k]) for k in out)


def test_segmentation_metric_compute_matches_the_reference(golden):
    for tag, assign in (("agg0", False), ("agg1", True)):
        metric = M.SegmentationMetric("seg", assign_pseudo=assign)
        for batch in (0, 1):
            metric.update({k: _t(golden[f"seg19_{batch}_out_{k}"]) for k in ("direct_cluster", "stego_cluster")})
        out = metric.compute()
        want_keys = sorted(k[len(tag) + 1:] for k in golden if k.startswith(tag + "_"))
        assert sorted(out) == want_keys
        for k, val in out.items():
            want = golden[f"{tag}_{k}"]
            if torch.is_tensor(val) and not val.is_floating_point():
                assert torch.equal(val, _t(want)) and val.dtype == _t(want).dtype, k
            elif torch.is_tensor(val):
                assert val.dtype == torch.float32
                _close(val, _t(want), 0.0, k)
            else:
                assert isinstance(val, float) and val == float(want), k
        assert out["direct_cluster_confusion_matrix"].dtype == torch.int32


def test_stego_metrics_pass_through_a_corr_map():
    from scenedino_amd.downstream_head.semantic_head import StegoCorrMap
    assert M.compute_stego_metrics({"segmentation": {}}) == {}
    vals = {k: torch.tensor(float(i)) for i, k in enumerate(
        ("stego_self_corr", "stego_nn_corr", "stego_random_corr", "dino_self_corr"))}
    out = M.compute_stego_metrics({"segmentation": {"stego_corr": vals}})
    assert list(out) == ["stego_self_corr", "stego_nn_corr", "stego_random_corr"]
    assert all(out[k] is vals[k] for k in out)
    g = torch.Generator().manual_seed(0)
    dino = [torch.randn(2, 5, 16, generator=g) for _ in range(3)]
    stego = [torch.randn(2, 5, 8, generator=g) for _ in range(3)]
    built = []

    def corr(a, b):
        built.append(1)
        return torch.einsum("npc,nqc->npq", a, b)

    cmap = StegoCorrMap(dino, stego, corr)
    out = M.compute_stego_metrics({"segmentation": {"stego_corr": cmap}})
    assert list(out) == ["stego_self_corr", "stego_nn_corr", "stego_random_corr"]
    for k in out:
        assert torch.equal(out[k], cmap[k])
    assert len(built) == 3  # the DINO correlations were never built


# ------------------------------------------------------------------------------ assignment
def _feasible(assignment, gt, n):
    a = assignment.tolist()
    return len(a) == n and all(0 <= i < gt for i in a) and set(a) == set(range(gt))


def _objective(costs, assignment):
    return int(sum(int(costs[i, j]) for j, i in enumerate(assignment.tolist())))


def _brute_force(costs):
    gt, n = costs.shape
    best = None
    for a in itertools.product(range(gt), repeat=n):
        if len(set(a)) == gt:
            s = sum(int(costs[i, j]) for j, i in enumerate(a))
            best = s if best is None or s > best else best
    return best


def test_assignment_equals_brute_force_on_small_matrices():
    g = torch.Generator().manual_seed(5)
    n_cases = 0
    for gt in (2, 3, 4):
        for n in range(gt, gt + 4):
            for trial in range(8):
                # tied: few distinct values, so optima are not unique; untied: large distinct ones
                hi = 3 if trial % 2 else 10 ** 6
                costs = torch.randint(0, hi, (gt, n), generator=g, dtype=torch.int32)
                a = M.pseudo_label_assignment(costs)
                assert a.dtype == torch.int64 and _feasible(a, gt, n), (costs, a)
                assert _objective(costs, a) == _brute_force(costs.numpy()), (costs, a)
                n_cases += 1
    assert n_cases == 96
    # the method of the aggregator is the same function
    costs = torch.tensor([[5, 1, 0], [4, 9, 9]], dtype=torch.int32)
    a = M.SegmentationMetric("seg")._calculate_pseudo_label_assignment(costs)
    assert a.tolist() == [0, 1, 1]


def test_assignment_is_optimal_at_19_by_27():
    """Feasible, and its objective equals the optimum of the LP relaxation of the reference's own
    program (every column sums to 1, every row to >= 1, 0 <= x <= 1): the LP optimum bounds the
    integer optimum from above, so equality proves optimality."""
    from scipy.optimize import linprog
    gt, n = 19, 27
    g = torch.Generator().manual_seed(9)
    a_eq = np.zeros((n, gt * n))
    a_ub = np.zeros((gt, gt * n))
    for i in range(gt):
        for j in range(n):
            a_eq[j, i * n + j] = 1.0
            a_ub[i, i * n + j] = -1.0
    for trial in range(4):
        costs = torch.randint(0, 5000, (gt, n), generator=g, dtype=torch.int32)
        if trial % 2:  # a confusion matrix with a strong diagonal and empty classes
            costs = costs // 50
            costs[torch.arange(gt), torch.arange(gt)] += 4000
            costs[:, 20:] = 0
        a = M.pseudo_label_assignment(costs)
        assert _feasible(a, gt, n)
        lp = linprog(-costs.numpy().astype(np.float64).reshape(-1), A_ub=a_ub, b_ub=-np.ones(gt),
                     A_eq=a_eq, b_eq=np.ones(n), bounds=(0, 1), method="highs")
        assert lp.status == 0
        assert abs(-lp.fun - _objective(costs, a)) <= 1e-6 * max(1.0, -lp.fun), (trial, -lp.fun)


def test_assignment_with_fewer_columns_than_rows_raises():
    with pytest.raises(ValueError, match="infeasible"):
        M.pseudo_label_assignment(torch.ones(4, 3, dtype=torch.int32))


# ------------------------------------------------------------------------------ aggregators
def test_dict_mean_metric_skips_nan_values():
    metric = M.DictMeanMetric("depth")
    with pytest.raises(M.NotComputableError):
        metric.compute()
    metric.update({"a": torch.tensor([[1.0], [3.0]]), "b": torch.tensor([2.0])})
    metric.update({"a": torch.tensor([[float("nan")], [5.0]]), "b": torch.tensor([4.0])})
    metric.update({"a": torch.tensor([[2.0], [2.0]]), "b": torch.tensor([float("nan")])})
    out = metric.compute()
    # sums of metric.sum() over the updates without a NaN, over the number of updates
    assert out == {"depth_a": (4.0 + 4.0) / 3, "depth_b": (2.0 + 4.0) / 3}
    metric.reset()
    metric.update({"a": torch.tensor([7.0])})
    assert metric.compute() == {"depth_a": 7.0}


def test_segmentation_metric_feeds_update_model_eval(golden):
    import _stego_oracle as so
    from scenedino_amd.downstream_head.semantic_head import SemanticHead
    metric = M.SegmentationMetric("seg", assign_pseudo=True)
    metric.update(M.compute_seg_metrics(_seg_data(golden, 19, 0), 19, 19))
    metric.update(M.compute_seg_metrics(_seg_data(golden, 19, 1), 19, 19))
    out = metric.compute()
    head = SemanticHead(**so.HEAD_ARGS)
    head.update_model_eval(out)
    assert torch.equal(head.direct_cluster_head.pseudo_assignment, out["direct_cluster_assignment"])
    assert torch.equal(head.stego_cluster_head.pseudo_assignment, out["stego_cluster_assignment"])
    assert sorted(out["direct_cluster_assignment"].tolist()) == list(range(19))
    # a bad-label count that came with the matrices surfaces in compute()
    bad = M.SegConfusion({"k": torch.zeros(3, 3, dtype=torch.int64)})
    bad.bad_labels = torch.tensor(2, dtype=torch.int32)
    metric = M.SegmentationMetric("seg", assign_pseudo=False)
    metric.update(bad)
    with pytest.raises(ValueError, match="2 pixels"):
        metric.compute()


# -------------------------------------------------------------------------------------- ABI
def _header_functions():
    src = open(os.path.join(ROOT, "include", "sdhip_metrics.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sd_[a-z_0-9]+)\s*\(", src)))


def test_header_functions_are_exported_and_bound():
    from scenedino_amd import _lib, build
    lib = _lib.load()
    names = _header_functions()
    assert names == ["sd_depth_metrics", "sd_depth_metrics_work", "sd_dino_metrics",
                     "sd_dino_metrics_work", "sd_seg_confusion"]
    for name in names:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert "csrc/sdhip_metrics.hip" in build.SOURCES
    assert "../include/sdhip_metrics.h" in build.HEADERS


def test_struct_layout_matches_the_header(tmp_path):
    import subprocess
    from scenedino_amd import _lib
    py = _lib.SdSegConfusionArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sdhip_metrics.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(sd_seg_confusion_args));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(sd_seg_confusion_args, {fname}));')
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o",
                    str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.strip().split("\n"))
    assert ctypes.sizeof(py) == int(got["size"])
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == int(got[fname]), fname


def test_out_of_domain_arguments_return_an_error_without_a_gpu():
    from scenedino_amd import _lib
    lib = _lib.load()
    p = 4096  # a 16-byte aligned non-null address; validation never dereferences it
    # depth
    assert lib.sd_depth_metrics(None, 4, None, 4, 1, 4, None, None, None) == -1
    assert b"sd_depth_metrics" in lib.sd_last_error()
    assert lib.sd_depth_metrics(p, 3, p, 4, 1, 4, p, p, None) == -1      # image stride < hw
    assert lib.sd_depth_metrics(p, 4, p + 4, 4, 1, 4, p, p, None) == -1  # misaligned
    assert lib.sd_depth_metrics(p, 4, p, 4, 0, 4, p, p, None) == -1
    assert lib.sd_depth_metrics_work(1, 0) == -1 and lib.sd_depth_metrics_work(1, (1 << 24) + 1) == -1
    assert lib.sd_depth_metrics_work(3, 2049) == 3 * 2 * 8 * 8
    # dino: C = 100, C = 832, a null pointer, an f16 prediction
    assert lib.sd_dino_metrics(p, _lib.SD_F32, p, 1, 1, 4, 100, p, p, None) == -1
    assert b"C % 64" in lib.sd_last_error()
    assert lib.sd_dino_metrics(p, _lib.SD_F32, p, 1, 1, 4, 832, p, p, None) == -1
    assert lib.sd_dino_metrics(p, _lib.SD_F32, None, 1, 1, 4, 64, p, p, None) == -1
    assert lib.sd_dino_metrics(p, _lib.SD_F16, p, 1, 1, 4, 64, p, p, None) == -1
    assert lib.sd_dino_metrics(p, _lib.SD_F32, p, 1, 65, 4, 64, p, p, None) == -1
    assert lib.sd_dino_metrics_work(1, 1, 4, 100) == -1
    assert lib.sd_dino_metrics_work(2, 3, 67, 64) == 2 * 3 * 5 * 3 * 8
    # seg: R = 9, too many bins, null pointers
    def seg(**kw):
        a = _lib.SdSegConfusionArgs(target=p, n=1, hw=4, n_results=1, gt_classes=19, n_classes=19, conf=p)
        a.pred[0], a.pred_stride[0] = p, 4
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.sd_seg_confusion(ctypes.byref(a), None)
    assert seg(n_results=9) == -1 and b"sd_seg_confusion" in lib.sd_last_error()
    assert seg(gt_classes=91, n_classes=91) == -1          # 8281 bins
    assert seg(n_results=2) == -1                          # the second prediction is NULL
    assert seg(target=None) == -1 and seg(conf=None) == -1
    assert seg(hw=5) == -1                                 # prediction stride < hw
    assert lib.sd_seg_confusion(None, None) == -1


# ----------------------------------------------------------------------------------- drop-in
_REFERENCE_METRICS = textwrap.dedent("""
    def compute_depth_metrics(depth_gt, depth_pred, scaling_fn):
        return 'reference depth'
    def compute_dino_metrics(data):
        return 'reference dino'
    def compute_seg_metrics(data, n_classes, gt_classes):
        return 'reference seg'
    def compute_stego_metrics(data):
        return 'reference stego'
    def compute_nvs_metrics(data, lpips):
        return 'reference nvs'
    class SegmentationMetric:
        def _calculate_pseudo_label_assignment(self, metric_matrix):
            return 'reference pulp'
    """)


@pytest.fixture
def fake_reference(tmp_path, monkeypatch):
    """A stand-in ``scenedino`` checkout (the pattern of tests/test_crop3d.py) whose
    common/metrics.py imports; a test that wants the other case rewrites that file."""
    root = tmp_path / "ref"
    files = {
        "scenedino/__init__.py": "",
        "scenedino/renderer/__init__.py": "from .nerf import NeRFRenderer\n",
        "scenedino/renderer/nerf.py": "class NeRFRenderer:\n    origin = 'reference'\n",
        "scenedino/models/__init__.py": "def make_model(config, downstream_config=None):\n    return 0\n",
        "scenedino/models/bts.py": "class BTSNet:\n    origin = 'reference'\n",
        "scenedino/common/__init__.py": "",
        "scenedino/common/ray_sampler.py": "class ImageRaySampler:\n    origin = 'reference'\n",
        "scenedino/common/metrics.py": _REFERENCE_METRICS,
    }
    for rel, txt in files.items():
        f = root / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(txt)
    saved = {k: v for k, v in sys.modules.items() if k == "scenedino" or k.startswith("scenedino.")}
    for k in saved:
        del sys.modules[k]
    monkeypatch.syspath_prepend(str(root))
    yield root
    for k in [k for k in sys.modules if k == "scenedino" or k.startswith("scenedino.")]:
        del sys.modules[k]
    sys.modules.update(saved)


def test_install_default_leaves_the_reference_metrics(fake_reference):
    import inspect
    from scenedino_amd import dropin
    assert inspect.signature(dropin.install).parameters["native_metrics"].default is False
    dropin.install()
    cm = importlib.import_module("scenedino.common.metrics")
    assert cm.compute_depth_metrics(None, None, None) == "reference depth"
    assert cm.SegmentationMetric()._calculate_pseudo_label_assignment(None) == "reference pulp"


def test_install_native_metrics_replaces_the_functions(fake_reference):
    from scenedino_amd import dropin
    dropin.install(native_metrics=True)
    cm = importlib.import_module("scenedino.common.metrics")
    for name in ("compute_depth_metrics", "compute_dino_metrics", "compute_seg_metrics",
                 "compute_stego_metrics"):
        assert getattr(cm, name) is getattr(M, name)
    assert cm.compute_nvs_metrics(None, None) == "reference nvs"  # out of scope: left alone
    costs = torch.tensor([[5, 1, 0], [4, 9, 9]], dtype=torch.int32)
    assert cm.SegmentationMetric()._calculate_pseudo_label_assignment(costs).tolist() == [0, 1, 1]


def test_install_native_metrics_registers_a_module_when_the_reference_does_not_import(fake_reference):
    (fake_reference / "scenedino" / "common" / "metrics.py").write_text(
        "import a_module_that_is_not_installed\n" + _REFERENCE_METRICS)
    from scenedino_amd import dropin
    dropin.install(native_metrics=True)
    cm = importlib.import_module("scenedino.common.metrics")
    from scenedino.common import metrics as again
    assert again is cm
    for name in ("compute_depth_metrics", "compute_dino_metrics", "compute_seg_metrics",
                 "compute_stego_metrics", "l2_scaling", "median_scaling", "DictMeanMetric",
                 "SegmentationMetric"):
        assert getattr(cm, name) is getattr(M, name)
    gt = torch.tensor([[[[2.0, 0.0]]]])
    out = cm.compute_depth_metrics(gt, gt.clone() + 1, None)
    assert out["rmse"].shape == (1, 1) and float(out["rmse"]) == 1.0


def test_install_without_the_switch_does_not_register_a_module(fake_reference):
    (fake_reference / "scenedino" / "common" / "metrics.py").write_text(
        "import a_module_that_is_not_installed\n")
    from scenedino_amd import dropin
    dropin.install()
    assert "scenedino.common.metrics" not in sys.modules
    with pytest.raises(ImportError):
        importlib.import_module("scenedino.common.metrics")
