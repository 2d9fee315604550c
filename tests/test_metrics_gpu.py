"""sd_depth_metrics, sd_dino_metrics and sd_seg_confusion (csrc/sdhip_metrics.hip) on the GPU,
through scenedino_amd/common/metrics.py, against that module's torch route.

Floating-point outputs follow the project's 2x convention (tests/test_msc_gt_gpu.py): the oracle
is the torch route in f64 (on the CPU, computed once per case), the yardstick the torch route in
f32 on the GPU on the same input, and the native result must lie within twice the yardstick's own
error, with a floor of 4 x 2^-23 relative to the oracle's value (a yardstick that happens to round
to the oracle exactly would otherwise allow nothing).  Integer outputs (the threshold counts, the
valid count, every confusion matrix) are exact.
"""
from __future__ import annotations

import functools
import importlib
import sys

import pytest
import torch

from scenedino_amd.common import metrics as M

FLOOR = 4 * 2.0 ** -23
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _within(native, f64, f32, what):
    """|native - f64| <= max(2 |f32 - f64|, FLOOR |f64|) per element; NaNs where the oracle's are."""
    native, f64, f32 = (t.detach().double().cpu().reshape(-1) for t in (native, f64, f32))
    nan = torch.isnan(f64)
    assert torch.equal(torch.isnan(native), nan), f"{what}: NaN pattern differs from the oracle's"
    err_n, err_t = (native - f64).abs()[~nan], (f32 - f64).abs()[~nan]
    bound = torch.maximum(2 * err_t, FLOOR * f64.abs()[~nan])
    print(f"{what}: native error {float(err_n.max()) if err_n.numel() else 0.0:.3e}, f32 torch error "
          f"{float(err_t.max()) if err_t.numel() else 0.0:.3e}, bound {float(bound.min()) if bound.numel() else 0.0:.3e}")
    assert bool((err_n <= bound).all()), (what, native, f64, f32)


# ------------------------------------------------------------------------------------ depth
DEPTH_HW = {1: (1, 1), 257: (1, 257), 1920: (24, 80), 5000: (50, 100), 192 * 640: (192, 640)}


@functools.lru_cache(maxsize=None)
def _depth_case(hw, n):
    """gt (n, 1, h, w) with about half of the pixels zero, the prediction as view 0 of a two-view
    (n, 2, h, w) tensor, predictions below 1e-3 and above 80 on valid pixels, and for n = 3 image
    1 without a valid pixel.  No max(gt / pred, pred / gt) lies within 1e-5 relative of a
    threshold (such pixels are made invalid, and the condition is asserted)."""
    h, w = DEPTH_HW[hw]
    g = torch.Generator().manual_seed(1000 * n + hw % 997)
    gt = torch.rand(n, 1, h, w, generator=g) * 70 + 1
    gt[torch.rand(n, 1, h, w, generator=g) < 0.5] = 0
    gt.view(n, -1)[:, 0] = 7.0 + torch.arange(n)  # every image has a valid pixel (but see n = 3)
    both = gt.expand(n, 2, h, w) * (0.5 + 1.8 * torch.rand(n, 2, h, w, generator=g))
    flat = both.view(n, 2, -1)
    if hw >= 257:
        gt.view(n, -1)[0, 1:5] = torch.tensor([3.0, 5.0, 60.0, 75.0])
        flat[0, 0, 1:5] = torch.tensor([1e-5, -2.0, 90.0, 400.0])
    if n == 3:
        gt[1] = 0
    pred = both[:, :1]
    ratio = torch.maximum(gt.double() / pred.double().clamp(1e-3, 80),
                          pred.double().clamp(1e-3, 80) / gt.double())
    for t in THRESHOLDS:
        gt[((ratio / t - 1).abs() < 1e-4) & (gt != 0)] = 0
    ratio = torch.maximum(gt.double() / pred.double().clamp(1e-3, 80),
                          pred.double().clamp(1e-3, 80) / gt.double())
    valid = gt != 0
    assert all(bool((((ratio / t - 1).abs() >= 1e-5) | ~valid).all()) for t in THRESHOLDS)
    counts = torch.stack([((ratio < t) & valid).flatten(1).sum(1) for t in THRESHOLDS]
                         + [valid.flatten(1).sum(1)], dim=1)
    oracle = M.compute_depth_metrics(gt.double(), pred.double(), None)
    return gt, both, counts, oracle


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", sorted(DEPTH_HW))
def test_depth_metrics(gpu, hw, n):
    from scenedino_amd import _lib
    gt, both, counts, oracle = _depth_case(hw, n)
    gt_d, both_d = gt.to(gpu), both.to(gpu)
    pred_d = both_d[:, :1]
    assert not pred_d.is_contiguous() or n == 1
    f32 = M.compute_depth_metrics(gt_d, pred_d, None, native=False)
    out = M.compute_depth_metrics(gt_d, pred_d, None, native=True)
    assert tuple(out) == M.DEPTH_KEYS
    for k in M.DEPTH_KEYS:
        assert out[k].shape == (n, 1) and out[k].dtype == torch.float32 and out[k].is_cuda
        _within(out[k], oracle[k], f32[k], f"depth hw={hw} n={n} {k}")
    raw = _lib.depth_metrics(gt_d.view(n, hw), both_d.view(n, 2, hw)[:, 0])
    assert raw.shape == (n, 8) and torch.equal(
        raw[:, :7].contiguous().view(torch.int32),
        torch.stack([out[k].view(n) for k in M.DEPTH_KEYS], dim=1).view(torch.int32))
    raw = raw.cpu()
    assert torch.equal(raw[:, 7].long(), counts[:, 3])  # the valid count, exact
    for i, k in enumerate(("a1", "a2", "a3")):
        got = (raw[:, 4 + i].double() * raw[:, 7].double())
        ok = counts[:, 3] > 0
        assert torch.equal(torch.round(got[ok]).long(), counts[ok, i]), (k, got, counts)
        assert bool(((got[ok] - counts[ok, i]).abs() < 0.05).all())
    if n == 3:  # the image without a valid pixel: NaN where the torch route's is, count 0
        assert int(raw[1, 7]) == 0 and bool(torch.isnan(raw[1, :7]).all())
        assert all(bool(torch.isnan(f32[k][1]).all()) for k in M.DEPTH_KEYS)
        assert not bool(torch.isnan(raw[0]).any()) and not bool(torch.isnan(raw[2]).any())


@pytest.mark.gpu
def test_depth_scaling_runs_in_torch_first(gpu):
    gt, both, _, _ = _depth_case(1920, 1)
    gt_d, pred_d = gt.to(gpu), both.to(gpu)[:, :1]
    out = M.compute_depth_metrics(gt_d, pred_d, M.l2_scaling)
    f32 = M.compute_depth_metrics(gt_d, pred_d, M.l2_scaling, native=False)
    scaled = M.l2_scaling(gt_d, pred_d)
    oracle = M.compute_depth_metrics(gt.double(), scaled.double().cpu(), None)
    for k in ("abs_rel", "sq_rel", "rmse", "rmse_log"):
        _within(out[k], oracle[k], f32[k], f"depth l2_scaling {k}")
    with pytest.raises(NotImplementedError):
        M.compute_depth_metrics(gt_d, pred_d, M.median_scaling)


# ------------------------------------------------------------------------------------- dino
@functools.lru_cache(maxsize=None)
def _dino_case(C, P, bf16):
    n, v = 2, 3
    g = torch.Generator().manual_seed(100 * C + P)
    pred = torch.randn(n, v, P, 1, 1, C, generator=g)
    gt = 0.6 * pred.squeeze(-2) + 0.5 * torch.randn(n, v, P, 1, C, generator=g)
    pred[0, 0, 0] = 0       # a zero prediction row: the epsilon branch
    gt[1, 1, P - 1] = 0     # a zero target row
    if bf16:
        pred = pred.bfloat16()
    data64 = {"dino_gt": gt.double(), "coarse": [{"dino_features": pred.double()}]}
    return pred, gt, M.compute_dino_metrics(data64)


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("P", [1, 5, 67])
@pytest.mark.parametrize("C", [64, 384, 768])
def test_dino_metrics(gpu, C, P, bf16):
    pred, gt, oracle = _dino_case(C, P, bf16)
    data = {"dino_gt": gt.to(gpu), "coarse": [{"dino_features": pred.to(gpu)}]}
    f32 = M.compute_dino_metrics(data, native=False)
    out = M.compute_dino_metrics(data, native=True)
    assert list(out) == list(oracle) and len(out) == 12
    for k in out:
        assert out[k].shape == (1,) and out[k].dtype == torch.float32 and out[k].is_cuda
        assert bool(torch.isfinite(out[k]).all())
        _within(out[k], oracle[k], f32[k], f"dino C={C} P={P} bf16={bf16} {k}")
    base = out["l1"].untyped_storage().data_ptr()
    assert all(t.untyped_storage().data_ptr() == base for t in out.values())  # one result row
    for name in ("l1", "l2", "cos_sim"):  # the means row: the view rows added in order, over v
        rows = [out[f"{name}_{i}"].cpu() for i in range(3)]
        assert torch.equal(out[name].cpu(), ((rows[0] + rows[1]) + rows[2]) / 3.0)


# -------------------------------------------------------------------------------------- seg
def _seg_case(gt_classes, n_classes, hw, R, seed=0):
    n, v = 2, 2
    g = torch.Generator().manual_seed(seed + 31 * hw + n_classes)
    target = torch.randint(-1, gt_classes, (n, 1, hw), generator=g)
    results = {}
    for r in range(R):
        pred = torch.randint(0, n_classes, (n, v, 1, hw), generator=g)
        other = torch.randint(0, n_classes, (n, v, 1, hw), generator=g)
        results[f"r{r}"] = {"segs_pred": other, "pseudo_segs_pred": pred} if r % 2 else {"segs_pred": pred}
    return {"segmentation": {"target": target, "results": results}}


def _to(data, dev):
    if isinstance(data, dict):
        return {k: _to(v, dev) for k, v in data.items()}
    return data.to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [1, 20, 1000])
@pytest.mark.parametrize("gt_classes,n_classes", [(19, 19), (19, 27), (3, 5)])
def test_seg_confusion_equals_the_torch_route(gpu, gt_classes, n_classes, hw):
    for R in (1, 2, 3, 4):
        data = _seg_case(gt_classes, n_classes, hw, R)
        want = M.compute_seg_metrics(data, n_classes, gt_classes)
        got = M.compute_seg_metrics(_to(data, gpu), n_classes, gt_classes, native=True)
        assert list(got) == list(want)
        for k in want:
            assert got[k].dtype == torch.int64 and got[k].shape == (gt_classes, n_classes)
            assert torch.equal(got[k].cpu(), want[k]), (R, k)
        assert got.bad_labels.dtype == torch.int32 and int(got.bad_labels) == 0
    # all targets -1: nothing is counted
    data["segmentation"]["target"].fill_(-1)
    got = M.compute_seg_metrics(_to(data, gpu), n_classes, gt_classes, native=True)
    assert all(not bool(m.any()) for m in got.values()) and int(got.bad_labels) == 0


@pytest.mark.gpu
def test_seg_out_of_range_labels_are_counted_not_binned(gpu):
    gt_classes, n_classes, hw = 19, 27, 1000
    data = _seg_case(gt_classes, n_classes, hw, 3)
    seg = data["segmentation"]
    seg["target"][0, 0, 10] = 4
    seg["target"][1, 0, 20] = 5
    clean = M.compute_seg_metrics(data, n_classes, gt_classes)
    want = {k: m.clone() for k, m in clean.items()}
    # pixel (0, 10) gets a target past the table, pixel (1, 20) a bad prediction in result r1
    for k, r in seg["results"].items():
        p = r["pseudo_segs_pred"] if "pseudo_segs_pred" in r else r["segs_pred"]
        want[k][4, p[0, 0, 0, 10]] -= 1
    want["r1"][5, seg["results"]["r1"]["pseudo_segs_pred"][1, 0, 0, 20]] -= 1
    seg["target"][0, 0, 10] = gt_classes
    seg["results"]["r1"]["pseudo_segs_pred"][1, 0, 0, 20] = -3
    got = M.compute_seg_metrics(_to(data, gpu), n_classes, gt_classes, native=True)
    assert int(got.bad_labels) == 2
    for k in want:
        assert torch.equal(got[k].cpu(), want[k]), k
    metric = M.SegmentationMetric("seg", assign_pseudo=False)
    metric.update(got)
    with pytest.raises(ValueError, match="2 pixels"):
        metric.compute()
    seg["results"]["r1"]["pseudo_segs_pred"][1, 0, 0, 20] = n_classes
    assert int(M.compute_seg_metrics(_to(data, gpu), n_classes, gt_classes).bad_labels) == 2


# --------------------------------------------------------------------- all three kernels
def _three_cases(gpu):
    gt, both, _, _ = _depth_case(5000, 3)
    pred, dgt, _ = _dino_case(384, 67, False)
    seg = _to(_seg_case(19, 27, 1000, 4), gpu)
    gt_d, both_d = gt.to(gpu), both.to(gpu)
    dino = {"dino_gt": dgt.to(gpu), "coarse": [{"dino_features": pred.to(gpu)}]}

    def run():
        d = M.compute_depth_metrics(gt_d, both_d[:, :1], None, native=True)
        f = M.compute_dino_metrics(dino, native=True)
        s = M.compute_seg_metrics(seg, 27, 19, native=True)
        return [d[k] for k in M.DEPTH_KEYS] + list(f.values()) + list(s.values()) + [s.bad_labels]

    return run


def _bit_equal(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


@pytest.mark.gpu
def test_repeat_side_stream_and_graph_replay_are_bit_equal(gpu):
    run = _three_cases(gpu)
    first = run()
    assert bool(torch.isnan(first[0]).any())  # the NaN row compares by its bits
    assert _bit_equal(first, run())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run()
    torch.cuda.current_stream().wait_stream(s)
    assert _bit_equal(first, side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _bit_equal(first, captured)


@pytest.mark.gpu
def test_no_host_sync_in_the_metrics_or_the_aggregators(gpu):
    run = _three_cases(gpu)
    run()  # library load, first-launch set-up
    depth, dino, seg = M.DictMeanMetric("depth"), M.DictMeanMetric("dino"), M.SegmentationMetric("seg")
    gt, both, _, _ = _depth_case(5000, 1)
    gt_d, both_d = gt.to(gpu), both.to(gpu)
    nan_gt, nan_both, _, _ = _depth_case(5000, 3)
    nan_gt, nan_both = nan_gt.to(gpu), nan_both.to(gpu)
    pred, dgt, _ = _dino_case(384, 67, False)
    data = {"dino_gt": dgt.to(gpu), "coarse": [{"dino_features": pred.to(gpu)}]}
    sdata = _to(_seg_case(19, 27, 1000, 4), gpu)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            depth.update(M.compute_depth_metrics(gt_d, both_d[:, :1], None))
            dino.update(M.compute_dino_metrics(data))
            seg.update(M.compute_seg_metrics(sdata, 27, 19))
        # an update whose values hold a NaN (the image without a valid pixel) is left out
        depth.update(M.compute_depth_metrics(nan_gt, nan_both[:, :1], None))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out = depth.compute()
    want = M.compute_depth_metrics(gt_d, both_d[:, :1], None, native=False)
    assert sorted(out) == sorted("depth_" + k for k in M.DEPTH_KEYS)
    for k in M.DEPTH_KEYS:  # two updates summed, the NaN one skipped, over three updates
        assert abs(out["depth_" + k] - 2 * float(want[k]) / 3) <= 1e-5 * float(want[k])
    want = M.compute_dino_metrics(data, native=False)
    got = dino.compute()
    assert abs(got["dino_l1"] - float(want["l1"])) <= 1e-5 * float(want["l1"])
    ref = M.compute_seg_metrics(_seg_case(19, 27, 1000, 4), 27, 19)
    res = seg.compute()
    total = M.SegmentationMetric("seg")
    total.update(ref), total.update(ref)
    assert torch.equal(res["r2_assignment"], total.compute()["r2_assignment"])
    assert torch.equal(res["r2_confusion_matrix"], total.compute()["r2_confusion_matrix"])


@pytest.fixture
def fake_reference(tmp_path, monkeypatch):
    """A stand-in ``scenedino`` checkout without common/metrics.py (tests/test_metrics.py's)."""
    root = tmp_path / "ref"
    files = {
        "scenedino/__init__.py": "",
        "scenedino/renderer/__init__.py": "from .nerf import NeRFRenderer\n",
        "scenedino/renderer/nerf.py": "class NeRFRenderer:\n    origin = 'reference'\n",
        "scenedino/models/__init__.py": "def make_model(config, downstream_config=None):\n    return 0\n",
        "scenedino/models/bts.py": "class BTSNet:\n    origin = 'reference'\n",
        "scenedino/common/__init__.py": "",
        "scenedino/common/ray_sampler.py": "class ImageRaySampler:\n    origin = 'reference'\n",
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


@pytest.mark.gpu
def test_install_native_metrics_end_to_end_on_a_small_net(gpu, fake_reference):
    """install(native_metrics=True), then the registered scenedino.common.metrics scores one
    render of a small BTSNet: depth against a synthetic ground truth, the rendered features
    against synthetic targets, both inside the bounds above."""
    from _helpers import build_net
    from scenedino_amd import dropin
    dropin.install(native_metrics=True)
    cm = importlib.import_module("scenedino.common.metrics")
    from scenedino.renderer import NeRFRenderer
    from scenedino.common.ray_sampler import ImageRaySampler
    g = torch.Generator().manual_seed(0)
    H, W, K, C, D = 16, 48, 32, 256, 64
    images = torch.rand(1, 2, 3, H, W, generator=g) * 2 - 1
    grid = torch.randn(1, C, 8, 24, generator=g)
    W_in = torch.randn(128, C + 39, generator=g) * 0.08
    b_in = torch.randn(128, generator=g) * 0.1
    W_out = torch.randn(1 + D, 128, generator=g) * 0.1
    b_out = torch.randn(1 + D, generator=g) * 0.1
    Kn = torch.tensor([[0.7849, 0.0, -0.0312], [0.0, 2.9391, 0.2701], [0.0, 0.0, 1.0]]).expand(1, 2, 3, 3)
    pose = torch.eye(4).repeat(1, 2, 1, 1)
    pose[0, 1, 0, 3] = 0.5
    net = build_net(grid, W_in, b_in, W_out, b_out, "fp32", gpu)
    net.encode(images[:, :1].contiguous().to(gpu), Kn[:, :1].contiguous().to(gpu),
               pose[:, :1].contiguous().to(gpu), ids_encoder=[0], ids_render=[0])
    rays, _ = ImageRaySampler(3, 80, H, W).sample(None, pose.to(gpu), Kn.contiguous().to(gpu))
    r = NeRFRenderer(n_coarse=K, lindisp=True)
    r.z_jitter = torch.rand(2 * H * W, K, generator=g).to(gpu)
    with torch.no_grad():
        c = r.bind_parallel(net).eval()(rays, want_weights=True)["coarse"]
    depth = c["depth"].view(1, 2, H, W)
    feats = c["dino_features"].view(1, 2, H, W, 1, D)
    depth_gt = (depth[:, :1] * (0.7 + 0.6 * torch.rand(1, 1, H, W, generator=g).to(gpu))).contiguous()
    depth_gt[torch.rand(1, 1, H, W, generator=g).to(gpu) < 0.4] = 0
    dino_gt = (0.5 * feats.squeeze(-2) + 0.1 * torch.randn(1, 2, H, W, D, generator=g).to(gpu)).contiguous()
    data = {"coarse": [{"depth": depth, "dino_features": feats}], "dino_gt": dino_gt}

    got = cm.compute_depth_metrics(depth_gt, data["coarse"][0]["depth"][:, :1], None)
    f32 = M.compute_depth_metrics(depth_gt, depth[:, :1], None, native=False)
    f64 = M.compute_depth_metrics(depth_gt.double().cpu(), depth[:, :1].double().cpu(), None)
    for k in M.DEPTH_KEYS:
        _within(got[k], f64[k], f32[k], f"end to end depth {k}")
    got = cm.compute_dino_metrics(data)
    f32 = M.compute_dino_metrics(data, native=False)
    f64 = M.compute_dino_metrics({"coarse": [{"dino_features": feats.double().cpu()}],
                                  "dino_gt": dino_gt.double().cpu()})
    assert got["l1"].untyped_storage().data_ptr() == got["cos_sim_1"].untyped_storage().data_ptr()
    for k in f64:
        _within(got[k], f64[k], f32[k], f"end to end dino {k}")
