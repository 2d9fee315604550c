"""Memory hygiene of the evaluation-metric kernels (include/sdhip_metrics.h): inputs between
poisoned margins (the strided prediction and target rows included), outputs and scratch behind
sentinels and fully written, on tests/_arena.py's harness; and the ratchet that every stream
entry point of that header has a case here."""
import ctypes
import os
import re

import pytest
import torch

from _arena import assert_clean, run3
from conftest import ROOT

from scenedino_amd.common import metrics as M

F32, BF, I32, I64 = torch.float32, torch.bfloat16, torch.int32, torch.int64

# stream entry point of include/sdhip_metrics.h -> its case in this file
CASES = {
    "sd_depth_metrics": "test_hygiene_depth_metrics",
    "sd_dino_metrics": "test_hygiene_dino_metrics",
    "sd_seg_confusion": "test_hygiene_seg_confusion",
}


def _entry_points():
    src = open(os.path.join(ROOT, "include", "sdhip_metrics.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return sorted(set(re.findall(r"\bint\s+(sd_\w+)\s*\([^;{}]*?void\s*\*\s*stream\s*\)\s*;", src)))


def test_every_entry_point_of_the_metrics_header_has_a_case():
    names = _entry_points()
    assert names == sorted(CASES), names
    src = open(__file__).read()
    for name, func in CASES.items():
        assert re.search(rf"^def {re.escape(func)}\(", src, flags=re.M), (name, func)
        body = src.split(f"def {func}(")[1].split("\n@pytest")[0]
        assert f"lib.{name}(" in body and "ar.arm()" in body, name


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _run(gpu, body):
    findings, plain = run3(gpu, body)
    assert_clean(findings)
    return plain


@pytest.mark.gpu
def test_hygiene_depth_metrics(gpu):
    """n = 3 images of 2500 pixels (two partials, the second ragged); gt rows 2504 apart, the
    prediction rows 5008 apart (view 0 of two views); image 1 has no valid pixel."""
    from scenedino_amd import _lib
    lib = _lib.load()
    n, hw = 3, 2500
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(n, hw, generator=g) * 60 + 1
    gt[torch.rand(n, hw, generator=g) < 0.5] = 0
    gt[1] = 0
    pred = (gt + 1) * (0.5 + torch.rand(n, hw, generator=g))
    nbytes = int(lib.sd_depth_metrics_work(n, hw))
    assert nbytes == n * 2 * 8 * 8

    def body(ar):
        gv, pv = ar.input("gt", gt, ld=hw + 4), ar.input("pred", pred, ld=2 * hw + 8)
        work = ar.output("work", (nbytes // 4,), F32)   # every partial is written
        out = ar.output("out", (n, 8), F32)
        ar.arm()
        _lib._check(lib.sd_depth_metrics(_p(gv), gv.stride(0), _p(pv), pv.stride(0), n, hw, _p(work),
                                         _p(out), _stream()), "sd_depth_metrics")

    plain = _run(gpu, body)
    want = M.compute_depth_metrics(gt.view(n, 1, 50, 50).to(gpu), pred.view(n, 1, 50, 50).to(gpu), None)
    got = plain["out"]
    assert torch.equal(got[:, 7].cpu(), (gt != 0).sum(1).float())
    assert bool(torch.isnan(got[1, :7]).all())
    for i, k in enumerate(M.DEPTH_KEYS):
        assert torch.equal(got[:, i].view(torch.int32), want[k].view(n).view(torch.int32)), k


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, BF])
def test_hygiene_dino_metrics(gpu, dt):
    """n, v = 2, 2 with P = 37 rows of C = 128: three workgroups per slab, the last ragged."""
    from scenedino_amd import _lib
    lib = _lib.load()
    n, v, P, C = 2, 2, 37, 128
    g = torch.Generator().manual_seed(1)
    pred = torch.randn(n, v, P, C, generator=g).to(dt)
    gt = torch.randn(n, v, P, C, generator=g) + 0.5 * pred.float()
    nbytes = int(lib.sd_dino_metrics_work(n, v, P, C))
    assert nbytes == n * v * 3 * 3 * 8

    def body(ar):
        pv, gv = ar.input("pred", pred.view(n * v * P, C)), ar.input("gt", gt.view(n * v * P, C))
        work = ar.output("work", (nbytes // 4,), F32)
        out = ar.output("out", (v + 1, 3), F32)
        ar.arm()
        _lib._check(lib.sd_dino_metrics(_p(pv), _lib.SD_OF_TORCH[dt], _p(gv), n, v, P, C, _p(work),
                                        _p(out), _stream()), "sd_dino_metrics")

    plain = _run(gpu, body)
    want = M.compute_dino_metrics({"dino_gt": gt.view(n, v, P, 1, C).to(gpu),
                                   "coarse": [{"dino_features": pred.view(n, v, P, 1, 1, C).to(gpu)}]},
                                  native=False)
    got = plain["out"]
    for q, name in enumerate(("l1", "l2", "cos_sim")):
        torch.testing.assert_close(got[v, q].view(1), want[name].float(), rtol=1e-5, atol=1e-7)
        for j in range(v):
            torch.testing.assert_close(got[j, q].view(1), want[f"{name}_{j}"].float(), rtol=1e-5, atol=1e-7)


@pytest.mark.gpu
def test_hygiene_seg_confusion(gpu):
    """Three results on n = 2 images of 300 pixels at 19 x 27; prediction rows 604 apart (view 0
    of two views and a gap), so a read past an image meets the poison: an out-of-range label."""
    from scenedino_amd import _lib
    lib = _lib.load()
    n, hw, R, gt_classes, n_classes = 2, 300, 3, 19, 27
    g = torch.Generator().manual_seed(2)
    target = torch.randint(-1, gt_classes, (n, hw), generator=g)
    preds = [torch.randint(0, n_classes, (n, hw), generator=g) for _ in range(R)]
    nb = R * gt_classes * n_classes + 1

    def body(ar):
        tv = ar.input("target", target)
        pv = [ar.input(f"pred{r}", p, ld=2 * hw + 4) for r, p in enumerate(preds)]
        conf = ar.output("conf", (nb,), I32)   # zeroed on the stream by the call itself
        a = _lib.SdSegConfusionArgs(target=tv.data_ptr(), n=n, hw=hw, n_results=R,
                                    gt_classes=gt_classes, n_classes=n_classes, conf=conf.data_ptr())
        for r, p in enumerate(pv):
            a.pred[r], a.pred_stride[r] = p.data_ptr(), p.stride(0)
        ar.arm()
        _lib._check(lib.sd_seg_confusion(ctypes.byref(a), _stream()), "sd_seg_confusion")

    plain = _run(gpu, body)
    want = M.compute_seg_metrics({"segmentation": {"target": target, "results": {
        str(r): {"segs_pred": p.view(n, 1, 1, hw)} for r, p in enumerate(preds)}}}, n_classes, gt_classes)
    got = plain["conf"].cpu()
    assert int(got[-1]) == 0
    for r in range(R):
        assert torch.equal(got[:-1].view(R, gt_classes, n_classes)[r].long(), want[str(r)])
