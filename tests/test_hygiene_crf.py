"""Memory hygiene of the dense-CRF kernels (include/sdhip_crf.h): the image, the unaries and the
scratch between poisoned margins, labels and Q behind sentinels and fully written, on
tests/_arena.py's harness; and the ratchet that every stream entry point of that header has a
case here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _crf_oracle as O
from _arena import assert_clean, run3
from conftest import ROOT

F32, I64, U8 = torch.float32, torch.int64, torch.uint8

# stream entry point of include/sdhip_crf.h -> its case in this file
CASES = {
    "sd_dense_crf": "test_hygiene_dense_crf",
}


def _entry_points():
    src = open(os.path.join(ROOT, "include", "sdhip_crf.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return sorted(set(re.findall(r"\bint\s+(sd_\w+)\s*\([^;{}]*?void\s*\*\s*stream\s*\)\s*;", src)))


def test_every_entry_point_of_the_crf_header_has_a_case():
    names = _entry_points()
    assert names == sorted(CASES), names
    src = open(__file__).read()
    for name, func in CASES.items():
        assert re.search(rf"^def {re.escape(func)}\(", src, flags=re.M), (name, func)
        body = src.split(f"def {func}(")[1].split("\n@pytest")[0]
        assert f"lib.{name}(" in body and "ar.arm()" in body, name


def test_crf_entry_points_stay_out_of_the_main_header():
    """include/sdhip.h's entry points are pinned by tests/test_hygiene_registry.py."""
    main = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    assert "sd_dense_crf" not in main


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.gpu
def test_hygiene_dense_crf(gpu):
    """13 x 37 (N = 481: the last query tile and the last key block are ragged) with two results
    of 2 and 19 classes (21 columns: two column tiles, the second ragged), 3 iterations."""
    from scenedino_amd import _lib
    from scenedino_amd.downstream_head import crf
    lib = _lib.load()
    H, W, classes, iters = 13, 37, (2, 19), 3
    N, CT = H * W, sum(classes)
    fx = O.fixture(13, 37, 2)
    g = torch.Generator().manual_seed(3)
    image = torch.from_numpy(fx["image"].copy())
    labs = [torch.from_numpy(fx["labels"].copy()).reshape(-1), torch.randint(0, 19, (N,), generator=g)]
    unary = torch.cat([crf.unary_from_labels(lab, c) for lab, c in zip(labs, classes)])
    cls = (ctypes.c_int32 * 8)(*classes)
    nbytes = int(lib.sd_dense_crf_work(H, W, 2, cls))
    assert nbytes > 0 and nbytes % 16 == 0

    def body(ar):
        iv = ar.input("image", image.view(H, W * 3))
        uv = ar.input("unary", unary)
        work = ar.work("work", nbytes // 4)
        labels = ar.output("labels", (2, N), I64)
        q = ar.output("q", (CT, N), F32)
        a = _lib.SdCrfArgs(image=iv.data_ptr(), unary=uv.data_ptr(), work=work.data_ptr(),
                           labels=labels.data_ptr(), q=q.data_ptr(), H=H, W=W, n_results=2,
                           iters=iters, classes=cls, w_g=3.0, sxy_g=0.3, w_b=4.0, sxy_b=20.0, srgb=3.0)
        ar.arm()
        _lib._check(lib.sd_dense_crf(ctypes.byref(a), _stream()), "sd_dense_crf")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    got_q, got_l = plain["q"].cpu().numpy(), plain["labels"].cpu().numpy()
    assert np.array_equal(got_l[0], got_q[:2].argmax(0)) and np.array_equal(got_l[1], got_q[2:].argmax(0))
    from test_crf_gpu import Q_BOUND
    for r, (c0, c) in enumerate(zip((0, 2), classes)):
        want = O.oracle(fx["image"], unary[c0:c0 + c].numpy().T.astype(np.float64), **dict(O.DEFAULTS, iters=iters))
        assert float(np.abs(got_q[c0:c0 + c].T - want).max()) <= Q_BOUND, r
