"""Memory hygiene of the SSCBench pooling kernel (include/sdhip_ssc_pool.h): the fine densities
and labels between NaN- and 1e30-poisoned margins, the pooled outputs behind sentinels and fully
written, on tests/_arena.py's harness; and the ratchet that every stream entry point of that
header has a case here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _ssc_pool_oracle as PO
from _arena import assert_clean, run3
from conftest import ROOT

F32, U8 = torch.float32, torch.uint8

# stream entry point of include/sdhip_ssc_pool.h -> its case in this file
CASES = {
    "sd_ssc_pool": "test_hygiene_ssc_pool",
}


def _entry_points():
    src = open(os.path.join(ROOT, "include", "sdhip_ssc_pool.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return sorted(set(re.findall(r"\bint\s+(sd_\w+)\s*\([^;{}]*?void\s*\*\s*stream\s*\)\s*;", src)))


def test_every_entry_point_of_the_ssc_pool_header_has_a_case():
    names = _entry_points()
    assert names == sorted(CASES), names
    src = open(__file__).read()
    for name, func in CASES.items():
        assert re.search(rf"^def {re.escape(func)}\(", src, flags=re.M), (name, func)
        body = src.split(f"def {func}(")[1].split("\n@pytest")[0]
        assert f"lib.{name}(" in body and "ar.arm()" in body, name


def test_ssc_pool_entry_points_stay_out_of_the_main_header():
    """include/sdhip.h's entry points are pinned by tests/test_hygiene_registry.py."""
    main = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    for name in CASES:
        assert name not in main


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.gpu
@pytest.mark.parametrize("dims,f", [((3, 5, 7), 2), ((2, 3, 33), 4)])
def test_hygiene_ssc_pool(gpu, dims, f):
    """(3, 5, 7) at factor 2: 35 lanes of the one 256-lane block of a plane are live, 14-float
    fine rows; (2, 3, 33) at factor 4: 99 live lanes, 132-float rows, 16-byte loads."""
    from scenedino_amd import _lib
    lib = _lib.load()
    sigma, label = PO.make_inputs(dims, f, 19, 7)
    fine = tuple(f * d for d in dims)
    sig_t, lab_t = torch.from_numpy(sigma), torch.from_numpy(label)

    def body(ar):
        # rows = fine z-runs; the margins hold whole fine (y, z) planes
        sv = ar.input("sigma_f", sig_t.view(-1, fine[2]), tile_rows=2 * fine[1])
        lv = ar.input("seg_f", lab_t.view(-1, fine[2]), tile_rows=2 * fine[1])
        so = ar.output("sigma", (dims[0] * dims[1], dims[2]), F32, tile_rows=2 * dims[1])
        go = ar.output("seg", (dims[0] * dims[1], dims[2]), U8, tile_rows=2 * dims[1])
        ar.arm()
        _lib._check(lib.sd_ssc_pool(sv.data_ptr(), lv.data_ptr(), dims[0], dims[1], dims[2], f,
                                    0.2 / f, 19, so.data_ptr(), go.data_ptr(), _stream()),
                    "sd_ssc_pool")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    _, labels, margin, smax = PO.oracle(sigma, label, f, 0.2 / f, 19)
    clear = margin > PO.MARGIN
    assert (plain["seg"].cpu().numpy().reshape(dims) == labels)[clear].all()
    np.testing.assert_array_equal(plain["sigma"].cpu().numpy().reshape(dims), smax)
