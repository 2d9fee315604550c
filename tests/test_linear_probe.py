"""sd_linear_probe (csrc/sdhip_linear_probe.hip) without a GPU: the exported interface, the
argument checks (which return before any launch), LinearHead's torch-op route against the
restated reference formula, and the cached label table against map_kitti_id_to_train_id's loop.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import pytest
import torch

import _linear_probe_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.fixture(scope="module")
def lib():
    from scenedino_amd import _lib
    return _lib.load()


def _last_error(lib):
    return lib.sd_last_error().decode()


def _args(**over):
    """A well-formed argument block over made-up, 16-byte aligned addresses: the checks return
    before anything is read."""
    from scenedino_amd import _lib
    a = dict(x=0x1000, m=None, W=0x2000, b=0x3000, target=0x4000, N=100, rows_per_group=1,
             n_groups=0, d=64, C=19, x_dtype=_lib.SD_F32, normalize=1, work=0x5000, pred=0x6000,
             loss_sum=0x7000, n_valid=0x8000, gW=0x9000, gb=0xa000, row_loss=None)
    a.update(over)
    return _lib.SdLinearProbeArgs(**a)


def test_symbols_and_struct_are_exported(lib):
    from scenedino_amd import _lib
    assert hasattr(lib, "sd_linear_probe") and hasattr(lib, "sd_linear_probe_work")
    assert "sd_linear_probe" in _lib.SIGNATURES and "sd_linear_probe_work" in _lib.SIGNATURES
    names = [f[0] for f in _lib.SdLinearProbeArgs._fields_]
    assert names == ["x", "m", "W", "b", "target", "N", "rows_per_group", "n_groups", "d", "C",
                     "x_dtype", "normalize", "work", "pred", "loss_sum", "n_valid", "gW", "gb",
                     "row_loss"]
    assert ctypes.sizeof(_lib.SdLinearProbeArgs) == 5 * 8 + 3 * 8 + 4 * 4 + 7 * 8
    assert callable(_lib.linear_probe)
    # work: the W pack (32 d floats) and, per workgroup, loss, count, gW and gb
    assert lib.sd_linear_probe_work(100, 64, 19) == 32 * 64 + 4 * (2 + 19 * 64 + 19)
    assert lib.sd_linear_probe_work(16417, 64, 19) == 32 * 64 + 257 * (2 + 19 * 64 + 19)
    assert lib.sd_linear_probe_work(100, 768, 32) == 32 * 768 + 4 * (2 + 32 * 768 + 32)


def test_args_struct_layout_matches_the_c_header(tmp_path):
    """tests/test_stego_train.py's check: every field's offset against gcc's offsetof."""
    from scenedino_amd import _lib
    py, cname = _lib.SdLinearProbeArgs, "sd_linear_probe_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sdhip.h"', "int main(void){",
             f'printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], map(int, out[1::2])))
    assert ctypes.sizeof(py) == got["size"]
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == got[fname], fname


def test_null_argument_block_is_rejected(lib):
    assert lib.sd_linear_probe(None, None) == -1
    assert "sd_linear_probe:" in _last_error(lib)


@pytest.mark.parametrize("over", [dict(d=100), dict(C=0), dict(C=33), dict(N=0),
                                  dict(target=None, loss_sum=None, n_valid=None, gb=None),
                                  dict(target=None, loss_sum=None, n_valid=None)],
                         ids=["d100", "C0", "C33", "N0", "gW_without_target", "grads_without_target"])
def test_out_of_domain_arguments_are_rejected(lib, over):
    a = _args(**over)
    lib.sd_last_error()
    assert lib.sd_linear_probe(ctypes.byref(a), None) == -1
    assert "sd_linear_probe:" in _last_error(lib)


@pytest.mark.parametrize("N,d,C", [(100, 100, 19), (100, 64, 0), (100, 64, 33), (0, 64, 19)])
def test_work_rejects_the_same_shapes(lib, N, d, C):
    assert lib.sd_linear_probe_work(N, d, C) == -1
    assert "sd_linear_probe_work:" in _last_error(lib)


def test_cpu_route_is_the_reference_formula():
    """LinearHead on CPU tensors (the torch-op route) with mask, normalisation, -1 targets and a
    second view: loss, W.grad, b.grad and segs_pred equal the restated formula; the loss reads
    view 0 only, segs_pred covers both views."""
    from scenedino_amd.downstream_head.semantic_head import LinearHead
    n, v, h, w, d, C = 2, 2, 6, 8, 64, 19
    N = n * v * h * w
    W, b, x, _, target = lo.inputs("a", N, d, C)
    g = torch.Generator().manual_seed(9)
    m = lo.dropout_scales(n * v, d, g)
    target = target.view(n, v, h, w)[:, 0].contiguous()
    assert bool((target == -1).any()) and bool((target >= 0).any())
    head = LinearHead(d, C)
    with torch.no_grad():
        head.linear.weight.copy_(W)
        head.linear.bias.copy_(b)
    feats = x.view(n, v, h, w, 1, d)
    res = head(feats, target, _mask=m, _rows_per_group=h * w, _normalize=True)
    res["loss"].backward()

    xh = lo.xhat(x, m, h * w, True)
    z = lo.logits(xh, W, b)
    assert res["segs_pred"].dtype == torch.int64 and res["segs_pred"].shape == (n, v, h, w, 1)
    assert torch.equal(res["segs_pred"].flatten(), z.argmax(dim=1))
    view0 = torch.zeros(n, v, h * w, dtype=torch.bool)
    view0[:, 0] = True
    rows0 = view0.flatten()
    want = lo.probe_eval(x[rows0], W, b, target.flatten(), m[::v].contiguous(), h * w, True)
    torch.testing.assert_close(res["loss"].view(1), want["loss"], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(head.linear.weight.grad, want["gW"], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(head.linear.bias.grad, want["gb"], rtol=1e-5, atol=1e-7)
    # without the private arguments: today's plain call
    plain = head(xh.view(n, v, h, w, 1, d), target)
    torch.testing.assert_close(plain["loss"], res["loss"], rtol=1e-6, atol=1e-7)
    assert torch.equal(plain["segs_pred"], res["segs_pred"])
    assert set(head(xh)) == {"segs_pred"}


def test_train_id_lut_matches_the_loop(monkeypatch):
    """Every id in [-1, 255], ids the table lacks and trainId 255 -> -1 included; the table is
    the tests' own stub."""
    from scenedino_amd.downstream_head.semantic_head import SemanticHead
    mod = lo.install_stub_labels(monkeypatch)
    assert len(mod.labels) == 10
    assert any(lab.id == -1 for lab in mod.labels) and any(lab.trainId == 255 for lab in mod.labels)
    head = SemanticHead(**lo.so.HEAD_ARGS)
    ids = torch.arange(-1, 256).view(1, -1)
    loop = head.map_kitti_id_to_train_id(ids)
    assert loop.dtype == torch.int64 and loop.device.type == "cpu" and loop.shape == ids.shape
    lut = head._train_id_lut("cpu")
    assert lut.dtype == torch.int64 and lut.shape == (257,)
    assert torch.equal(lut[ids + 1], loop)
    assert head._train_id_lut("cpu").data_ptr() == lut.data_ptr()  # built once
    assert int(loop[0, 0 + 1]) == -1 and int(loop[0, 5 + 1]) == 7 and int(loop[0, 100 + 1]) == 0
    # uint8 labels: the loop's comparison wraps the table's id -1 to 255
    ids8 = torch.arange(0, 256, dtype=torch.uint8).view(1, -1)
    assert torch.equal(head._train_id_lut("cpu", uint8=True)[ids8.long() + 1],
                       head.map_kitti_id_to_train_id(ids8))
