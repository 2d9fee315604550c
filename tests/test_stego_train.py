"""StegoClusterHead in train mode: sd_stego_train_fwd / sd_stego_train_bwd
(csrc/sdhip_stego_train.hip) and the autograd wiring in downstream_head/semantic_head.py (the six
parameter gradients are sd_conv_wgrad calls, taps = 1).

Tolerance rule (tests/test_expand_train.py's yardstick): y and every parameter gradient lie
within 2 x the rel-L2 error of the same formula (tests/_stego_oracle.py) under CPU bf16
autocast of its CPU fp32 evaluation, measured here on the same inputs, per tensor.
rows_per_group = 48, so 32-row tiles straddle mask groups; the masks hold about 10 % zeros and
1 / 0.9 elsewhere.
"""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import pytest
import torch

import _stego_oracle as so
from conftest import ROOT

CASES = [(M, d) for d in (384, 768) for M in (1, 31, 33, 130, 1000)]
NAMES = so.STEGO_NAMES
ALL = ("y",) + NAMES


@functools.lru_cache(maxsize=None)
def _oracle(M, d_in, masks=True, zero_row=None):
    """(inputs, fp32 results, bf16-autocast results) on the CPU, computed once per case."""
    d = so.stego_inputs(M, d_in, zero_row=zero_row)
    return d, so.stego_eval(d, False, masks), so.stego_eval(d, True, masks)


# ------------------------------------------------------------------------ CPU
def test_entry_points_are_exported_and_abi_is_13():
    from scenedino_amd import _lib
    lib = _lib.load()
    for name in ("sd_stego_train_fwd", "sd_stego_train_bwd", "sd_cluster_probe",
                 "sd_cluster_probe_work"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.sd_abi_version() == 13 and _lib.ABI_VERSION == 13


@pytest.mark.parametrize("py_name,cname", [("SdStegoTrainArgs", "sd_stego_train_args"),
                                           ("SdClusterProbeArgs", "sd_cluster_probe_args")])
def test_args_struct_layouts_match_the_c_header(tmp_path, py_name, cname):
    from scenedino_amd import _lib
    py = getattr(_lib, py_name)
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


def test_invalid_arguments_return_error_before_any_launch():
    """Validation runs before any HIP call, so this needs no device."""
    from scenedino_amd import _lib
    lib = _lib.load()
    ok = dict(x=16, wl=16, wn1=16, wn2=16, wn2t=16, bl=16, bn1=16, bn2=16, m_lin=16, m_non=16,
              M=100, rows_per_group=48, n_groups=3, d_in=768, d_code=64, normalize=1, y=16,
              xh=16, mid=16, e=16, dy=16, dlin=16, dnon=16, dmid=16)
    bad = [dict(ok, M=0), dict(ok, M=-3), dict(ok, d_in=512), dict(ok, d_in=100),
           dict(ok, d_code=32), dict(ok, rows_per_group=0), dict(ok, n_groups=2)]
    for fn, extra in ((lib.sd_stego_train_fwd, [dict(ok, x=None), dict(ok, wn1=None),
                                                dict(ok, y=None), dict(ok, x=20), dict(ok, mid=8)]),
                      (lib.sd_stego_train_bwd, [dict(ok, e=None), dict(ok, dy=None),
                                                dict(ok, mid=None), dict(ok, wn2t=None),
                                                dict(ok, dy=4), dict(ok, dmid=24)])):
        assert fn(None, None) == -1
        for args in bad + extra:
            rc = fn(ctypes.byref(_lib.SdStegoTrainArgs(**args)), None)
            assert rc == -1 and b"sd_stego_train" in lib.sd_last_error() \
                and b"invalid" in lib.sd_last_error(), args
    pr = dict(x=16, m=None, centres=16, w=None, N=100, rows_per_group=1, n_groups=0, d=768, K=19,
              x_dtype=_lib.SD_F32, work=16, labels=16, S=16, counts=16)
    assert lib.sd_cluster_probe(None, None) == -1
    for args in (dict(pr, N=0), dict(pr, d=96), dict(pr, d=832), dict(pr, d=32), dict(pr, K=0),
                 dict(pr, K=33), dict(pr, x_dtype=_lib.SD_F16), dict(pr, x=None),
                 dict(pr, labels=None), dict(pr, S=8), dict(pr, m=16, rows_per_group=48, n_groups=2),
                 dict(pr, rows_per_group=0)):
        rc = lib.sd_cluster_probe(ctypes.byref(_lib.SdClusterProbeArgs(**args)), None)
        assert rc == -1 and b"sd_cluster_probe" in lib.sd_last_error(), args
    assert lib.sd_cluster_probe_work(0, 768, 19) == -1
    assert lib.sd_cluster_probe_work(100, 100, 19) == -1
    # 4 tiles -> 4 workgroups; the centre pack (32 x d floats) plus K (d + 1) per workgroup
    assert lib.sd_cluster_probe_work(100, 768, 19) == 32 * 768 + 4 * 19 * 769


@pytest.mark.parametrize("M,d_in", CASES)
def test_autocast_yardstick_is_not_vacuous(M, d_in):
    _, f32, f16 = _oracle(M, d_in)
    for n in ALL:
        e = so.rel_l2(f16[n], f32[n])
        assert 0 < e < 0.1, (n, e)


def test_cpu_fallback_is_the_formula():
    """StegoClusterHead.train_rows on CPU tensors: the torch-op path, equal to the oracle."""
    d, f32, _ = _oracle(33, 384)
    m = _module(d, "cpu")
    y = m.train_rows(d["x"], d["m_lin"], d["m_non"], 48)
    y.backward(d["dy"])
    got = {n: p.grad for n, p in m.named_parameters()}
    got["y"] = y.detach()
    for n in ALL:
        assert so.rel_l2(got[n], f32[n]) < 1e-5, n


# ------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _module(d, dev):
    from scenedino_amd.downstream_head.semantic_head import StegoClusterHead
    d_in = d["x"].shape[1]
    m = StegoClusterHead(d_in, 64)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(d[n])
    return m.to(dev).train()


def _native(m, d, dev, masks=True, dy=None):
    m.zero_grad(set_to_none=True)
    ml = d["m_lin"].to(dev) if masks else None
    mn = d["m_non"].to(dev) if masks else None
    y = m.train_rows(d["x"].to(dev), ml, mn, d["rows_per_group"])
    y.backward((d["dy"] if dy is None else dy).to(dev))
    out = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    out["y"] = y.detach().clone()
    return out


_RUNS = {}


def _run(M, d_in, dev):
    if (M, d_in) not in _RUNS:
        d = _oracle(M, d_in)[0]
        m = _module(d, dev)
        _RUNS[(M, d_in)] = (_native(m, d, dev), _native(m, d, dev), m)
    return _RUNS[(M, d_in)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,d_in", CASES)
def test_output_and_gradients_against_the_yardstick(gpu, M, d_in):
    g1, _, _ = _run(M, d_in, gpu)
    _, f32, f16 = _oracle(M, d_in)
    assert g1["y"].shape == (M, 64) and g1["y"].dtype == torch.float32
    so.check(g1, f32, f16, ALL, what=f"M={M} d_in={d_in}")


@pytest.mark.gpu
@pytest.mark.parametrize("M,d_in", CASES)
def test_two_launches_give_the_same_bits(gpu, M, d_in):
    g1, g2, _ = _run(M, d_in, gpu)
    for n in ALL:
        assert torch.equal(g1[n], g2[n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("M,d_in", [(130, 384), (33, 768)])
def test_forward_only_equals_the_saving_forward(gpu, M, d_in):
    g1, _, m = _run(M, d_in, gpu)
    d = _oracle(M, d_in)[0]
    with torch.no_grad():
        y = m.train_rows(d["x"].to(gpu), d["m_lin"].to(gpu), d["m_non"].to(gpu), 48)
    y2 = m.train_rows(d["x"].to(gpu), d["m_lin"].to(gpu), d["m_non"].to(gpu), 48, differentiable=False)
    assert y.grad_fn is None and y2.grad_fn is None
    assert torch.equal(y, g1["y"]) and torch.equal(y2, g1["y"])


@pytest.mark.gpu
@pytest.mark.parametrize("M,d_in", [(130, 384), (130, 768)])
def test_null_masks_equal_all_ones_masks(gpu, M, d_in):
    d, f32, f16 = _oracle(M, d_in, False)
    m = _module(d, gpu)
    none = _native(m, d, gpu, masks=False)
    ones = dict(d, m_lin=torch.ones_like(d["m_lin"]), m_non=torch.ones_like(d["m_non"]))
    one = _native(m, ones, gpu)
    for n in ALL:
        assert torch.equal(none[n], one[n]), n
    so.check(none, f32, f16, ALL, what=f"no masks M={M} d_in={d_in}")


@pytest.mark.gpu
def test_an_all_zero_row_is_finite_and_contributes_nothing(gpu):
    """xh of a zero row is zero: lin = bl, mid = relu(bn1); its dlin / dmid rows multiply zeros in
    the Wl / Wn1 gradients, so changing its dy leaves those two gradients bit-equal."""
    from scenedino_amd import _lib
    d, f32, f16 = _oracle(130, 384, True, 5)
    m = _module(d, gpu)
    g = _native(m, d, gpu)
    so.check(g, f32, f16, ALL, what="zero row")
    _, saved = _lib.stego_train_fwd(d["x"].to(gpu), m._train_pack(), d["m_lin"].to(gpu),
                                    d["m_non"].to(gpu), 48, save=True)
    assert not saved[0][5].any() and bool(saved[0][4].any())
    dy2 = d["dy"].clone()
    dy2[5] = dy2[5] * 7 + 1
    g2 = _native(m, d, gpu, dy=dy2)
    for n in ("linear_path.0.weight", "nonlinear_path.0.weight"):
        assert torch.equal(g[n], g2[n]), n
    assert not torch.equal(g["linear_path.0.bias"], g2["linear_path.0.bias"])


@pytest.mark.gpu
def test_rows_used_as_given_and_frozen_parameters(gpu):
    """normalize=False (forward_training's crops: normalised, then dropped out) against the
    formula; frozen parameters get no gradient and the others keep their bits."""
    d = dict(_oracle(130, 768)[0])
    d["x"] = torch.nn.functional.normalize(d["x"], dim=1) * so.rows_scale(
        so.dropout_scales(3, 768, torch.Generator().manual_seed(3)), 48, 130)

    def cpu(autocast):
        leaves = [d[n].clone().requires_grad_(True) for n in NAMES]
        with torch.autocast("cpu", dtype=so.BF, enabled=autocast):
            y = so.stego_formula(d["x"], *leaves, d["m_lin"], d["m_non"], 48, normalize=False)
        out = dict(zip(NAMES, torch.autograd.grad((y.float() * d["dy"]).sum(), leaves)))
        out["y"] = y.detach().float()
        return out

    m = _module(d, gpu)

    def native():
        m.zero_grad(set_to_none=True)
        y = m.train_rows(d["x"].to(gpu), d["m_lin"].to(gpu), d["m_non"].to(gpu), 48, normalize=False)
        y.backward(d["dy"].to(gpu))
        out = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
        out["y"] = y.detach()
        return out

    full = native()
    so.check(full, cpu(False), cpu(True), ALL, what="normalize=False")
    m.nonlinear_path[0].weight.requires_grad_(False)
    m.nonlinear_path[0].bias.requires_grad_(False)
    part = native()
    assert "nonlinear_path.0.weight" not in part and "nonlinear_path.0.bias" not in part
    for n in part:
        assert torch.equal(part[n], full[n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_packs_follow_adam_step(gpu, fused):
    d = _oracle(130, 384)[0]
    m = _module(d, gpu)
    x, ml, mn = d["x"].to(gpu), d["m_lin"].to(gpu), d["m_non"].to(gpu)
    opt = torch.optim.Adam(m.parameters(), lr=1e-2, fused=fused)
    y = m.train_rows(x, ml, mn, 48)
    pack = m._train_pack()
    y.backward(d["dy"].to(gpu))
    assert m._train_pack() is pack
    opt.step()
    post = m.train_rows(x, ml, mn, 48, differentiable=False)
    assert m._train_pack() is not pack
    ref = so.stego_formula(d["x"], *(p.detach().cpu() for _, p in m.named_parameters()),
                           d["m_lin"], d["m_non"], 48)
    assert so.rel_l2(post, ref) <= 1e-2
    assert so.rel_l2(y, ref) > 2e-2
