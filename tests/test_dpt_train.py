"""DPT decoder backward: sd_conv_wgrad / sd_upsample2x_bwd / sd_relu_bwd, the autograd
Functions of dpt_autograd.py, the differentiable DPTHead path and DINOv2Module.train_decoder.

Gradient oracle: CPU fp32 autograd of torch ops / oracle.dpt_oracle on the same bf16-rounded
operands (dY included).  Single-op tolerances are tests/test_dpt.py's: bf16 outputs
max |d| <= 2e-2 max |ref|, f32 outputs (dW, db) max |d| <= 1e-3 max |ref|.

Whole head / module: per-parameter rel-L2 against the fp32 gradients, bounded by twice the
error e_n of a bf16 pipeline that is not the code under test (the same oracle under CPU bf16
autocast; e_n floored at the median over the parameters), and the concatenated gradient
vector by twice that pipeline's own concatenated error, see check_head_gradients.
"""
import copy
import ctypes
import math
import os
import statistics

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _helpers import build_net, load
from oracle import dpt_oracle as DO
from test_dpt import det_fill, make_head
from test_dropin import fake_reference  # noqa: F401  (fixture: a stand-in scenedino package)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONF = dict(type="dinov2", mode="downsample-prediction", decoder_arch="dpt",
            downsampler_arch="featup", encoder_arch="vit-s", version="v1_16",
            separate_gt_version=None, encoder_freeze=True, flip_avg_gt=False,
            dim_reduction_arch="mlp", num_ch_enc=[64, 64, 128, 256],
            intermediate_features=[3, 6, 9], decoder_out_dim=256, dino_pca_dim=64,
            image_size=[32, 64], key_features=False)


def _q(t):
    return t.to(torch.bfloat16).float()


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous().to(dev)


def _nchw(t):
    return t.float().permute(0, 3, 1, 2).cpu()


def _maxrel(got, ref):
    return (got - ref).abs().max().item() / ref.abs().max().item()


# ------------------------------------------------------------------------ CPU
def test_conv_wgrad_struct_layout_matches_the_c_header(tmp_path):
    import subprocess
    from scenedino_amd import _lib
    py, cname = _lib.SdConvWgradArgs, "sd_conv_wgrad_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sdhip.h"', "int main(void){",
             f'printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in py._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {line.split()[0]: int(line.split()[1]) for line in out if line}
    assert ctypes.sizeof(py) == got["size"]
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == got[fname], fname


def test_conv_wgrad_rejects_bad_arguments_without_gpu():
    from scenedino_amd import _lib
    lib = _lib.load()
    assert lib.sd_abi_version() == 13

    def args(**kw):
        d = dict(x=16, dy=16, work=16, dw=16, db=16, B=1, H=4, W=4, Cin=64, Cout=64, taps=9,
                 stride=1, relu_in=0, nparts=1)
        d.update(kw)
        return _lib.SdConvWgradArgs(**d)

    for bad in (dict(Cin=96), dict(taps=4), dict(x=None), dict(dy=None), dict(work=None),
                dict(dw=None), dict(stride=3), dict(Cout=12), dict(nparts=0), dict(x=8)):
        rc = lib.sd_conv_wgrad(ctypes.byref(args(**bad)), None)
        assert rc == -1 and b"sd_conv_wgrad" in lib.sd_last_error(), bad
    assert lib.sd_conv_wgrad(None, None) == -1
    assert lib.sd_conv_wgrad_work(ctypes.byref(args(Cin=96))) == -1
    assert lib.sd_conv_wgrad_parts(ctypes.byref(args(taps=4))) == -1
    assert lib.sd_conv_wgrad_work(ctypes.byref(args(nparts=3))) == 3 * 64 * (9 * 64 + 1)
    assert lib.sd_upsample2x_bwd(None, 1, 2, 2, 64, None, None) == -1
    assert lib.sd_upsample2x_bwd(16, 1, 2, 2, 12, 16, None) == -1
    assert lib.sd_relu_bwd(None, None, None, 8, None, None) == -1
    assert lib.sd_relu_bwd(16, 16, None, 12, 16, None) == -1


@pytest.mark.parametrize("H,W,stride", [(12, 40, 1), (5, 3, 1), (12, 40, 2), (5, 3, 2)])
def test_dgrad_weight_packs_in_float64(H, W, stride):
    """conv2d(dyz, W') with the rotated / swapped pack equals the autograd dX (float64), the
    stride-2 gradient through the zero-embedded dY; the transposed 1x1 / ConvTranspose packs
    likewise."""
    from scenedino_amd.models.backbones.dino import dpt_autograd as A
    g = torch.Generator().manual_seed(H * W + stride)
    cin, cout = 6, 4
    x = torch.randn(2, cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, stride=stride, padding=1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dx, = torch.autograd.grad(y, x, dy)
    # pack_dgrad3 without its bf16 cast: (Cin, ky, kx, co) rows -> a conv weight (Cin, Cout, 3, 3)
    wd = w.flip(2, 3).permute(1, 2, 3, 0).reshape(cin, -1)
    assert torch.equal(A.pack_dgrad3(w.float()).double(), wd.float().bfloat16().double())
    dyn = dy.permute(0, 2, 3, 1)
    dyz = dyn if stride == 1 else A.embed_stride2(dyn, H, W)
    got = F.conv2d(dyz.permute(0, 3, 1, 2), wd.view(cin, 3, 3, cout).permute(0, 3, 1, 2), padding=1)
    assert (got - dx).abs().max().item() <= 1e-12 * dx.abs().max().item()
    if stride == 1:
        from scenedino_amd.models.backbones.dino.dpt_head import _pack_convT
        for k in (2, 4):
            conv = torch.nn.ConvTranspose2d(cin, cout, k, stride=k).double()
            wp = conv.weight.detach().permute(2, 3, 1, 0).reshape(k * k * cout, cin)
            assert torch.equal(_pack_convT(conv)[0], wp.to(torch.bfloat16))
            xx = x.detach().clone().requires_grad_(True)
            yy = conv(xx)
            dyy = torch.randn(yy.shape, generator=g, dtype=torch.float64)
            dxx, = torch.autograd.grad(yy, xx, dyy)
            dyu = dyy.permute(0, 2, 3, 1).reshape(2, H, k, W, k, cout).permute(0, 1, 3, 2, 4, 5)
            got = (dyu.reshape(-1, k * k * cout) @ wp).view(2, H, W, cin).permute(0, 3, 1, 2)
            assert (got - dxx).abs().max().item() <= 1e-12 * dxx.abs().max().item()


def _module(conf=CONF):
    from scenedino_amd.models.backbones import make_backbone
    torch.manual_seed(11)
    m = make_backbone(conf)
    det_fill(m.decoder, 70)
    return m


def test_guard_without_train_decoder_is_unchanged():
    m = _module().train()
    assert m.train_decoder is False
    with pytest.raises(NotImplementedError, match="forward-only") as e:
        m(torch.zeros(1, 3, 32, 64))
    assert "train_decoder" in str(e.value)


def test_guard_with_trainable_vit_still_raises():
    m = _module(dict(CONF, encoder_freeze=False, separate_gt_version="v1_16")).train()
    m.train_decoder = True
    assert any(p.requires_grad for p in m.encoder.parameters())
    with pytest.raises(NotImplementedError, match="forward-only") as e:
        m(torch.zeros(1, 3, 32, 64))
    assert "encoder." in str(e.value) and "decoder." not in str(e.value)


def test_install_train_decoder_switch():
    from scenedino_amd import dropin
    import inspect
    sig = inspect.signature(dropin.install)
    assert sig.parameters["train_decoder"].default is False
    assert sig.parameters["native_encoder"].default is True


def test_step_hook_counts_only_the_decoders_own_optimizer():
    """module_key follows steps of an optimizer that holds the decoder's parameters (fused
    steps bump no version counter) and ignores other optimizers' steps."""
    from scenedino_amd.pack_cache import module_key, track_steps
    head = make_head()
    other = torch.nn.Linear(4, 4)
    track_steps(head)
    for p in list(head.parameters()) + list(other.parameters()):
        p.grad = torch.zeros_like(p)
    k0 = module_key(head)
    torch.optim.SGD(other.parameters(), lr=0.1).step()
    assert module_key(head) == k0
    torch.optim.SGD(head.parameters(), lr=0.1).step()
    assert head._step_gen == 1 and module_key(head) != k0


MODEL_CONF = {"arch": "BTSNet", "predict_dino": True, "dino_dims": 64, "learn_empty": False,
              "code_mode": "z", "inv_z": True, "z_near": 3, "z_far": 80, "sample_color": True,
              "encoder": CONF, "code": {"num_freqs": 6, "freq_factor": 1.5, "include_input": True},
              "decoder_heads": [{"type": "resnet", "name": "normal_head", "freeze": False,
                                 "args": {"n_blocks": 0, "d_hidden": 128}}],
              "final_prediction_head": "normal_head", "precision": "bf16"}


def test_install_train_decoder_reaches_the_built_encoder(fake_reference):
    """install(train_decoder=True) -> the make_model it aliases sets the switch on the
    native encoder it builds; a plain install() resets it."""
    from scenedino_amd import dropin
    from scenedino_amd.models.backbones.dino.dinov2_module import DINOv2Module
    try:
        dropin.install(train_decoder=True)
        from scenedino.models import make_model
        assert make_model is dropin._ref_make_model
        enc = make_model(MODEL_CONF).encoder
        assert isinstance(enc, DINOv2Module) and enc.train_decoder is True
        dropin.install()
        assert make_model(MODEL_CONF).encoder.train_decoder is False
    finally:
        dropin.install()


# ------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


WGRAD_CASES = [(2, 7, 9, 64, 128, 1), (1, 5, 3, 128, 64, 2), (1, 12, 40, 256, 256, 1),
               (1, 12, 40, 256, 256, 2), (2, 33, 65, 64, 128, 1)]


def _conv_case(B, H, W, Cin, Cout, stride, taps=9):
    g = torch.Generator().manual_seed(H * W + Cin + stride)
    k = 3 if taps == 9 else 1
    x = _q(torch.randn(B, Cin, H, W, generator=g))
    w = _q(torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(taps * Cin))
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = _q(torch.randn(B, Cout, OH, OW, generator=g))
    return x, w, dy


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", WGRAD_CASES)
def test_conv_wgrad(gpu, B, H, W, Cin, Cout, stride):
    from scenedino_amd import _lib
    x, w, dy = _conv_case(B, H, W, Cin, Cout, stride)
    xn, dyn = _nhwc(x, gpu), _nhwc(dy, gpu)
    if (B, H, W) == (2, 33, 65):  # 4290 pixels = 135 chunks of 32: several parts, ragged last
        parts = _lib.conv_wgrad_parts(B, H, W, Cin, Cout, 9, stride)
        nchunk = (B * H * W + 31) // 32
        per = (nchunk + parts - 1) // parts
        assert parts > 1 and (B * H * W) % 32 != 0 and (parts - 1) * per < nchunk
        g = _lib.conv_wgrad_args(B, H, W, Cin, Cout, 9, stride, nparts=parts)
        assert _lib.load().sd_conv_wgrad_work(ctypes.byref(g)) == parts * Cout * (9 * Cin + 1)
    for relu in (False, True):
        wl = w.clone().requires_grad_(True)
        b = torch.zeros(Cout, requires_grad=True)
        y = F.conv2d(F.relu(x) if relu else x, wl, b, stride=stride, padding=1)
        dw_ref, db_ref = torch.autograd.grad(y, (wl, b), dy)
        dw, db = _lib.conv_wgrad(xn, dyn, taps=9, stride=stride, relu_in=relu)
        dw2, db2 = _lib.conv_wgrad(xn, dyn, taps=9, stride=stride, relu_in=relu)
        assert torch.equal(dw, dw2) and torch.equal(db, db2)
        got = dw.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).cpu()
        print(f"dW {_maxrel(got, dw_ref):.3g} db {_maxrel(db.cpu(), db_ref):.3g}")
        assert torch.isfinite(got).all()
        assert _maxrel(got, dw_ref) <= 1e-3
        assert _maxrel(db.cpu(), db_ref) <= 1e-3
    # another part count gives the same sums up to f32 order
    dw1, db1 = _lib.conv_wgrad(xn, dyn, taps=9, stride=stride, relu_in=True, nparts=1)
    assert _maxrel(dw1.cpu(), dw.cpu()) <= 1e-3 and _maxrel(db1.cpu(), db.cpu()) <= 1e-3
    dwn, dbn = _lib.conv_wgrad(xn, dyn, taps=9, stride=stride, relu_in=True, bias=False)
    assert dbn is None and torch.equal(dwn, dw)


@pytest.mark.gpu
def test_conv_wgrad_1x1(gpu):
    from scenedino_amd import _lib
    B, H, W, Cin, Cout = 2, 5, 7, 64, 96
    x, w, dy = _conv_case(B, H, W, Cin, Cout, 1, taps=1)
    wl = w.clone().requires_grad_(True)
    b = torch.zeros(Cout, requires_grad=True)
    dw_ref, db_ref = torch.autograd.grad(F.conv2d(x, wl, b), (wl, b), dy)
    dw, db = _lib.conv_wgrad(_nhwc(x, gpu), _nhwc(dy, gpu), taps=1)
    dw2, db2 = _lib.conv_wgrad(_nhwc(x, gpu), _nhwc(dy, gpu), taps=1)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    assert _maxrel(dw.cpu().view_as(dw_ref), dw_ref) <= 1e-3
    assert _maxrel(db.cpu(), db_ref) <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", WGRAD_CASES[:3])
@pytest.mark.parametrize("relu", [False, True])
def test_conv3x3_function_gradients(gpu, B, H, W, Cin, Cout, stride, relu):
    from scenedino_amd.models.backbones.dino import dpt_autograd as A
    x, w, dy = _conv_case(B, H, W, Cin, Cout, stride)
    conv = torch.nn.Conv2d(Cin, Cout, 3, stride=stride, padding=1)
    with torch.no_grad():
        conv.weight.copy_(w)
    xl = x.clone().requires_grad_(True)
    y = F.conv2d(F.relu(xl) if relu else xl, w, conv.bias.detach(), stride=stride, padding=1)
    dx_ref, = torch.autograd.grad(y, xl, dy)
    conv = conv.to(gpu)
    xn = _nhwc(x, gpu).requires_grad_(True)
    out = A.conv3x3(xn, conv, stride=stride, relu_in=relu)
    assert _maxrel(_nchw(out.detach()), y.detach()) <= 2e-2
    out.backward(_nhwc(dy, gpu))
    assert xn.grad.dtype == torch.bfloat16 and conv.weight.grad.dtype == torch.float32
    assert _maxrel(_nchw(xn.grad), dx_ref) <= 2e-2
    assert conv.weight.grad.shape == conv.weight.shape and conv.bias.grad.shape == conv.bias.shape


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 2, 4])
def test_linear_function_gradients(gpu, k):
    """1x1 (k = 0) and ConvTranspose2d(k, stride k) on test_conv_transpose_shuffle's case."""
    from scenedino_amd.models.backbones.dino import dpt_autograd as A
    g = torch.Generator().manual_seed(k)
    conv = torch.nn.ConvTranspose2d(64, 96, k, stride=k) if k else torch.nn.Conv2d(64, 96, 1)
    with torch.no_grad():
        conv.weight.copy_(_q(conv.weight))
    x = _q(torch.randn(2, 64, 5, 7, generator=g))
    xl = x.clone().requires_grad_(True)
    y = conv(xl)
    dy = _q(torch.randn(y.shape, generator=g))
    dx_ref, dw_ref, db_ref = torch.autograd.grad(y, (xl, conv.weight, conv.bias), dy)
    conv = conv.to(gpu)
    xn = _nhwc(x, gpu).requires_grad_(True)
    out = A.linear(xn, conv)
    assert _maxrel(_nchw(out.detach()), y.detach()) <= 2e-2
    out.backward(_nhwc(dy, gpu))
    assert _maxrel(_nchw(xn.grad), dx_ref) <= 2e-2
    assert _maxrel(conv.weight.grad.cpu(), dw_ref) <= 1e-3
    assert _maxrel(conv.bias.grad.cpu(), db_ref) <= 1e-3
    # the projections' input (ViT tokens) needs no gradient: dX is skipped
    conv.zero_grad()
    A.linear(_nhwc(x, gpu), conv).backward(_nhwc(dy, gpu))
    assert _maxrel(conv.weight.grad.cpu(), dw_ref) <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 6, 20, 64), (1, 5, 3, 64)])
def test_upsample2x_bwd(gpu, shape):
    from scenedino_amd import _lib
    B, H, W, C = shape
    g = torch.Generator().manual_seed(H * W)
    x = torch.zeros(B, C, H, W, requires_grad=True)
    y = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    dy = _q(torch.randn(y.shape, generator=g))
    ref, = torch.autograd.grad(y, x, dy)
    dyn = _nhwc(dy, gpu)
    got = _lib.upsample2x_bwd(dyn)
    assert torch.equal(got, _lib.upsample2x_bwd(dyn))
    assert got.shape == (B, H, W, C)
    assert _maxrel(_nchw(got), ref) <= 2e-2


@pytest.mark.gpu
def test_relu_bwd_exact(gpu):
    from scenedino_amd import _lib
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 7, 64, generator=g).to(torch.bfloat16)
    x.view(-1)[::5] = 0.0
    x.view(-1)[1::7] = -0.0
    gr = torch.randn(x.shape, generator=g).to(torch.bfloat16)
    res = torch.randn(x.shape, generator=g).to(torch.bfloat16)
    assert (x == 0).any() and torch.signbit(x[x == 0].float()).any()
    ref = torch.where(x > 0, gr, torch.zeros_like(gr))
    assert torch.equal(_lib.relu_bwd(x.to(gpu), gr.to(gpu)).cpu(), ref)
    ref2 = (ref.float() + res.float()).to(torch.bfloat16)
    assert torch.equal(_lib.relu_bwd(x.to(gpu), gr.to(gpu), res.to(gpu)).cpu(), ref2)


@pytest.mark.gpu
def test_residual_unit_gradients(gpu):
    """x, extra -> conv2(relu(conv1(relu(x)))) + x + extra through the Functions against
    autograd of dpt_oracle._rcu: dX, d extra and the four parameter gradients."""
    from scenedino_amd.models.backbones.dino import dpt_autograd as A
    from scenedino_amd.models.backbones.dino.dpt_head import PreActResidualConvUnit
    g = torch.Generator().manual_seed(9)
    unit = PreActResidualConvUnit(64)
    det_fill(unit, 3)
    with torch.no_grad():
        for p in unit.parameters():
            if p.dim() > 1:
                p.copy_(_q(p))
    x = _q(torch.randn(2, 64, 7, 9, generator=g))
    extra = _q(torch.randn(2, 64, 7, 9, generator=g))
    xl, el = x.clone().requires_grad_(True), extra.clone().requires_grad_(True)
    y = DO._rcu(unit, xl) + el
    dy = _q(torch.randn(y.shape, generator=g))
    ps = [unit.conv1.weight, unit.conv1.bias, unit.conv2.weight, unit.conv2.bias]
    refs = torch.autograd.grad(y, [xl, el] + ps, dy)
    cpu_unit = copy.deepcopy(unit)
    unit = unit.to(gpu)
    xn, en = _nhwc(x, gpu).requires_grad_(True), _nhwc(extra, gpu).requires_grad_(True)
    t = A.conv3x3(xn, unit.conv1, relu_in=True)
    out = A.conv3x3(t, unit.conv2, relu_in=True, res=xn, res2=en)
    assert _maxrel(_nchw(out.detach()), y.detach()) <= 2e-2
    out.backward(_nhwc(dy, gpu))
    assert _maxrel(_nchw(xn.grad), refs[0]) <= 2e-2
    assert _maxrel(_nchw(en.grad), refs[1]) <= 2e-2
    # Against _rcu, whose intermediates t and dT stay fp32 while the native ones are rounded
    # to bf16, conv1's gradients (made from dT) and conv2.weight (made from t) are held to the
    # bf16 tolerance; conv2.bias (a sum of dY alone) to the f32 one.  Measured on MI355X:
    # conv1.weight 1.8e-3, conv1.bias 9.4e-4, conv2.weight 1.9e-3, conv2.bias 0; conv2.weight
    # against the oracle with t rounded too (below) 1.1e-7.
    got = [unit.conv1.weight.grad, unit.conv1.bias.grad, unit.conv2.weight.grad, unit.conv2.bias.grad]
    errs = [_maxrel(gg.cpu(), rr) for gg, rr in zip(got, refs[2:])]
    print("rcu parameter gradients vs _rcu: " + " ".join(f"{e:.3g}" for e in errs))
    for e, tol in zip(errs, (2e-2, 2e-2, 2e-2, 1e-3)):
        assert e <= tol
    # conv2.weight against the same unit with t rounded to bf16 in the oracle too (straight
    # through): the same operands as the kernel's, so the f32 tolerance
    t = F.conv2d(F.relu(x), cpu_unit.conv1.weight, cpu_unit.conv1.bias, padding=1)
    y2 = F.conv2d(F.relu(_q(t.detach())), cpu_unit.conv2.weight, cpu_unit.conv2.bias, padding=1)
    dw2_ref, = torch.autograd.grad(y2, cpu_unit.conv2.weight, dy)
    e2 = _maxrel(unit.conv2.weight.grad.cpu(), dw2_ref)
    print(f"conv2.weight vs oracle with bf16 t: {e2:.3g}")
    assert e2 <= 1e-3


def _oracle_grads(head_cpu, inputs, go, autocast):
    head_cpu.zero_grad()
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        out = DO.dpt_forward(head_cpu, inputs)
    (out.float() * go).sum().backward()
    return out.detach().float(), {n: p.grad.detach().clone() for n, p in head_cpu.named_parameters()}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def check_head_gradients(native, head_cpu, inputs, go):
    """native: {name: grad} of the code under test.  Asserts, per parameter, rel-L2 against
    the fp32 oracle <= 2 max(e_n, median e), e_n the error of the CPU bf16-autocast oracle
    against fp32, and on the concatenated gradient vector rel-L2 <= 2 e_all (no floor)."""
    _, g32 = _oracle_grads(head_cpu, inputs, go, False)
    _, g16 = _oracle_grads(head_cpu, inputs, go, True)
    names = sorted(g32)
    e = {n: _rel(g16[n], g32[n]) for n in names}
    med = statistics.median(e.values())
    worst = []
    for n in names:
        assert n in native and native[n] is not None, f"{n}: no gradient"
        gn = native[n].detach().float().cpu()
        assert torch.isfinite(gn).all() and gn.abs().max() > 0, n
        r = _rel(gn, g32[n])
        worst.append((r / (2 * max(e[n], med)), n, r, e[n]))
    cat = lambda d: torch.cat([d[n].detach().float().cpu().reshape(-1) for n in names])
    r_all, e_all = _rel(cat(native), cat(g32)), _rel(cat(g16), cat(g32))
    worst.sort(reverse=True)
    rels = [w[2] for w in worst]
    print(f"autocast e: median {med:.4f} max {max(e.values()):.4f} all {e_all:.4f}; native: "
          f"median {statistics.median(rels):.4f} max {max(rels):.4f} all {r_all:.4f}; "
          f"closest to bound: {worst[0][1]} rel {worst[0][2]:.4f} (e_n {worst[0][3]:.4f})")
    for ratio, n, r, en in worst:
        assert ratio <= 1.0, f"{n}: rel-L2 {r:.4f} > 2 max(e_n {en:.4f}, median {med:.4f})"
    assert r_all <= 2 * e_all, (r_all, e_all)


@pytest.mark.gpu
def test_head_gradients(gpu):
    """make_head().train() on the inputs of dpt_head.npz, upstream gradient seed 5.
    Measured on MI355X (per-parameter rel-L2 against the fp32 gradients): autocast oracle e
    median 0.0386, max 0.0999, concatenated 0.0243; native median 0.0392, max 0.0686,
    concatenated 0.0230; closest to its bound reassemble_blocks.projects.2.bias, 0.0438
    against 2 x 0.0386.  Training-forward output 7.5e-3 rel-L2 from the fixture."""
    d = load("dpt_head.npz")
    inputs = [torch.as_tensor(d[f"in{i}"]) for i in range(4)]
    ref = torch.as_tensor(d["out"].astype(np.float32))
    go = torch.randn(ref.shape, generator=torch.Generator().manual_seed(5))
    head_cpu = make_head()
    head = copy.deepcopy(head_cpu).to(gpu).train()
    out = head([x.to(gpu) for x in inputs])[0]
    assert out.grad_fn is not None and out.dtype == torch.float32 and out.shape == ref.shape
    rel = _rel(out.detach().cpu(), ref)
    print(f"training forward rel-L2 {rel:.4g}")
    assert rel <= 3e-2
    (out * go.to(gpu)).sum().backward()
    check_head_gradients({n: p.grad for n, p in head.named_parameters()}, head_cpu, inputs, go)


@pytest.fixture(scope="module")
def trained(gpu):
    """A DINOv2Module with train_decoder on the GPU, its eval output before any training
    forward, one training forward + backward."""
    m = _module().to(gpu)
    m.train_decoder = True
    x = torch.rand(1, 3, 32, 64, generator=torch.Generator().manual_seed(2)).to(gpu) * 2 - 1
    m.eval()
    with torch.no_grad():
        before = m(x)[0].clone()
    assert m._graph is not None
    m.train()
    grid = m(x)[0]
    go = torch.randn(grid.shape, generator=torch.Generator().manual_seed(5))
    (grid * go.to(gpu)).sum().backward()
    return m, x, before, grid, go


@pytest.mark.gpu
def test_module_trains_decoder(trained, gpu):
    """Measured on MI355X: autocast oracle e median 0.0353, max 0.0586, concatenated 0.0208;
    native median 0.0377, max 0.0571, concatenated 0.0206."""
    from scenedino_amd.models.backbones.dino.vit import vit_forward
    m, x, before, grid, go = trained
    assert grid.grad_fn is not None and grid.shape == (1, 256, 32, 64)
    assert all(p.grad is not None for p in m.decoder.parameters())
    assert all(p.grad is None for p in m.encoder.parameters())
    vit = m.encoder.model
    with torch.no_grad():
        grids, final = vit_forward(vit.vit, x, vit.packed(), vit.intermediate, nhwc=True)
    inputs = [_nchw(t) for t in grids + [final]]
    head_cpu = copy.deepcopy(m.decoder).cpu()
    check_head_gradients({n: p.grad for n, p in m.decoder.named_parameters()}, head_cpu, inputs, go)


@pytest.mark.gpu
def test_module_eval_path_unchanged(trained, gpu):
    m, x, before, _, _ = trained
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x)[0], before)
    m.train()
    with torch.no_grad():
        out = m(x)[0]
    assert out.grad_fn is None and torch.equal(out, before)
    assert m._graph is not None


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
def test_packs_follow_adam_step(gpu, fused):
    m = _module().to(gpu).train()
    m.train_decoder = True
    x = torch.rand(1, 3, 32, 64, generator=torch.Generator().manual_seed(2)).to(gpu) * 2 - 1
    opt = torch.optim.Adam([p for p in m.decoder.parameters()], lr=1e-3, fused=fused)
    first = m(x)[0]
    first.square().mean().backward()
    opt.step()
    second = m(x)[0].detach()
    assert not torch.equal(second, first.detach())
    fresh = _module().to(gpu)
    fresh.load_state_dict(m.state_dict())
    fresh.train_decoder = True
    assert torch.equal(fresh.train()(x)[0].detach(), second)
    # the inference packs (graph path) follow the step too
    with torch.no_grad():
        assert torch.equal(m.eval()(x)[0], fresh.eval()(x)[0])


@pytest.mark.gpu
def test_render_loss_reaches_decoder(gpu):
    from scenedino_amd.renderer import NeRFRenderer
    from scenedino_amd.common.ray_sampler import ImageRaySampler
    g = torch.Generator().manual_seed(0)
    H, W, K, C = 32, 64, 32, 256
    m = _module().to(gpu).train()
    m.train_decoder = True
    images = torch.rand(1, 1, 3, H, W, generator=g) * 2 - 1
    W_in = torch.randn(128, C + 39, generator=g) * 0.08
    b_in = torch.randn(128, generator=g) * 0.1
    W_out = torch.randn(65, 128, generator=g) * 0.1
    b_out = torch.randn(65, generator=g) * 0.1
    Kn = torch.tensor([[0.7849, 0.0, -0.0312], [0.0, 2.9391, 0.2701], [0.0, 0.0, 1.0]]).view(1, 1, 3, 3)
    pose = torch.eye(4).view(1, 1, 4, 4)
    net = build_net(torch.zeros(1, C, H, W), W_in, b_in, W_out, b_out, "fp32", gpu)
    net.encode(images.to(gpu), Kn.to(gpu), pose.to(gpu), ids_encoder=[0], ids_render=[0])
    grid = m(images[0].to(gpu))[0]
    assert grid.grad_fn is not None
    net.grid_f_features[0] = grid.view(1, 1, C, H, W)
    net.train()
    rays, _ = ImageRaySampler(3, 80, 16, 48).sample(None, pose.to(gpu), Kn.to(gpu))
    r = NeRFRenderer(n_coarse=K, lindisp=True, hard_alpha_cap=True)
    r.z_jitter = torch.rand(16 * 48, K, generator=g).to(gpu)
    c = r.bind_parallel(net).train()(rays)["coarse"]
    (c["dino_features"].square().sum() + c["depth"].sum()).backward()
    for n, p in list(m.decoder.named_parameters()) + list(net.heads["normal_head"].named_parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
