"""Train-mode MlpDimReduction.transform_expand: sd_expand_bwd (csrc/sdhip_expand_bwd.hip), the
autograd wiring (models/backbones/dino/dim_reduction.py) and the packs following optimizer
steps.

Tolerance rule (the decoder / ViT backward tests' yardstick without their median
floor): a gradient's rel-L2 distance to CPU fp32 autograd of the reference formula
F.normalize(linear_out(relu(linear_in(x))), dim=-1) is at most 2 x the rel-L2 error of the same
computation under CPU bf16 autocast, measured here on the same inputs, per tensor.
"""
from __future__ import annotations

import ctypes
import functools
import math
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from _helpers import build_net, rel_l2
from conftest import ROOT

BF = torch.bfloat16
CASES = [(P, DF) for DF in (384, 768) for P in (1, 31, 33, 130, 1000)] + [(130, 96)]
NAMES = ("x", "linear_in.weight", "linear_in.bias", "linear_out.weight", "linear_out.bias")


# ------------------------------------------------------------------------ shared inputs
def _inputs(P, DF, zero_out=False):
    """Codes, weights and an output gradient of a case.  linear_in's rows give pre-activations
    of about unit spread around a small bias: about half of the latents of a row are dead."""
    g = torch.Generator().manual_seed(1000 * DF + P)
    d = {"x": torch.randn(P, 64, generator=g),
         "linear_in.weight": torch.randn(128, 64, generator=g) * 0.125,
         "linear_in.bias": torch.randn(128, generator=g) * 0.1,
         "linear_out.weight": torch.randn(DF, 128, generator=g) * 0.09,
         "linear_out.bias": torch.randn(DF, generator=g) * 0.1,
         "dy": torch.randn(P, DF, generator=g)}
    if zero_out:
        d["linear_out.weight"].zero_()
        d["linear_out.bias"].zero_()
    return d


def _formula(x, w1, b1, w2, b2):
    return F.normalize(F.linear(F.relu(F.linear(x, w1, b1)), w2, b2), dim=-1)


def _cpu_grads(d, autocast):
    leaves = [d[n].clone().requires_grad_(True) for n in NAMES]
    with torch.autocast("cpu", dtype=BF, enabled=autocast):
        y = _formula(*leaves)
    gs = torch.autograd.grad((y.float() * d["dy"]).sum(), leaves)
    return {n: g.float() for n, g in zip(NAMES, gs)}


@functools.lru_cache(maxsize=None)
def _oracle(P, DF, zero_out=False):
    """(inputs, fp32 gradients, bf16-autocast gradients) on the CPU, computed once per case."""
    d = _inputs(P, DF, zero_out)
    return d, _cpu_grads(d, False), _cpu_grads(d, True)


def _module(d, dev):
    from scenedino_amd.models.backbones.dino.dim_reduction import MlpDimReduction
    m = MlpDimReduction(d["linear_out.weight"].shape[0], 64, 128)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(d[n])
    return m.to(dev).train()


def _native_grads(m, d, dev):
    x = d["x"].to(dev).requires_grad_(True)
    m.zero_grad(set_to_none=True)
    out = m.transform_expand(x)
    out.backward(d["dy"].to(dev))
    g = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    g["x"] = x.grad.detach().clone()
    return out.detach(), g


def _check(native, g32, g16, names=NAMES, what=""):
    for n in names:
        e = rel_l2(g16[n], g32[n])
        r = rel_l2(native[n], g32[n])
        print(f"{what} {n}: native rel-L2 {r:.5f}, autocast oracle {e:.5f}")
    for n in names:
        gn = native[n].float().cpu()
        assert gn.shape == g32[n].shape and bool(torch.isfinite(gn).all()), n
        e = rel_l2(g16[n], g32[n])
        assert math.isfinite(e) and e > 0, f"{n}: the autocast yardstick is {e}"
        r = rel_l2(gn, g32[n])
        assert r <= 2 * e, f"{what} {n}: rel-L2 {r:.5f} > 2 x {e:.5f}"


# ------------------------------------------------------------------------ CPU
def test_entry_point_is_exported_and_abi_is_13():
    from scenedino_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "sd_expand_bwd") and "sd_expand_bwd" in _lib.SIGNATURES
    assert lib.sd_abi_version() == 13 and _lib.ABI_VERSION == 13


def test_args_struct_layout_matches_the_c_header(tmp_path):
    from scenedino_amd import _lib
    py, cname = _lib.SdExpandBwdArgs, "sd_expand_bwd_args"
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
    """A null pointer, P = 0 and d_full = 100 (validation runs before any HIP call, so this
    needs no device)."""
    from scenedino_amd import _lib
    lib = _lib.load()
    ok = dict(x=16, dy=16, w1=16, w2=16, w1t=16, w2t=16, b1=16, b2=16, P=32, x_dtype=_lib.SD_F32,
              dx=16, h=16, de=16, dh=16, xb=16)
    rec = dict(w1=16, b1=16, w2=16, b2=16, wg=16, g2=16, d_in=64, d_latent=128, d_full=768,
               frag_layout=_lib.SD_SEG_FRAG16)

    def call(args, r):
        a = _lib.SdExpandBwdArgs(**args) if args is not None else None
        h = _lib.SdSegHead(**r) if r is not None else None
        rc = lib.sd_expand_bwd(ctypes.byref(a) if a is not None else None,
                               ctypes.byref(h) if h is not None else None, None)
        return rc, lib.sd_last_error()

    for args, r in ((None, rec), (ok, None), (dict(ok, x=None), rec), (dict(ok, dy=None), rec),
                    (dict(ok, w2t=None), rec), (dict(ok, dx=None), rec), (dict(ok, P=0), rec),
                    (dict(ok, P=-5), rec), (ok, dict(rec, d_full=100)), (ok, dict(rec, d_in=32)),
                    (ok, dict(rec, d_latent=64)), (dict(ok, x_dtype=_lib.SD_F16), rec),
                    (dict(ok, dy=20), rec)):
        rc, msg = call(args, r)
        assert rc == -1 and b"sd_expand_bwd" in msg and b"invalid" in msg, (args, r)


@pytest.mark.parametrize("P,DF", CASES)
def test_autocast_yardstick_is_not_vacuous(P, DF):
    """The bound of the GPU tests is 2 x this error: it has to be a finite, non-zero number
    for every tensor at every shape they use (and for the zeroed linear_out's two tensors)."""
    _, g32, g16 = _oracle(P, DF)
    for n in NAMES:
        e = rel_l2(g16[n], g32[n])
        assert math.isfinite(e) and 0 < e < 0.1, (n, e)
    if (P, DF) == (130, 384):
        _, z32, z16 = _oracle(P, DF, True)
        for n in ("linear_out.weight", "linear_out.bias"):
            e = rel_l2(z16[n], z32[n])
            assert math.isfinite(e) and 0 < e < 0.1, (n, e)
        for n in ("x", "linear_in.weight", "linear_in.bias"):
            assert not z32[n].any()


def test_a_module_that_never_trained_keys_as_before():
    from scenedino_amd.models.backbones.dino.dim_reduction import MlpDimReduction
    from scenedino_amd import pack_cache
    m = MlpDimReduction(384, 64, 128)
    raw = pack_cache.tensor_key(*m.parameters(), *m.buffers())
    assert len(raw) == 4 and m._key() == raw and m not in pack_cache._TRACKED
    assert "_step_gen" not in m.state_dict()
    m._step_gen = 3
    assert m._key() == raw + (("step", 3),)


# ------------------------------------------------------------------------ GPU, single op
@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


_RUNS = {}


def _run(P, DF, dev):
    """Eval output, then two training forward + backward passes of a case (once per case)."""
    if (P, DF) not in _RUNS:
        d = _oracle(P, DF)[0]
        m = _module(d, dev)
        with torch.no_grad():
            ev = m.eval().transform_expand(d["x"].to(dev)).clone()
        m.train()
        out, g1 = _native_grads(m, d, dev)
        _, g2 = _native_grads(m, d, dev)
        _RUNS[(P, DF)] = (ev, out, g1, g2)
    return _RUNS[(P, DF)]


@pytest.mark.gpu
@pytest.mark.parametrize("P,DF", CASES)
def test_training_forward_equals_eval(gpu, P, DF):
    ev, out, _, _ = _run(P, DF, gpu)
    assert out.shape == (P, DF) and out.dtype == torch.float32
    assert torch.equal(out, ev)
    d = _oracle(P, DF)[0]
    ref = _formula(*(d[n] for n in NAMES))
    assert rel_l2(out, ref) <= 1e-2  # tests/test_seg.py's forward tolerance


@pytest.mark.gpu
@pytest.mark.parametrize("P,DF", CASES)
def test_gradients_against_fp32_autograd(gpu, P, DF):
    """Measured on MI355X: see DESIGN §4 (transform_expand backward)."""
    _, _, g1, _ = _run(P, DF, gpu)
    _, g32, g16 = _oracle(P, DF)
    _check(g1, g32, g16, what=f"P={P} d_full={DF}")


@pytest.mark.gpu
@pytest.mark.parametrize("P,DF", CASES)
def test_two_launches_give_the_same_bits(gpu, P, DF):
    _, _, g1, g2 = _run(P, DF, gpu)
    for n in NAMES:
        assert torch.equal(g1[n], g2[n]), n


@pytest.mark.gpu
def test_zero_dy_gives_exact_zeros(gpu):
    d = dict(_oracle(33, 384)[0])
    d["dy"] = torch.zeros_like(d["dy"])
    _, g = _native_grads(_module(d, gpu), d, gpu)
    for n in NAMES:
        assert g[n].shape == d[n].shape and not g[n].any(), n


@pytest.mark.gpu
def test_zeroed_linear_out_takes_the_eps_branch(gpu):
    """|e| = 0 < 1e-12 in every row: de = dy / 1e-12, only linear_out gets a gradient."""
    d, g32, g16 = _oracle(130, 384, True)
    out, g = _native_grads(_module(d, gpu), d, gpu)
    assert not out.any()
    for n in ("x", "linear_in.weight", "linear_in.bias"):
        assert not g[n].any(), n
    _check(g, g32, g16, names=("linear_out.weight", "linear_out.bias"), what="zeroed linear_out")


@pytest.mark.gpu
def test_requires_grad_subsets(gpu):
    d, g32, g16 = _oracle(130, 384)
    m = _module(d, gpu)
    m.linear_in.weight.requires_grad_(False)
    m.linear_in.bias.requires_grad_(False)
    _, g = _native_grads(m, d, gpu)
    assert m.linear_in.weight.grad is None and m.linear_in.bias.grad is None
    full = _run(130, 384, gpu)[2]
    for n in ("x", "linear_out.weight", "linear_out.bias"):
        assert torch.equal(g[n], full[n]), n
    # detached input, trainable weights: weight gradients only
    m = _module(d, gpu)
    x = d["x"].to(gpu)
    out = m.transform_expand(x)
    assert out.grad_fn is not None
    out.backward(d["dy"].to(gpu))
    assert x.grad is None
    for n, p in m.named_parameters():
        assert torch.equal(p.grad, full[n]), n
    # eval mode with grad enabled: the plain kernel call, as before
    out3 = m.eval().transform_expand(x)
    assert out3.grad_fn is None and torch.equal(out3, out.detach())
    m.train()
    # frozen module, detached input: today's path, no graph (train mode, grad enabled)
    for p in m.parameters():
        p.requires_grad_(False)
    out2 = m.transform_expand(x)
    assert out2.grad_fn is None and torch.equal(out2, out.detach())
    assert out2._sd_expand[1] is m and out._sd_expand[1] is m


@pytest.mark.gpu
def test_bf16_input_under_autocast(gpu):
    d, g32, g16 = _oracle(130, 384)
    m = _module(d, gpu)
    x = d["x"].to(gpu).to(BF).requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        out = m.transform_expand(x.view(2, 65, 64))
    assert out.dtype == torch.float32 and out.shape == (2, 65, 384)
    with torch.no_grad():
        assert torch.equal(out.detach(), m.eval().transform_expand(x.detach().view(2, 65, 64)))
    out.backward(d["dy"].to(gpu).view(2, 65, 384))
    assert x.grad.dtype == BF and x.grad.shape == x.shape
    assert bool(torch.isfinite(x.grad.float()).all()) and float(x.grad.float().abs().max()) > 0
    # the kernel on the bf16 codes themselves (sd_seg_query's other input type)
    from scenedino_amd import _lib
    seg, bwd = m._packs(train=True)
    xb = x.detach().contiguous()
    dy = d["dy"].to(gpu)
    dx16, h16, de16, dh16, xb_out = _lib.expand_bwd(xb, seg.rec, bwd, dy)
    dx32, h32, de32, dh32, xb32 = _lib.expand_bwd(xb.float(), seg.rec, bwd, dy)
    assert xb_out is xb and torch.equal(xb32, xb)
    for a, b in ((dx16, dx32), (h16, h32), (de16, de32), (dh16, dh32)):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------ GPU, wiring
@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_packs_follow_adam_step(gpu, fused):
    d = _oracle(130, 384)[0]
    m = _module(d, gpu)
    x = d["x"].to(gpu)
    with torch.no_grad():
        pre = m.eval().transform_expand(x).clone()
    rec = m._rec()
    other = torch.nn.Linear(4, 4).to(gpu)
    other.weight.grad = torch.ones_like(other.weight)
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-2, fused=fused)
    out = m.transform_expand(x)
    assert m._rec() is rec
    out.backward(d["dy"].to(gpu))
    # an optimizer over unrelated parameters: the cached record stays
    torch.optim.SGD(other.parameters(), lr=0.1).step()
    assert m._rec() is rec and m._step_gen == 0
    opt.step()
    assert m._step_gen == 1
    with torch.no_grad():
        post = m.eval().transform_expand(x)
    assert m._rec() is not rec
    ref = _formula(x.cpu(), *(p.detach().cpu() for p in (m.linear_in.weight, m.linear_in.bias,
                                                          m.linear_out.weight, m.linear_out.bias)))
    assert rel_l2(post, ref) <= 1e-2
    assert rel_l2(pre, ref) > 2e-2 and not torch.equal(post, pre)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_net_seg_record_follows_adam_step_over_dim_reduction(gpu, fused):
    """BTSNet._seg_rec (predict_voxels' record, built like the folded 2-D head's) carries
    encoder.dim_reduction's own step count: a fused Adam step over dim_reduction.* bumps no
    version counter and is no step of the downstream head."""
    from scenedino_amd import _lib
    d = _oracle(130, 384)[0]
    net = build_net(torch.zeros(1, 32, 2, 2), torch.zeros(128, 32 + 39), torch.zeros(128),
                    torch.zeros(65, 128), torch.zeros(65), device=gpu)
    net.encoder.dim_reduction = dr = _module(d, gpu)
    x = d["x"].to(gpu)
    expand = lambda r: _lib.seg_query(x, r.rec, want_labels=False, want_full=True)[2]  # noqa: E731
    rec = net._seg_rec(False)
    opt = torch.optim.Adam(dr.parameters(), lr=1e-2, fused=fused)
    dr.transform_expand(x).backward(d["dy"].to(gpu))
    assert net._seg_rec(False) is rec
    opt.step()
    new = net._seg_rec(False)
    assert new is not rec
    ref = _formula(x.cpu(), *(p.detach().cpu() for p in (dr.linear_in.weight, dr.linear_in.bias,
                                                          dr.linear_out.weight, dr.linear_out.bias)))
    assert rel_l2(expand(new), ref) <= 1e-2
    assert rel_l2(expand(rec), ref) > 2e-2


KN = torch.tensor([[0.7849, 0.0, -0.0312], [0.0, 2.9391, 0.2701], [0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def bts(gpu):
    """A small BTSNet on the native DINOv2Module (tests/test_dpt_train.py's configuration:
    ViT-S/16 frozen, DPT decoder trained), encoded in train mode on one 32 x 64 frame."""
    from test_dpt_train import _module as dino_module
    from scenedino_amd.common.positional_encoding import PositionalEncoding
    from scenedino_amd.models import BTSNet
    from scenedino_amd.models.prediction_heads import ResnetFC
    enc = dino_module()
    enc.train_decoder = True
    torch.manual_seed(2)
    head = ResnetFC(d_in=256 + 39, d_out=65, n_blocks=0, d_hidden=128)
    conf = {"predict_dino": True, "dino_dims": 64, "learn_empty": False, "code_mode": "z",
            "inv_z": True, "z_near": 3, "z_far": 80, "sample_color": True, "precision": "fp32"}
    net = BTSNet(conf, enc, PositionalEncoding(6, 3, 1.5, True), {"normal_head": head},
                 final_pred_head="normal_head").to(gpu).train()
    g = torch.Generator().manual_seed(0)
    images = (torch.rand(1, 1, 3, 32, 64, generator=g) * 2 - 1).to(gpu)
    Ks = KN.view(1, 1, 3, 3).to(gpu)
    poses = torch.eye(4).view(1, 1, 4, 4).to(gpu)
    net.encode(images, Ks, poses, ids_encoder=[0], ids_render=[0], ids_loss=[0])
    return net, images, Ks, poses


def _downsample_formula(ds, x):
    """PatchSalienceDownsampler.forward_patches (downsampler.py:82-98) in torch ops."""
    n, p, ph, pw, _, c = x.shape
    s = F.conv2d(x.reshape(-1, ph, pw, c).permute(0, 3, 1, 2), ds["conv.weight"], ds["conv.bias"]).squeeze(1)
    a = torch.softmax((s * ds["patch_weight"] + ds["patch_bias"]).reshape(-1, ph * pw), dim=1)
    y = torch.sum(a.reshape(n, p, ph, pw, 1, 1) * x, dim=(2, 3))
    return y / torch.linalg.norm(y, dim=-1, keepdim=True)


def _dino_loss(pred, gt):
    """ReconstructionLoss's dino term: criterion cosine at temperature_dino 5."""
    c = pred.shape[-1]
    return (1 - F.cosine_similarity(5 * pred.reshape(-1, c), 5 * gt.reshape(-1, c), dim=1)).mean()


@pytest.mark.gpu
def test_end_of_the_reference_step(bts, gpu):
    """encode -> PatchRaySampler -> train-mode render -> expand_dim -> downsample("patch") ->
    cosine DINO loss -> backward -> Adam (trainer.py:180-300 with training/loss/scenedino.yaml's
    dino criterion)."""
    from scenedino_amd.common.ray_sampler import PatchRaySampler
    from scenedino_amd.renderer import NeRFRenderer
    net, images, Ks, poses = bts
    enc = net.encoder
    assert net.grid_f_features[0].grad_fn is not None
    dino_map = net.grid_l_loss_features[0]
    sampler = PatchRaySampler(3, 80, 512, 16, snap_to_grid=True, dino_upscaled=False)
    torch.manual_seed(7)
    rays, _, dino_gt = sampler.sample(images, poses, Ks, dino_features=dino_map)
    assert dino_gt.shape == (1, 2, 384)
    r = NeRFRenderer(n_coarse=32, lindisp=True, hard_alpha_cap=True)
    r.z_jitter = torch.rand(512, 32, generator=torch.Generator().manual_seed(3)).to(gpu)
    feats = r.bind_parallel(net).train()(rays)["coarse"]["dino_features"]
    assert feats.shape == (1, 512, 64) and feats.grad_fn is not None
    trained = [(n, p) for n, p in net.named_parameters()
               if n.startswith(("encoder.dim_reduction.", "heads.normal_head.", "encoder.decoder."))]
    assert len(trained) > 8
    opt = torch.optim.Adam([p for _, p in trained], lr=1e-4)
    opt.zero_grad(set_to_none=True)

    def tail(f):
        full = enc.expand_dim(f.view(1, 2, 16, 16, 1, 64))
        down = enc.downsample(full, "patch")[0]
        return _dino_loss(down, dino_gt)

    loss = tail(feats)
    loss.backward()
    for n, p in trained:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        assert float(p.grad.abs().max()) > 0, n
    before = [p.detach().clone() for _, p in trained]
    opt.step()
    assert all(not torch.equal(p.detach(), b) for (_, p), b in zip(trained, before))

    # the tail alone, from the rendered features detached, under autocast as the trainer runs
    # it, against CPU autograd of the same torch formula
    dr = enc.dim_reduction
    dr.zero_grad(set_to_none=True)
    leaf = feats.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=BF):
        tail(leaf).backward()
    native = {"x": leaf.grad.view(-1, 64)}
    native.update({n: p.grad for n, p in dr.named_parameters()})
    ds = {n: p.detach().cpu() for n, p in enc.downsampler.named_parameters()}
    w = {n: p.detach().cpu() for n, p in dr.named_parameters()}
    f_cpu, gt_cpu = feats.detach().cpu().view(-1, 64), dino_gt.cpu()

    def cpu_grads(autocast):
        leaves = [f_cpu.clone().requires_grad_(True)] + [w[n].clone().requires_grad_(True) for n in NAMES[1:]]
        with torch.autocast("cpu", dtype=BF, enabled=autocast):
            full = _formula(*leaves).view(1, 2, 16, 16, 1, 384)
            lo = _dino_loss(_downsample_formula(ds, full), gt_cpu)
        return {n: g.float() for n, g in zip(NAMES, torch.autograd.grad(lo.float(), leaves))}

    _check(native, cpu_grads(False), cpu_grads(True), what="tail")


@pytest.mark.gpu
def test_sample_from_3d_route_reaches_the_field_head(bts, gpu):
    """trainer.py:441-445: BTSNet.forward on raw points in train mode, then expand_dim."""
    net, images, Ks, poses = bts
    net.zero_grad(set_to_none=True)
    # a fresh grid (an earlier backward freed the encoder graph the fixture's grid hangs on)
    net.train().encode(images, Ks, poses, ids_encoder=[0], ids_render=[0], ids_loss=[0])
    g = torch.Generator().manual_seed(5)
    xyz = torch.stack([torch.rand(1, 96, generator=g) * 2 - 1, torch.rand(1, 96, generator=g) * 0.6 - 0.3,
                       torch.rand(1, 96, generator=g) * 16 + 4], -1).to(gpu)
    _, _, sigma, _, state = net.train()(xyz)
    dino = state["dino_features"].view(1, 12, 8, -1)
    full = net.encoder.expand_dim(dino)
    assert full.shape == (1, 12, 8, 384) and full.grad_fn is not None
    go = torch.randn(full.shape, generator=g).to(gpu)
    (full * go).sum().backward()
    for n, p in list(net.heads["normal_head"].named_parameters()) + \
            list(net.encoder.dim_reduction.named_parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        assert float(p.grad.abs().max()) > 0, n
