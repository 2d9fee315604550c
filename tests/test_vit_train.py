"""ViT encoder backward: sd_attention_bwd / sd_layernorm_bwd / sd_gelu_bwd, the whole-encoder
autograd Function of vit_autograd.py and DINOv2Module.train_encoder.

Gradient oracle: oracle.vit_oracle's block / normalize_input under CPU autograd (its
encoder_forward is wrapped in no_grad, so the loop is restated here), fp32 ("fp32 oracle") and
under torch.autocast("cpu", bfloat16) ("autocast oracle": how the reference trains the ViT).

Tolerance rule (tests/test_dpt_train.py's check_head_gradients, restated in check_gradients
for any set of named gradients): per entry rel-L2 against fp32 <= 2 max(e_n, median e), e_n
the autocast oracle's rel-L2 against fp32 for that entry; the concatenated vector
rel-L2 <= 2 e_all.  Single operations use the same rule with the op's torch form under
autocast as the yardstick, both sides on the same bf16-rounded inputs.  sd_layernorm_bwd is
f32 arithmetic on f32 rows, where autocast keeps layer_norm in fp32 (a zero yardstick): it is
held to the project's f32 bound instead (tests/test_dpt.py: max |d| <= 1e-3 max |ref|).
"""
import copy
import ctypes
import functools
import inspect
import math
import os
import statistics
import subprocess

import pytest
import torch
import torch.nn.functional as F

from _helpers import build_net
from oracle import dpt_oracle as DO
from oracle import vit_oracle as VO
from test_dpt import det_fill
from test_dpt_train import CONF, MODEL_CONF
from test_dropin import fake_reference  # noqa: F401  (fixture: a stand-in scenedino package)
from test_vit import init_vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def _q(t):
    return t.to(BF).float()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _maxrel(got, ref):
    return (got - ref).abs().max().item() / ref.abs().max().item()


def check_gradients(native, g32, g16, what=""):
    """check_head_gradients' rule on named gradients: native, fp32 oracle, autocast oracle."""
    names = sorted(g32)
    e = {n: _rel(g16[n], g32[n]) for n in names}
    assert all(math.isfinite(v) and v > 0 for v in e.values()), "autocast yardstick is zero"
    med = statistics.median(e.values())
    worst = []
    for n in names:
        assert n in native and native[n] is not None, f"{n}: no gradient"
        gn = native[n].detach().float().cpu()
        assert gn.shape == g32[n].shape, (n, gn.shape, g32[n].shape)
        assert torch.isfinite(gn).all() and gn.abs().max() > 0, n
        r = _rel(gn, g32[n])
        worst.append((r / (2 * max(e[n], med)), n, r, e[n]))
    cat = lambda d: torch.cat([d[n].detach().float().cpu().reshape(-1) for n in names])
    r_all, e_all = _rel(cat(native), cat(g32)), _rel(cat(g16), cat(g32))
    worst.sort(reverse=True)
    rels = [w[2] for w in worst]
    print(f"{what}: autocast e median {med:.4f} max {max(e.values()):.4f} all {e_all:.4f}; native "
          f"median {statistics.median(rels):.4f} max {max(rels):.4f} all {r_all:.4f}; closest to "
          f"bound: {worst[0][1]} rel {worst[0][2]:.4f} (e_n {worst[0][3]:.4f})")
    for ratio, n, r, en in worst:
        assert ratio <= 1.0, f"{n}: rel-L2 {r:.4f} > 2 max(e_n {en:.4f}, median {med:.4f})"
    assert r_all <= 2 * e_all, (r_all, e_all)


# ------------------------------------------------------------------ the encoder oracle
def oracle_forward(vit, images, intermediate):
    """vit_oracle.encoder_forward's loop with grad enabled."""
    x = VO.normalize_input(images.float())
    B = x.shape[0]
    C, nh, p = vit.embed_dim, vit.num_heads, vit.patch_size
    gh, gw = x.shape[-2] // p, x.shape[-1] // p
    t = F.conv2d(x, vit.patch_embed.proj.weight, vit.patch_embed.proj.bias, stride=p)
    t = t.flatten(2).transpose(1, 2)
    t = torch.cat([vit.cls_token.expand(B, -1, -1), t], 1) + vit.pos_embed
    grids = []
    to_grid = lambda z: z[:, 1:].transpose(1, 2).reshape(B, C, gh, gw)
    for i, b in enumerate(vit.blocks):
        t = VO.block(t, b, nh)
        if i in intermediate:
            grids.append(to_grid(t))
    f = F.layer_norm(t, (C,), vit.norm.weight, vit.norm.bias, 1e-6)
    f = F.normalize(f[:, 1:], p=2, dim=2)
    f = F.normalize(f.transpose(1, 2), dim=1).reshape(B, C, gh, gw)
    return grids + [f]


def oracle_grads(vit, images, intermediate, gos, autocast):
    vit.zero_grad()
    with torch.autocast("cpu", dtype=BF, enabled=autocast):
        outs = oracle_forward(vit, images, intermediate)
    sum((o.float() * g).sum() for o, g in zip(outs, gos)).backward()
    return {n: p.grad.detach().clone() for n, p in vit.named_parameters()}


# (C, heads, patch, image, batch, layer scale): the generic path with a batch > 1, the
# fuse_ln route at the shipped token count, the padded patch-embed K (588 -> 608 / 640)
ENC_CASES = {"c128": (128, 2, 16, (32, 48), 2, True),
             "c384": (384, 6, 16, (192, 640), 1, False),
             "c768": (768, 12, 14, (56, 84), 2, True)}
INTER = [0, 1]


@functools.lru_cache(maxsize=None)
def enc_case(name):
    """(vit on CPU, images, upstream gradients (NCHW), fp32 grads, autocast grads), once."""
    from scenedino_amd.models.backbones.dino.vit import VisionTransformer
    C, nh, p, img, B, ls = ENC_CASES[name]
    vit = init_vit(VisionTransformer(img, p, C, 2, nh, layer_scale=ls), seed=C)
    g = torch.Generator().manual_seed(C + 1)
    with torch.no_grad():
        for n, prm in vit.named_parameters():
            if n.endswith("gamma"):  # LayerScale drawn around 1 (1e-5 would starve the branch)
                prm.copy_(0.8 + 0.4 * torch.rand(prm.shape, generator=g))
    images = torch.rand(B, 3, *img, generator=g) * 2 - 1
    gh, gw = img[0] // p, img[1] // p
    gos = [torch.randn(B, C, gh, gw, generator=g) for _ in range(3)]
    g32 = oracle_grads(vit, images, INTER, gos, False)
    g16 = oracle_grads(vit, images, INTER, gos, True)
    vit.zero_grad()
    return vit, images, gos, g32, g16


# ------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("py,cname", [("SdAttnBwdArgs", "sd_attn_bwd_args"),
                                      ("SdLnBwdArgs", "sd_ln_bwd_args")])
def test_vit_bwd_struct_layouts_match_the_c_header(tmp_path, py, cname):
    from scenedino_amd import _lib
    py = getattr(_lib, py)
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


def test_vit_bwd_rejects_bad_arguments_without_gpu():
    from scenedino_amd import _lib
    lib = _lib.load()
    assert lib.sd_abi_version() == 13

    def attn(**kw):
        d = dict(q=16, k=16, vt=16, ao=16, d_ao=16, d_qkv=16, work=16, B=1, heads=2, tokens=65,
                 tokens_pad=128, head_dim=64, scale=0.125)
        d.update(kw)
        return _lib.SdAttnBwdArgs(**d)

    for bad in (dict(q=None), dict(k=None), dict(vt=None), dict(ao=None), dict(d_ao=None),
                dict(d_qkv=None), dict(work=None), dict(head_dim=32), dict(head_dim=128),
                dict(tokens_pad=64), dict(tokens_pad=100), dict(tokens=0), dict(q=8),
                dict(scale=0.0)):
        rc = lib.sd_attention_bwd(ctypes.byref(attn(**bad)), None)
        assert rc == -1 and b"sd_attention_bwd" in lib.sd_last_error(), bad
    assert lib.sd_attention_bwd(None, None) == -1 and b"sd_attention_bwd" in lib.sd_last_error()

    def ln(**kw):
        d = dict(x=16, w=16, dy=16, rows=4, C=384, dy_f32=0, accumulate=0, nparts=1, eps=1e-6,
                 dx=16, work=16, dw=16, db=16)
        d.update(kw)
        return _lib.SdLnBwdArgs(**d)

    for bad in (dict(x=None), dict(w=None), dict(dy=None), dict(dx=None), dict(work=None),
                dict(C=386), dict(C=1028), dict(C=0), dict(nparts=0), dict(rows=-1), dict(dx=8)):
        rc = lib.sd_layernorm_bwd(ctypes.byref(ln(**bad)), None)
        assert rc == -1 and b"sd_layernorm_bwd" in lib.sd_last_error(), bad
    assert lib.sd_layernorm_bwd(None, None) == -1 and b"sd_layernorm_bwd" in lib.sd_last_error()
    assert lib.sd_layernorm_bwd_parts(1) == 1 and lib.sd_layernorm_bwd_parts(481) == 121
    assert lib.sd_layernorm_bwd_parts(10 ** 6) == 256

    for bad in ((None, 16, 8, 16), (16, None, 8, 16), (16, 16, 8, None), (16, 16, 12, 16),
                (16, 16, -8, 16), (8, 16, 8, 16)):
        rc = lib.sd_gelu_bwd(bad[0], bad[1], bad[2], bad[3], None)
        assert rc == -1 and b"sd_gelu_bwd" in lib.sd_last_error(), bad


def test_load_names_missing_symbols_and_says_rebuild(monkeypatch):
    """A libsdhip.so from before the ViT backward (same ABI number) must not surface as a bare
    AttributeError."""
    from scenedino_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.SIGNATURES, "sd_not_in_this_build", [])
    with pytest.raises(RuntimeError, match="rebuild") as e:
        _lib.load()
    assert "sd_not_in_this_build" in str(e.value)


def test_install_train_encoder_switch(fake_reference):
    from scenedino_amd import dropin
    from scenedino_amd.models.backbones.dino.dinov2_module import DINOv2Module
    sig = inspect.signature(dropin.install)
    assert sig.parameters["train_encoder"].default is False
    assert sig.parameters["train_decoder"].default is False
    assert sig.parameters["native_encoder"].default is True
    conf = dict(MODEL_CONF, encoder=dict(CONF, encoder_freeze=False, separate_gt_version="v1_16"))
    try:
        dropin.install(train_encoder=True)
        from scenedino.models import make_model
        enc = make_model(conf).encoder
        assert isinstance(enc, DINOv2Module) and enc.train_encoder is True
        assert enc.train_decoder is True  # implied
        with pytest.raises(NotImplementedError, match="dpt"):
            make_model(dict(conf, encoder=dict(conf["encoder"], decoder_arch="bilinear")))
        dropin.install()
        enc = make_model(conf).encoder
        assert enc.train_encoder is False and enc.train_decoder is False
    finally:
        dropin.install()


def _module(conf):
    from scenedino_amd.models.backbones import make_backbone
    torch.manual_seed(11)
    m = make_backbone(conf)
    if hasattr(m.decoder, "reassemble_blocks"):
        det_fill(m.decoder, 70)
    init_vit(m.encoder.model.vit, seed=5)
    return m


TRAIN_CONF = dict(CONF, encoder_freeze=False, separate_gt_version="v1_16")


def test_train_encoder_guards():
    m = _module(dict(TRAIN_CONF, decoder_arch="bilinear")).train()
    assert m.train_encoder is False
    m.train_encoder = True
    with pytest.raises(NotImplementedError, match="dpt"):
        m(torch.zeros(1, 3, 32, 64))
    # the switch left False: a trainable ViT still raises, with or without train_decoder
    m = _module(TRAIN_CONF).train()
    m.train_decoder = True
    with pytest.raises(NotImplementedError, match="forward-only") as e:
        m(torch.zeros(1, 3, 32, 64))
    assert "encoder." in str(e.value) and "train_encoder" in str(e.value)
    # no image gradient
    m.train_encoder = True
    with pytest.raises(NotImplementedError, match="image"):
        m(torch.zeros(1, 3, 32, 64, requires_grad=True))


def test_layer_scale_identity_in_float64():
    from scenedino_amd.models.backbones.dino.vit_autograd import layer_scale_grads
    g = torch.Generator().manual_seed(1)
    M, K, N = 9, 6, 5
    f = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, a, d = f(M, N), f(M, K), f(M, N)
    for with_gamma in (True, False):
        W, b = f(N, K).requires_grad_(), f(N).requires_grad_()
        gamma = (1 + 0.3 * f(N)).requires_grad_() if with_gamma else None
        br = a @ W.t() + b
        y = x + (gamma * br if with_gamma else br)
        ps = [W, b] + ([gamma] if with_gamma else [])
        refs = torch.autograd.grad(y, ps, d)
        got = layer_scale_grads(d.t() @ a, d.sum(0), W.detach(), b.detach(),
                                gamma.detach() if with_gamma else None)
        for r, o in zip(refs, got):
            assert (o - r).abs().max().item() <= 1e-12 * r.abs().max().item()
        assert with_gamma or got[2] is None


def test_transposed_pack_identity_in_float64():
    """sd_gemm multiplies by its weight operand's transpose: dy @ pack_t(W)^T is F.linear's dX."""
    from scenedino_amd.models.backbones.dino.vit_autograd import pack_t
    g = torch.Generator().manual_seed(2)
    x = torch.randn(7, 6, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(10, 6, generator=g, dtype=torch.float64)
    dy = torch.randn(7, 10, generator=g, dtype=torch.float64)
    dx, = torch.autograd.grad(F.linear(x, w), x, dy)
    wt = pack_t(w)
    assert wt.shape == (6, 10) and wt.is_contiguous()
    assert ((dy @ wt.t()) - dx).abs().max().item() <= 1e-12 * dx.abs().max().item()


def test_step_hook_counts_only_the_vits_own_optimizer():
    from scenedino_amd.models.backbones.dino.vit import dino_small
    from scenedino_amd.pack_cache import track_steps
    vit = dino_small(image_size=(32, 64), intermediate_features=[3])
    other = torch.nn.Linear(4, 4)
    track_steps(vit)
    for p in list(vit.parameters()) + list(other.parameters()):
        p.grad = torch.zeros_like(p)
    k0 = vit.key()
    torch.optim.SGD(other.parameters(), lr=0.1).step()
    assert vit.key() == k0
    # versions are bumped by this (non-fused) step too; the step count moves regardless
    torch.optim.SGD(vit.parameters(), lr=0.1).step()
    assert vit._step_gen == 1 and vit.key() != k0 and vit.key()[-1] == ("step", 1)


def test_vit_autograd_holds_no_copy_of_the_route_switches(monkeypatch):
    """The training forward is vit_forward itself: patching a switch on the vit module (an A/B
    run, a test) leaves no second value behind in vit_autograd."""
    from scenedino_amd.models.backbones.dino import vit as V
    from scenedino_amd.models.backbones.dino import vit_autograd as VA
    monkeypatch.setattr(V, "LN_GEMM", False)
    for name in ("LN_GEMM", "LN_GEMM_ALL", "FC2_GRID"):
        assert hasattr(V, name) and not hasattr(VA, name), name
    assert VA.vit_forward is V.vit_forward


@pytest.mark.parametrize("name", sorted(ENC_CASES))
def test_autocast_oracle_yardstick_is_finite_and_nonzero(name):
    vit, _, _, g32, g16 = enc_case(name)
    for n, _ in vit.named_parameters():
        for g in (g32[n], g16[n]):
            assert torch.isfinite(g).all() and g.abs().max() > 0, n
        assert _rel(g16[n], g32[n]) > 0, n


# ------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _attn_case(B, H, T, gpu):
    """bf16-rounded q, k, v, dO; the kernel operands (k / vt padded) and sd_attention's ao."""
    from scenedino_amd import _lib
    g = torch.Generator().manual_seed(1000 * B + 10 * T + H)
    q, k, v = (_q(torch.randn(B, H, T, 64, generator=g)) for _ in range(3))
    do = _q(torch.randn(B, T, H * 64, generator=g))
    Tp = (T + 63) // 64 * 64
    qd = q.to(BF).to(gpu)
    kd = torch.zeros(B, H, Tp, 64, device=gpu, dtype=BF)
    vtd = torch.zeros(B, H, 64, Tp, device=gpu, dtype=BF)
    kd[:, :, :T] = k.to(BF).to(gpu)
    vtd[..., :T] = v.transpose(-1, -2).to(BF).to(gpu)
    ao = torch.empty(B * T, H * 64, device=gpu, dtype=BF)
    _lib.attention(qd, kd, vtd, 0.125, ao)
    return q, k, v, do, qd, kd, vtd, ao, do.to(BF).to(gpu).view(B * T, H * 64)


def _attn_ref(q, k, v, do, autocast):
    B, H, T, _ = q.shape
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    with torch.autocast("cpu", dtype=BF, enabled=autocast):
        att = ((ql * 0.125) @ kl.transpose(-2, -1)).softmax(dim=-1)
        o = (att @ vl).transpose(1, 2).reshape(B, T, H * 64)
    gs = torch.autograd.grad(o.float(), (ql, kl, vl), do)
    return dict(zip(("dq", "dk", "dv"), (t.float() for t in gs)))


def _split_dqkv(d_qkv, B, H, T):
    r = d_qkv.float().cpu().view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    return {"dq": r[0], "dk": r[1], "dv": r[2]}


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,T", [(1, 1, 1), (1, 2, 63), (2, 2, 64), (1, 2, 65), (2, 12, 77),
                                   (1, 6, 481)])
def test_attention_bwd(gpu, B, H, T):
    """sd_attention_bwd against fp32 CPU autograd of softmax(scale q k^T) v.  Measured on
    MI355X, rel-L2 against fp32 of dq / dk / dv (all three within 1e-4 of each other): native
    0.0025 (T = 63), 0.0024 (64, 65, 77), 0.0024 (481) against the autocast yardstick's 0.0040,
    0.0042, 0.0043, 0.0043, 0.0048; concatenated 0.0024-0.0025 against 0.0039-0.0047."""
    from scenedino_amd import _lib
    q, k, v, do, qd, kd, vtd, ao, dod = _attn_case(B, H, T, gpu)
    got = _split_dqkv(_lib.attention_bwd(qd, kd, vtd, ao, dod, 0.125), B, H, T)
    if T == 1:  # the softmax is the constant 1
        assert not got["dq"].any() and not got["dk"].any()
        assert torch.equal(got["dv"].reshape(B, H, 64), do.view(B, H, 64))
        return
    check_gradients(got, _attn_ref(q, k, v, do, False), _attn_ref(q, k, v, do, True),
                    f"attention_bwd {(B, H, T)}")


@pytest.mark.gpu
def test_attention_bwd_hygiene(gpu):
    from scenedino_amd import _lib
    B, H, T = 2, 2, 65
    _, _, _, _, qd, kd, vtd, ao, dod = _attn_case(B, H, T, gpu)
    keep = [t.clone() for t in (qd, kd, vtd, ao, dod)]
    guard = 8
    buf = torch.full((B * T + guard, 3 * H * 64), 7.0, device=gpu, dtype=BF)
    one = _lib.attention_bwd(qd, kd, vtd, ao, dod, 0.125, out=buf[:B * T]).clone()
    assert torch.equal(buf[B * T:], torch.full_like(buf[B * T:], 7.0))
    assert not (one == 7.0).all(dim=1).any()  # every token row was written
    two = _lib.attention_bwd(qd, kd, vtd, ao, dod, 0.125)
    assert torch.equal(one, two)
    assert not kd[:, :, T:].any() and not vtd[..., T:].any()
    for a, b in zip(keep, (qd, kd, vtd, ao, dod)):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [384, 768, 1024, 68])
@pytest.mark.parametrize("rows", [1, 33, 481])
@pytest.mark.parametrize("dy_f32", [False, True])
def test_layernorm_bwd(gpu, C, rows, dy_f32):
    """dx, dw, db against fp32 CPU autograd of F.layer_norm, max |d| / max |ref| <= 1e-3 (the
    module docstring's f32 bound).  Measured on MI355X over the 24 cases: dx <= 2.6e-7,
    dw <= 4.6e-7, db <= 3.1e-7."""
    from scenedino_amd import _lib
    g = torch.Generator().manual_seed(C + rows)
    x = torch.randn(rows, C, generator=g) * 1.5 + 0.3
    w = 1 + 0.1 * torch.randn(C, generator=g)
    b = 0.1 * torch.randn(C, generator=g)
    dy = torch.randn(rows, C, generator=g)
    dy = dy if dy_f32 else _q(dy)
    xl, wl, bl = (t.clone().requires_grad_(True) for t in (x, w, b))
    refs = torch.autograd.grad(F.layer_norm(xl, (C,), wl, bl, 1e-6), (xl, wl, bl), dy)
    xd, wd = x.to(gpu), w.to(gpu)
    dyd = dy.to(gpu) if dy_f32 else dy.to(BF).to(gpu)
    dx, dw, db = _lib.layernorm_bwd(xd, wd, dyd, 1e-6)
    errs = [_maxrel(t.cpu(), r) for t, r in zip((dx, dw, db), refs)]
    print(f"layernorm_bwd C={C} rows={rows} f32={dy_f32}: dx {errs[0]:.3g} dw {errs[1]:.3g} db {errs[2]:.3g}")
    for t, e in zip((dx, dw, db), errs):
        assert torch.isfinite(t).all() and e <= 1e-3
    # accumulate adds onto a prefilled buffer exactly once; repeated launches are bit-equal
    pre = torch.randn(rows, C, generator=g).to(gpu)
    acc = pre.clone()
    _, dw2, db2 = _lib.layernorm_bwd(xd, wd, dyd, 1e-6, dx=acc, accumulate=True)
    assert torch.equal(acc, dx + pre)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    dx3, dw3, db3 = _lib.layernorm_bwd(xd, wd, dyd, 1e-6, want_wb=False)
    assert torch.equal(dx3, dx) and dw3 is None and db3 is None
    # another part count gives the same sums up to f32 order
    _, dw1, db1 = _lib.layernorm_bwd(xd, wd, dyd, 1e-6, nparts=1)
    assert _maxrel(dw1.cpu(), refs[1]) <= 1e-3 and _maxrel(db1.cpu(), refs[2]) <= 1e-3


@pytest.mark.gpu
def test_gelu_bwd(gpu):
    """4096 values: 0, -0, +-large (30, 1e4: Phi is exactly 0 / 1 and u phi(u) exactly 0 in
    f32, no subnormal products), a dense sweep of |u| <= 4 and normal draws clipped there.
    Yardstick: the f32 formula Phi(u) + u phi(u) on the bf16 inputs, rounded to bf16, within 2
    bf16 ulps (one for the output rounding, one for the f32 erf / exp).  For |u| <= 4 an ulp
    of the f32 erf (6e-8, 3e-8 in Phi) is below 1e-4 of |gelu'(u)| >= 5e-4, far under a bf16
    ulp, so the rule is meaningful there.  In the mid tails 4 < |u| <= 8 the f32 formula
    itself cancels (1 + erf) to a few per cent of the result, so those entries are held to
    the float64 value instead: |d| <= 2^-8 |true| + 2e-7 |dh| (bf16 rounding of the result plus
    one f32 ulp of erf and exp in the sum).  Measured on MI355X: 0 ulps from the yardstick
    on every entry outside the mid tails; mid tails at most 0.72 of their bound."""
    from scenedino_amd import _lib
    g = torch.Generator().manual_seed(4)
    edge = torch.tensor([0.0, -0.0, 30.0, -30.0, 1e4, -1e4, 4.0, -4.0])
    u = torch.cat([edge, torch.linspace(-4, 4, 2040), (torch.randn(1536, generator=g) * 2).clamp(-4, 4),
                   torch.linspace(-8, -4.01, 256), torch.linspace(4.01, 8, 256)]).to(BF)
    dh = (torch.randn(4096, generator=g) + 0.1).to(BF)
    assert u.numel() == 4096
    got = _lib.gelu_bwd(u.to(gpu), dh.to(gpu)).cpu()
    assert torch.isfinite(got.float()).all()
    uf, df = u.float(), dh.float()
    deriv = 0.5 * (1 + torch.erf(uf * 0.70710678118654752)) + uf * (0.39894228040143268 * torch.exp(-0.5 * uf * uf))
    ref = (df * deriv).to(BF)
    mid = (uf.abs() > 4) & (uf.abs() <= 8)
    # distance in bf16 ulps: bf16 bit patterns are monotone in magnitude within a sign
    bits = lambda t: t.view(torch.int16).to(torch.int32) & 0x7fff
    zero = (ref.float() == 0) & (got.float() == 0)
    same_sign = torch.signbit(got.float()) == torch.signbit(ref.float())
    dist = (bits(got) - bits(ref)).abs()
    bad = ~mid & ~zero & (~same_sign | (dist > 2))
    print(f"gelu_bwd: max ulp distance outside the mid tails {int(dist[~mid & ~zero].max())}")
    assert not bad.any(), (u[bad][:5], got[bad][:5], ref[bad][:5])
    ud, dd = u.double(), dh.double()
    true = dd * (0.5 * (1 + torch.erf(ud / math.sqrt(2))) + ud * torch.exp(-0.5 * ud * ud) / math.sqrt(2 * math.pi))
    err = (got.double() - true).abs()[mid]
    bound = (2.0 ** -8 * true.abs() + 2e-7 * dd.abs())[mid]
    print(f"gelu_bwd: mid tails max err / bound {float((err / bound).max()):.3g}")
    assert (err <= bound).all()


def _native_grads(name, gpu, nhwc, freeze=False):
    """One training forward + backward of the case on the GPU: (vit, grids, final, grads)."""
    from scenedino_amd.models.backbones.dino.vit import _Packed
    from scenedino_amd.models.backbones.dino.vit_autograd import vit_forward_train
    vit_cpu, images, gos, _, _ = enc_case(name)
    vit = copy.deepcopy(vit_cpu).to(gpu).train()
    if freeze:
        vit.patch_embed.requires_grad_(False)
        vit.blocks[0].requires_grad_(False)
    grids, final = vit_forward_train(vit, images.to(gpu), _Packed(vit), INTER, nhwc=nhwc)
    outs = grids + [final]
    gd = [(g.permute(0, 2, 3, 1).contiguous() if nhwc else g).to(gpu) for g in gos]
    loss = sum((o.float() * g).sum() for o, g in zip(outs, gd))
    return vit, images, outs, loss


@pytest.mark.gpu
@pytest.mark.parametrize("nhwc", [True, False])
@pytest.mark.parametrize("name", sorted(ENC_CASES))
def test_encoder_gradients(gpu, name, nhwc):
    """Depth-2 encoders through vit_forward_train, loss = sum_i (out_i go_i).sum() over both
    intermediate grids and the final grid: every parameter gradient under the tolerance rule,
    the training forward bit-equal to vit_forward, a second backward doubling .grad.
    Measured on MI355X, per-parameter rel-L2 against fp32 (median / max / concatenated), bf16
    NHWC grids then f32 NCHW grids, against the autocast oracle's:
      c128: native 0.0058 / 0.0087 / 0.0057 and 0.0057 / 0.0088 / 0.0057, autocast 0.0059 /
            0.0094 / 0.0059; closest to its bound blocks.0.norm1.weight 0.0085 (2 x 0.0073);
      c384: native 0.0050 / 0.0088 / 0.0046 and 0.0045 / 0.0091 / 0.0042, autocast 0.0050 /
            0.0091 / 0.0049; closest blocks.0.norm2.bias 0.0056 (2 x 0.0052);
      c768: native 0.0052 / 0.0083 / 0.0055 and 0.0049 / 0.0079 / 0.0052, autocast 0.0055 /
            0.0088 / 0.0061; closest blocks.0.norm2.bias 0.0054 (2 x 0.0052)."""
    from scenedino_amd.models.backbones.dino.vit import _Packed, vit_forward
    _, _, _, g32, g16 = enc_case(name)
    vit, images, outs, loss = _native_grads(name, gpu, nhwc)
    assert all(o.grad_fn is not None for o in outs)
    with torch.no_grad():
        grids, final = vit_forward(vit, images.to(gpu), _Packed(vit), INTER, nhwc=nhwc)
    for a, b in zip(outs, grids + [final]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    loss.backward(retain_graph=True)
    native = {n: p.grad.clone() for n, p in vit.named_parameters()}
    check_gradients(native, g32, g16, f"encoder {name} nhwc={nhwc}")
    loss.backward()
    for n, p in vit.named_parameters():
        assert torch.equal(p.grad, 2 * native[n]), n


@pytest.mark.gpu
def test_encoder_frozen_subsets(gpu):
    name = "c128"
    vit, _, _, loss = _native_grads(name, gpu, True)
    loss.backward()
    full = {n: p.grad.clone() for n, p in vit.named_parameters()}
    vit2, _, _, loss2 = _native_grads(name, gpu, True, freeze=True)
    loss2.backward()
    for n, p in vit2.named_parameters():
        if n.startswith("patch_embed.") or n.startswith("blocks.0."):
            assert p.grad is None, n
        else:
            assert torch.equal(p.grad, full[n]), n


@pytest.mark.gpu
def test_training_forward_follows_a_patched_ln_gemm(gpu, monkeypatch):
    """vit.LN_GEMM = False takes the ViT-S case off the sd_ln_gemm route; the training forward
    goes with the inference walk (no sd_ln_gemm launch in either) and stays bit-equal to it."""
    from scenedino_amd import _lib
    from scenedino_amd.models.backbones.dino import vit as V
    from scenedino_amd.models.backbones.dino.vit_autograd import vit_forward_train
    vit_cpu, images, _, _, _ = enc_case("c384")
    vit = copy.deepcopy(vit_cpu).to(gpu).train()
    x, packed = images.to(gpu), V._Packed(vit)
    calls, real = [], _lib.ln_gemm
    monkeypatch.setattr(_lib, "ln_gemm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    vit_forward_train(vit, x, packed, INTER, nhwc=True)
    assert len(calls) == 4  # the default route here: norm1 + qkv and norm2 + fc1 of two blocks
    monkeypatch.setattr(V, "LN_GEMM", False)
    del calls[:]
    for nhwc in (True, False):
        grids, final = vit_forward_train(vit, x, packed, INTER, nhwc=nhwc)
        assert final.grad_fn is not None
        with torch.no_grad():
            ref_grids, ref_final = V.vit_forward(vit, x, packed, INTER, nhwc=nhwc)
        assert not calls
        for a, b in zip(grids + [final], ref_grids + [ref_final]):
            assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.gpu
def test_vit_forward_guard_is_unchanged(gpu):
    from scenedino_amd.models.backbones.dino.vit import _Packed, vit_forward
    vit_cpu, images, _, _, _ = enc_case("c128")
    vit = copy.deepcopy(vit_cpu).to(gpu).train()
    with pytest.raises(NotImplementedError, match="no backward kernels"):
        vit_forward(vit, images.to(gpu), _Packed(vit), INTER)


@pytest.fixture(scope="module")
def trained(gpu):
    """A DINOv2Module with train_encoder on the GPU, its eval / ground-truth outputs before any
    training forward, then one training forward + backward."""
    m = _module(TRAIN_CONF).to(gpu)
    m.train_encoder = True
    x = torch.rand(1, 3, 32, 64, generator=torch.Generator().manual_seed(2)).to(gpu) * 2 - 1
    m.eval()
    with torch.no_grad():
        before = m(x)[0].clone()
        gt = m(x, ground_truth=True)[0].clone()
    m.train()
    grid = m(x)[0]
    go = torch.randn(grid.shape, generator=torch.Generator().manual_seed(5))
    (grid * go.to(gpu)).sum().backward()
    return m, x, before, gt, grid, go


@pytest.mark.gpu
def test_module_trains_encoder(trained, gpu):
    """ViT-S/16 (12 blocks) + DPT at 32 x 64 against the encoder oracle composed with
    dpt_oracle.dpt_forward, all 300 ViT and decoder parameters under the tolerance rule.
    Measured on MI355X (per-parameter rel-L2 against fp32): autocast oracle e median 0.0506,
    max 0.0859, concatenated 0.0360; native median 0.0435, max 0.0785, concatenated 0.0328;
    closest to its bound decoder.fusion_blocks.2.res_conv_unit2.conv1.weight, 0.0615 against
    2 x 0.0507."""
    m, x, before, gt, grid, go = trained
    assert grid.grad_fn is not None and grid.shape == (1, 256, 32, 64)
    want = lambda n: n.startswith("encoder.model.vit.") or n.startswith("decoder.")
    for n, p in m.named_parameters():
        if want(n):
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n
        elif n.startswith("gt_encoder."):
            assert p.grad is None, n
    native = {n: p.grad for n, p in m.named_parameters() if want(n)}
    cpu = _module(TRAIN_CONF)  # (m holds captured graphs: no deepcopy)
    cpu.load_state_dict(m.state_dict())
    vit = cpu.encoder.model

    def grads(autocast):
        cpu.zero_grad()
        with torch.autocast("cpu", dtype=BF, enabled=autocast):
            out = DO.dpt_forward(cpu.decoder, oracle_forward(vit.vit, x.cpu(), vit.intermediate))
        (out.float() * go).sum().backward()
        return {n: p.grad.detach().clone() for n, p in cpu.named_parameters() if want(n)}

    check_gradients(native, grads(False), grads(True), "module")
    with torch.no_grad():
        assert torch.equal(m(x, ground_truth=True)[0], gt)


@pytest.mark.gpu
def test_module_eval_path_unchanged_after_training(trained, gpu):
    m, x, before, _, _, _ = trained
    fresh = _module(TRAIN_CONF).to(gpu)
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert torch.equal(m.eval()(x)[0], before)
        assert torch.equal(fresh.eval()(x)[0], before)
        out = m.train()(x)[0]
    assert out.grad_fn is None and torch.equal(out, before)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [False, True])
def test_packs_follow_adam_step(gpu, fused):
    m = _module(TRAIN_CONF).to(gpu).train()
    m.train_encoder = True
    x = torch.rand(1, 3, 32, 64, generator=torch.Generator().manual_seed(2)).to(gpu) * 2 - 1
    params = list(m.encoder.parameters()) + list(m.decoder.parameters())
    opt = torch.optim.Adam(params, lr=1e-3, fused=fused)

    def three(mod):
        train = mod.train()(x)[0].detach().clone()
        mod.eval()
        with torch.no_grad():
            mod.use_graph = False
            eager = mod(x)[0].clone()
            mod.use_graph = True
            graph = mod(x)[0].clone()
        return train, eager, graph

    b_train, b_eager, b_graph = three(m)
    first = m.train()(x)[0]
    first.square().mean().backward()
    opt.step()
    a = three(m)
    for before, after in zip((b_train, b_eager, b_graph), a):
        assert not torch.equal(before, after)
    fresh = _module(TRAIN_CONF).to(gpu)
    fresh.load_state_dict(m.state_dict())
    fresh.train_encoder = True
    f = three(fresh)
    for got, ref in zip(a, f):
        assert torch.equal(got, ref)


@pytest.mark.gpu
def test_render_loss_reaches_the_vit(gpu):
    """test_dpt_train.test_render_loss_reaches_decoder's end-to-end case with the encoder
    trainable."""
    from scenedino_amd.renderer import NeRFRenderer
    from scenedino_amd.common.ray_sampler import ImageRaySampler
    g = torch.Generator().manual_seed(0)
    H, W, K, C = 32, 64, 32, 256
    m = _module(TRAIN_CONF).to(gpu).train()
    m.train_encoder = True
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
    gq = m.encoder.model.vit.blocks[0].attn.qkv.weight.grad
    assert gq is not None and torch.isfinite(gq).all() and gq.abs().max() > 0
    for n, p in m.decoder.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
