"""Memory hygiene of the ViT encoder kernels (sdhip_vit.hip, sdhip_vit_bwd.hip): every output
behind guard bands, every input between poisoned margins (tests/_arena.py), plus the direct
float64 references of sd_tokens_to_nhwc and sd_patchify, which the suite otherwise only
compares with other kernels."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from _arena import assert_clean, run3, sentinel_bits

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _gemm_inputs(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF)
    bias = 0.1 * torch.randn(N, generator=g)
    gam = torch.rand(N, generator=g)
    x0 = torch.randn(M, N, generator=g)
    return a, w, bias, gam, x0


# One shape per tiling vt_pick_gemm can choose (read from sdhip_vit.hip's vt_pick_gemm for a
# 256-CU device; t32 / mid / big are its tile counts), from test_resid_gemm_every_tiling's list
# with M moved to the smallest ragged value where the list only has a multiple of the tile rows,
# and the two 32-deep K steps (K % 64 != 0) that list does not reach:
GEMM_SHAPES = [
    (481, 384, 384),    # 32 x 32 x 128 split-K over the waves: mid 48 < 256, K % 256 != 0
    (50, 256, 512),     # 32 x 32 x 256: t32 = 16 <= CUs, K % 256 == 0
    (1921, 768, 3072),  # 64 x 64 x 64: mid 372 >= 256, big 96 < 256
    (8100, 1024, 256),  # 128 x 128 x 64: big 512 (the list's 8192 is a multiple of 128)
    (77, 96, 96),       # 64 x 64 x 32: K % 64 != 0
    (8100, 1024, 96),   # 128 x 128 x 32: big 512, K % 64 != 0
]


def _run_gemm(gpu, M, N, K, epi_name, gamma=True):
    from scenedino_amd import _lib
    a, w, bias, gam, x0 = _gemm_inputs(M, N, K, M + N + K)
    epi = getattr(_lib, "SD_EPI_" + epi_name)

    def body(ar):
        av = ar.input("a", a, ld=K + 8, tile_rows=256)
        wv = ar.input("w", w, tile_rows=256)
        bv = ar.input("bias", bias)
        gv = ar.input("gamma", gam) if (epi_name == "RESID" and gamma) else None
        if epi_name == "RESID":
            out = ar.output("out", (M, N), F32, ld=N + 8, tile_rows=256, preset=x0)
        else:
            out = ar.output("out", (M, N), F32 if epi_name == "F32" else BF, ld=N + 8, tile_rows=256)
        ar.arm()
        _lib.gemm(av, wv, bv, epi, out=out, gamma=gv)

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    return plain, (a, w, bias, gam, x0)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("epi", ["F32", "BF16", "GELU", "RESID", "RESID_nogamma"])
def test_hygiene_gemm(gpu, M, N, K, epi):
    """sd_gemm, lda = K + 8 and ldo = N + 8: nothing outside the M x N payload is written,
    every payload element is, a, w, bias, gamma stay as they were, and NaN / 1e30 behind the
    ragged last rows and in the row gaps of a do not reach the product."""
    plain, (a, w, bias, gam, x0) = _run_gemm(gpu, M, N, K, epi.split("_")[0], gamma=epi == "RESID")
    assert torch.isfinite(plain["out"].float()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(481, 384, 1536), (97, 64, 2048)])
@pytest.mark.parametrize("epi", ["F32", "RESID", "GELU"])
def test_hygiene_gemm_split_k(gpu, M, N, K, epi, monkeypatch):
    """The cross-workgroup split-K route (SD_SPLITK_WG=512, as test_gemm_cross_workgroup_split_k
    sets it): the last arriver's combine keeps to the payload too."""
    monkeypatch.setenv("SD_SPLITK_WG", "512")
    plain, _ = _run_gemm(gpu, M, N, K, epi)
    assert torch.isfinite(plain["out"].float()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,C,Kh", [(2, 16, 384, 1536), (1, 78, 768, 768)])
def test_hygiene_gemm_resid_grid_out(gpu, B, T, C, Kh):
    """SD_EPI_RESID with grid_out: the bf16 (B, T - 1, C) copy is written in full and nothing
    around it; it is the bf16 rounding of the updated rows without each image's class token."""
    from scenedino_amd import _lib
    M = B * T
    a, w, bias, gam, x0 = _gemm_inputs(M, C, Kh, B * T + C)

    def body(ar):
        av = ar.input("a", a, ld=Kh + 8, tile_rows=256)
        wv, bv, gv = ar.input("w", w, tile_rows=256), ar.input("bias", bias), ar.input("gamma", gam)
        out = ar.output("out", (M, C), F32, ld=C + 8, tile_rows=256, preset=x0)
        grid = ar.output("grid", (B, T - 1, C), BF, tile_rows=256)
        ar.arm()
        _lib.gemm(av, wv, bv, _lib.SD_EPI_RESID, out=out, gamma=gv, tokens=T, grid_out=grid)

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert torch.equal(plain["grid"], plain["out"].view(B, T, C)[:, 1:].to(BF))


def _qkv_body(ar, B, T, H, call):
    Tp = (T + 63) // 64 * 64 + 64
    q = ar.output("q", (B, H, T, 64), BF, tile_rows=256)
    # the caller zeroes k and vt once; rows / columns T..Tp-1 are contract padding and stay zero
    k = ar.output("k", (B, H, Tp, 64), BF, tile_rows=256, preset=torch.zeros(B, H, Tp, 64, dtype=BF))
    vt = ar.output("vt", (B, H, 64, Tp), BF, tile_rows=256, preset=torch.zeros(B, H, 64, Tp, dtype=BF))
    ar.arm()
    call(q, k, vt)


def _check_qkv(plain, ref_rows, B, T, H):
    r = ref_rows.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    q, k, vt = plain["q"], plain["k"], plain["vt"]
    assert torch.equal(q, r[0])
    assert torch.equal(k[:, :, :T], r[1])
    assert torch.equal(vt[..., :T], r[2].transpose(-1, -2))
    assert not k[:, :, T:].any() and not vt[..., T:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H", [(2, 77, 2), (1, 65, 6)])
def test_hygiene_gemm_qkv(gpu, B, T, H):
    """SD_EPI_QKV with tokens_pad = ceil64(T) + 64: q is written in full, the pads of k and vt
    stay zero, the bytes behind q, k and vt stay untouched, and the scatter equals the BF16
    epilogue's rows."""
    from scenedino_amd import _lib
    C, M = 64 * H, B * T
    a, w, bias, _, _ = _gemm_inputs(M, 3 * C, C, T + H)

    def body(ar):
        av = ar.input("a", a, ld=C + 8, tile_rows=256)
        wv, bv = ar.input("w", w, tile_rows=256), ar.input("bias", bias)
        _qkv_body(ar, B, T, H, lambda q, k, vt: _lib.gemm(
            av, wv, bv, _lib.SD_EPI_QKV, qkv=(q, k, vt), tokens=T, heads=H))

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    rows = torch.empty(M, 3 * C, device=gpu, dtype=BF)
    _lib.gemm(a.to(gpu), w.to(gpu), bias.to(gpu), _lib.SD_EPI_BF16, out=rows)
    _check_qkv(plain, rows, B, T, H)


@pytest.mark.gpu
@pytest.mark.parametrize("B,P,N,K", [(2, 6, 384, 768), (3, 35, 96, 608)])
def test_hygiene_gemm_patch(gpu, B, P, N, K):
    """SD_EPI_PATCH: rows 1.. of each image are written, the class-token rows (sd_patchify's)
    and the row gaps are not."""
    from scenedino_amd import _lib
    M = B * P
    a, w, bias, _, _ = _gemm_inputs(M, N, K, P + N)
    pos = torch.randn(P + 1, N, generator=torch.Generator().manual_seed(P))

    def body(ar):
        av = ar.input("a", a, ld=K + 8, tile_rows=256)
        wv, bv, pv = ar.input("w", w, tile_rows=256), ar.input("bias", bias), ar.input("pos", pos)
        out = ar.output("out", (B, P + 1, N), F32, ld=N + 8, tile_rows=256, full=False)
        ar.arm()
        _lib.gemm(av, wv, bv, _lib.SD_EPI_PATCH, out=out, pos=pv, patches=P)

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    out = plain["out"]
    assert bool((out[:, 0].view(torch.int32) == sentinel_bits(F32)).all()), "class rows written"
    assert torch.isfinite(out[:, 1:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("B,plane,N,K", [(2, 63, 64, 256), (3, 35, 72, 96), (1, 260, 256, 64)])
def test_hygiene_gemm_nchw(gpu, B, plane, N, K):
    """SD_EPI_NCHW (16-byte stores of four pixels of one channel; plane % 4 != 0 takes the
    scalar path): the dense (B, N, plane) f32 output and nothing behind it."""
    from scenedino_amd import _lib
    M = B * plane
    a, w, bias, _, _ = _gemm_inputs(M, N, K, plane + N)

    def body(ar):
        av = ar.input("a", a, ld=K + 8, tile_rows=256)
        wv, bv = ar.input("w", w, tile_rows=256), ar.input("bias", bias)
        out = ar.output("out", (B, N, plane), F32, tile_rows=256)
        ar.arm()
        g = _lib.SdGemmArgs(a=av.data_ptr(), lda=K + 8 if ar.poison else K, w=wv.data_ptr(),
                            bias=bv.data_ptr(), M=M, N=N, K=K, epi=_lib.SD_EPI_NCHW,
                            out=out.data_ptr(), ldo=N, tokens=plane)
        _lib._check(_lib.load().sd_gemm(ctypes.byref(g), _stream()), "sd_gemm")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    ref = (a.double() @ w.double().t() + bias.double()).view(B, plane, N).transpose(1, 2)
    assert (plain["out"].cpu().double() - ref).abs().max() <= 1e-4 * ref.abs().max() + 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("C", [384, 768])
@pytest.mark.parametrize("M", [1, 33, 77])
@pytest.mark.parametrize("epi", ["BF16", "GELU", "QKV"])
def test_hygiene_ln_gemm(gpu, C, M, epi):
    """sd_ln_gemm's three epilogues at ragged M: x, the LayerNorm parameters and w untouched,
    out (ldo = N + 8) / q, k, vt written only where they should be."""
    from scenedino_amd import _lib
    H = C // 64
    N = 3 * C if epi == "QKV" else 200
    g = torch.Generator().manual_seed(C + M)
    x = 2 * torch.randn(M, C, generator=g) + 0.5
    lw, lb = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    w = (torch.randn(N, C, generator=g) / math.sqrt(C)).to(BF)
    bias = 0.1 * torch.randn(N, generator=g)

    def body(ar):
        xv, lwv, lbv = ar.input("x", x), ar.input("ln_w", lw), ar.input("ln_b", lb)
        wv, bv = ar.input("w", w, tile_rows=256), ar.input("bias", bias)
        if epi == "QKV":
            _qkv_body(ar, 1, M, H, lambda q, k, vt: _lib.ln_gemm(
                xv, lwv, lbv, 1e-6, wv, bv, _lib.SD_EPI_QKV, qkv=(q, k, vt), tokens=M, heads=H))
        else:
            out = ar.output("out", (M, N), BF, ld=N + 8, tile_rows=256)
            ar.arm()
            _lib.ln_gemm(xv, lwv, lbv, 1e-6, wv, bv, getattr(_lib, "SD_EPI_" + epi), out=out)

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    if epi == "QKV":
        rows = torch.empty(M, N, device=gpu, dtype=BF)
        _lib.ln_gemm(x.to(gpu), lw.to(gpu), lb.to(gpu), 1e-6, w.to(gpu), bias.to(gpu),
                     _lib.SD_EPI_BF16, out=rows)
        _check_qkv(plain, rows, 1, M, H)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [68, 384, 1024])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("f32", [False, True])
def test_hygiene_layernorm(gpu, C, rows, f32):
    from scenedino_amd import _lib
    g = torch.Generator().manual_seed(C + rows)
    x = 3 * torch.randn(rows, C, generator=g) + 1
    w, b = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)

    def body(ar):
        xv, wv, bv = ar.input("x", x), ar.input("w", w), ar.input("b", b)
        out = ar.output("out", (rows, C), F32 if f32 else BF)
        ar.arm()
        _lib.layernorm(xv, wv, bv, 1e-6, out)

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    ref = F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-6)
    assert (plain["out"].cpu().double() - ref).abs().max() <= (1e-4 if f32 else 2e-2)


def _token_rows(B, T, C, seed):
    return 2 * torch.randn(B, T, C, generator=torch.Generator().manual_seed(seed)) + 0.3


@pytest.mark.gpu
@pytest.mark.parametrize("C", [96, 384])
@pytest.mark.parametrize("n_prefix", [1, 5])
@pytest.mark.parametrize("l2", [False, True])
def test_hygiene_tokens_to_nhwc(gpu, C, n_prefix, l2):
    """sd_tokens_to_nhwc against its own reference (it is the reference side of two bit-equality
    tests): without l2 bit-equal to x[:, n_prefix:].to(bfloat16); with l2 |got - ref| <=
    2^-8 |ref| + 1e-6 against F.normalize in float64 (bf16 unit roundoff plus a few f32 ulps,
    |ref| <= 1)."""
    from scenedino_amd import _lib
    B, npix = 2, 7
    T = n_prefix + npix
    x = _token_rows(B, T, C, C + n_prefix)

    def body(ar):
        xv = ar.input("x", x)
        out = ar.output("out", (B, npix, C), BF)
        ar.arm()
        _lib._check(_lib.load().sd_tokens_to_nhwc(_p(xv), B, T, C, n_prefix, npix, int(l2), _p(out),
                                                  _stream()), "sd_tokens_to_nhwc")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    got = plain["out"].cpu()
    if not l2:
        assert torch.equal(got, x[:, n_prefix:].to(BF))
    else:
        ref = F.normalize(x[:, n_prefix:].double(), dim=-1, eps=1e-12)
        assert bool(((got.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-6).all())


@pytest.mark.gpu
@pytest.mark.parametrize("C", [96, 384])
@pytest.mark.parametrize("l2", [False, True])
def test_hygiene_layernorm_nhwc(gpu, C, l2):
    from scenedino_amd import _lib
    B, n_prefix, npix = 2, 5, 7
    T = n_prefix + npix
    x = _token_rows(B, T, C, C)
    g = torch.Generator().manual_seed(C)
    w, b = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)

    def body(ar):
        xv, wv, bv = ar.input("x", x), ar.input("w", w), ar.input("b", b)
        out = ar.output("out", (B, npix, C), BF)
        ar.arm()
        _lib._check(_lib.load().sd_layernorm_nhwc(_p(xv), B, T, C, _p(wv), _p(bv), 1e-6, n_prefix,
                                                  npix, int(l2), _p(out), _stream()),
                    "sd_layernorm_nhwc")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    ref = F.layer_norm(x[:, n_prefix:].double(), (C,), w.double(), b.double(), 1e-6)
    if l2:
        ref = F.normalize(ref, dim=-1, eps=1e-12)
    assert (plain["out"].cpu().double() - ref).abs().max() <= 2e-2  # test_layernorm's bf16 bound


@pytest.mark.gpu
@pytest.mark.parametrize("C", [68, 1100])  # 1100 takes the C > 1024 branch
@pytest.mark.parametrize("l2", [False, True])
def test_hygiene_tokens_to_grid(gpu, C, l2):
    from scenedino_amd import _lib
    B, n_prefix, gh, gw = 2, 1, 8, 8
    T = n_prefix + gh * gw  # 65 tokens
    x = _token_rows(B, T, C, C)

    def body(ar):
        xv = ar.input("x", x)
        out = ar.output("out", (B, C, gh, gw), F32)
        ar.arm()
        _lib._check(_lib.load().sd_tokens_to_grid(_p(xv), B, T, C, n_prefix, gh, gw, int(l2), _p(out),
                                                  _stream()), "sd_tokens_to_grid")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    ref = x[:, n_prefix:].double()
    if l2:
        ref = F.normalize(ref, dim=-1, eps=1e-12)
    ref = ref.transpose(1, 2).reshape(B, C, gh, gw)
    assert (plain["out"].cpu().double() - ref).abs().max() <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,p", [(32, 48, 16), (28, 42, 14)])
def test_hygiene_patchify(gpu, H, W, p):
    """sd_patchify against torch float64: |got - ref| <= 2^-8 |ref| + 2e-6 against
    ((x / 2 + 0.5) - mean) / std unfolded in c p^2 + ky p + kx order, columns >= 3 p^2 exactly
    zero, the class rows bit-equal to the f32 cls + pos[0], no other row of x written."""
    from scenedino_amd import _lib
    B, C = 2, 96
    Np = (H // p) * (W // p)
    K = 3 * p * p
    Kp = (K + 31) // 32 * 32
    g = torch.Generator().manual_seed(p)
    img = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    cls, pos = torch.randn(C, generator=g), torch.randn(Np + 1, C, generator=g)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

    def body(ar):
        iv, cv, pv = ar.input("img", img), ar.input("cls", cls), ar.input("pos", pos)
        patches = ar.output("patches", (B * Np, Kp), BF)
        x = ar.output("x", (B, Np + 1, C), F32, full=False)
        ar.arm()
        _lib.patchify(iv, p, Kp, mean, std, patches, cv, pv, x)

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    x = plain["x"].cpu()
    assert torch.equal(x[:, 0], (cls + pos[0]).expand(B, C))
    assert bool((x[:, 1:].contiguous().view(torch.int32) == sentinel_bits(F32)).all())
    m = torch.tensor([float(ctypes.c_float(v).value) for v in mean], dtype=torch.float64).view(1, 3, 1, 1)
    s = torch.tensor([float(ctypes.c_float(v).value) for v in std], dtype=torch.float64).view(1, 3, 1, 1)
    ref = F.unfold(((img.double() / 2 + 0.5) - m) / s, p, stride=p).transpose(1, 2).reshape(B * Np, K)
    got = plain["patches"].cpu().double()
    assert bool(((got[:, :K] - ref).abs() <= 2.0 ** -8 * ref.abs() + 2e-6).all())
    assert not got[:, K:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,T", [(2, 2, 33), (1, 3, 65)])
def test_hygiene_attention_bwd(gpu, B, H, T):
    """sd_attention_bwd with tokens_pad = ceil64(T) + 64: d_qkv written in full, work of exactly
    2 B heads T floats, every input (the zero pads of k and vt included) untouched."""
    from scenedino_amd import _lib
    Tp = (T + 63) // 64 * 64 + 64
    g = torch.Generator().manual_seed(T)
    q = torch.randn(B, H, T, 64, generator=g).to(BF)
    k = torch.zeros(B, H, Tp, 64, dtype=BF)
    k[:, :, :T] = torch.randn(B, H, T, 64, generator=g).to(BF)
    vt = torch.zeros(B, H, 64, Tp, dtype=BF)
    vt[..., :T] = torch.randn(B, H, 64, T, generator=g).to(BF)
    ao = torch.randn(B * T, H * 64, generator=g).to(BF)
    d_ao = torch.randn(B * T, H * 64, generator=g).to(BF)

    def body(ar):
        v = {n: ar.input(n, t) for n, t in (("q", q), ("k", k), ("vt", vt), ("ao", ao), ("d_ao", d_ao))}
        out = ar.output("d_qkv", (B * T, 3 * H * 64), BF)
        work = ar.work("work", 2 * B * H * T)
        ar.arm()
        a = _lib.SdAttnBwdArgs(q=v["q"].data_ptr(), k=v["k"].data_ptr(), vt=v["vt"].data_ptr(),
                               ao=v["ao"].data_ptr(), d_ao=v["d_ao"].data_ptr(),
                               d_qkv=out.data_ptr(), work=work.data_ptr(), B=B, heads=H, tokens=T,
                               tokens_pad=Tp, head_dim=64, scale=0.125)
        _lib._check(_lib.load().sd_attention_bwd(ctypes.byref(a), _stream()), "sd_attention_bwd")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert torch.isfinite(plain["d_qkv"].float()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,C", [(5, 68), (77, 384), (300, 1024)])
@pytest.mark.parametrize("nparts", [None, 1])
@pytest.mark.parametrize("dy_f32", [False, True])
def test_hygiene_layernorm_bwd(gpu, rows, C, nparts, dy_f32):
    """sd_layernorm_bwd: dx, dw, db written in full, work of exactly 2 nparts C floats."""
    from scenedino_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(rows + C)
    x = 2 * torch.randn(rows, C, generator=g) + 0.5
    w = 1 + 0.1 * torch.randn(C, generator=g)
    dy = torch.randn(rows, C, generator=g).to(F32 if dy_f32 else BF)
    npt = int(lib.sd_layernorm_bwd_parts(rows)) if nparts is None else nparts

    def body(ar):
        xv, wv, dv = ar.input("x", x), ar.input("w", w), ar.input("dy", dy)
        dx = ar.output("dx", (rows, C), F32)
        dw, db = ar.output("dw", (C,), F32), ar.output("db", (C,), F32)
        work = ar.work("work", 2 * npt * C)
        ar.arm()
        a = _lib.SdLnBwdArgs(x=xv.data_ptr(), w=wv.data_ptr(), dy=dv.data_ptr(), rows=rows, C=C,
                             dy_f32=int(dy_f32), accumulate=0, nparts=npt, eps=1e-6,
                             dx=dx.data_ptr(), work=work.data_ptr(), dw=dw.data_ptr(),
                             db=db.data_ptr())
        _lib._check(lib.sd_layernorm_bwd(ctypes.byref(a), _stream()), "sd_layernorm_bwd")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    # db = sum over rows of dy in f32: the worst case of any summation order, rows u sum |dy|
    bound = rows * 2.0 ** -24 * dy.double().abs().sum(0) + 1e-30
    assert bool(((plain["db"].cpu().double() - dy.double().sum(0)).abs() <= bound).all())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 2056, 5000])
def test_hygiene_gelu_bwd(gpu, n):
    from scenedino_amd import _lib
    g = torch.Generator().manual_seed(n)
    u, dh = torch.randn(n, generator=g).to(BF), torch.randn(n, generator=g).to(BF)

    def body(ar):
        uv, dv = ar.input("u", u), ar.input("dh", dh)
        out = ar.output("du", (n,), BF)
        ar.arm()
        _lib._check(_lib.load().sd_gelu_bwd(_p(uv), _p(dv), n, _p(out), _stream()), "sd_gelu_bwd")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert torch.isfinite(plain["du"].float()).all()


@pytest.mark.gpu
def test_hygiene_arena_reports_on_the_device(gpu):
    """The arena sees a stray device write: a torch "kernel" that stores one element into the
    row gap behind the payload's first row, and one that leaves an element unwritten."""
    def body(ar, stray):
        out = ar.output("out", (3, 5), F32, ld=8)
        ar.arm()
        out.fill_(1.0)
        if ar.poison and stray == "gap":
            out.as_strided((1,), (1,), out.storage_offset() + 6).fill_(2.0)
        if ar.poison and stray == "unwritten":
            out.view(torch.int32)[2, 4] = sentinel_bits(F32)

    assert run3(gpu, lambda ar: body(ar, None))[0] == []
    assert sum("row gap" in f for f in run3(gpu, lambda ar: body(ar, "gap"))[0]) == 2
    assert sum("never written" in f for f in run3(gpu, lambda ar: body(ar, "unwritten"))[0]) == 2
