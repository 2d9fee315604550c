"""Memory hygiene of the DPT decoder kernels (sd_gemm's convolution routes in sdhip_vit.hip /
sdhip_conv.hip, sdhip_dpt_bwd.hip): outputs behind guard bands, inputs between poisoned
margins (tests/_arena.py), and the float64 reference of sd_upsample2x at its two shapes."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from _arena import assert_clean, run3

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


def _conv_case(gpu, B, H, W, Cin, Cout, stride=1, relu_in=False, epi="BF16", res=0, seed=0):
    """One 3x3 convolution through sd_gemm with ldo = Cout + 8 (NCHW: dense).  Returns the plain
    run's output and the CPU operands."""
    from scenedino_amd import _lib
    g = torch.Generator().manual_seed(seed + H * W + Cout)
    x = torch.randn(B, H, W, Cin, generator=g).to(BF)
    w = (torch.randn(Cout, 9 * Cin, generator=g) / math.sqrt(9 * Cin)).to(BF)
    bias = 0.1 * torch.randn(Cout, generator=g)
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = B * OH * OW
    rs = [torch.randn(M, Cout, generator=g).to(BF) for _ in range(res)]
    nchw = epi == "NCHW"

    def body(ar):
        xv, wv, bv = ar.input("x", x, tile_rows=256), ar.input("w", w, tile_rows=256), ar.input("bias", bias)
        ldo = Cout + 8 if (ar.poison and not nchw) else Cout
        rv = [ar.input(f"res{i}", r, ld=ldo, tile_rows=256) for i, r in enumerate(rs)]
        if nchw:
            out = ar.output("out", (B, Cout, OH * OW), F32, tile_rows=256)
        else:
            out = ar.output("out", (M, Cout), F32 if epi == "F32" else BF, ld=ldo, tile_rows=256)
        ar.arm()
        a = _lib.SdGemmArgs(a=xv.data_ptr(), lda=9 * Cin, w=wv.data_ptr(), bias=bv.data_ptr(), M=M,
                            N=Cout, K=9 * Cin, epi=getattr(_lib, "SD_EPI_" + epi),
                            out=out.data_ptr(), ldo=ldo,
                            res=rv[0].data_ptr() if res > 0 else None,
                            res2=rv[1].data_ptr() if res > 1 else None,
                            conv=1, H=H, W=W, Cin=Cin, stride=stride, OH=OH, OW=OW,
                            relu_in=int(relu_in), tokens=OH * OW)
        _lib._check(_lib.load().sd_gemm(ctypes.byref(a), _stream()), "sd_gemm(conv3x3)")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert torch.isfinite(plain["out"].float()).all()
    return plain["out"], (x, w, bias, rs)


def _conv_ref(x, w, bias, rs, stride, relu_in):
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    xi = x.double().permute(0, 3, 1, 2)
    if relu_in:
        xi = xi.relu()
    wt = w.double().view(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    y = F.conv2d(xi, wt, bias.double(), stride=stride, padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
    for r in rs:
        y = y + r.double()
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("variant", ["plain", "relu_res", "relu_res2", "f32", "nchw"])
def test_hygiene_conv3x3_k_gemm(gpu, stride, variant):
    """conv3x3 on the k_gemm path ((2, 7, 9, 64 -> 128): far too few tiles for the big ones)."""
    kw = {"plain": {}, "relu_res": dict(relu_in=True, res=1), "relu_res2": dict(relu_in=True, res=2),
          "f32": dict(epi="F32"), "nchw": dict(epi="NCHW")}[variant]
    out, (x, w, bias, rs) = _conv_case(gpu, 2, 7, 9, 64, 128, stride=stride, **kw)
    ref = _conv_ref(x, w, bias, rs, stride, kw.get("relu_in", False))
    got = out.cpu().double()
    if variant == "nchw":
        got = got.transpose(1, 2).reshape(-1, 128)
    # test_vit's sd_gemm bound: 1e-4 of the output scale for f32 epilogues, 8e-3 for bf16 ones
    tol = 8e-3 if kw.get("epi", "BF16") == "BF16" else 1e-4
    assert (got - ref).abs().max() <= tol * ref.abs().max() + 1e-5


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ragged_hw(min_pixels, min_w=33):
    """The smallest H x W >= min_pixels near 1 : 3 with H % 8 != 0 and W % 32 != 0."""
    H = max(3, int(math.sqrt(min_pixels / 3.0)))
    if H % 8 == 0:
        H += 1
    W = max(min_w, -(-min_pixels // H))
    if W % 32 == 0:
        W += 1
    return H, W


def _im2col_min_pixels(bm, bn, cout, ncu):
    """Fewest output pixels at which sd_conv_big_try's im2col rule picks bm x bn tiles: the
    first of 256 x 256 (>= 15/8 tiles per CU), 256 x 128, 128 x 128, 128 x 64 (>= 7/8)."""
    need = ncu * 15 // 8 if (bm, bn) == (256, 256) else ncu * 7 // 8
    rows = -(-need // (cout // bn))          # row tiles needed
    return (rows - 1) * bm + 1


@pytest.mark.gpu
@pytest.mark.parametrize("bm,bn", [(128, 64), (128, 128), (256, 128), (256, 256)])
@pytest.mark.parametrize("variant", ["relu_res", "f32"])
def test_hygiene_conv3x3_im2col_tiles(gpu, bm, bn, variant, monkeypatch):
    """Each im2col tile of k_conv_big (SD_CONV_BIG=b, as test_conv3x3_big_tiles forces them) at
    the smallest ragged H x W that sd_conv_big_try sends there on this device (Cout = 256:
    with 256 CUs the 128 x 64 tiles need 7041 output pixels)."""
    monkeypatch.setenv("SD_CONV_BIG", "b")
    ncu = _cus()
    H, W = _ragged_hw(_im2col_min_pixels(bm, bn, 256, ncu))
    # the shape must not already qualify for the next larger tile
    tiles = lambda m, n: -(-(H * W) // m) * (256 // n)
    order = [(256, 256), (256, 128), (128, 128), (128, 64)]
    for m, n in order[:order.index((bm, bn))]:
        assert tiles(m, n) < (ncu * 15 // 8 if (m, n) == (256, 256) else ncu * 7 // 8)
    kw = dict(relu_in=True, res=1) if variant == "relu_res" else dict(epi="F32")
    _conv_case(gpu, 1, H, W, 64, 256, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("hbn", [128, 256])
@pytest.mark.parametrize("variant", ["relu_res", "f32"])
def test_hygiene_conv3x3_halo_tiles(gpu, hbn, variant, monkeypatch):
    """The 8 x 32 halo tiles of k_conv_halo at the smallest ragged shape the default routing
    sends there: 128 channels per tile where ceil(OH / 8) ceil(OW / 32) (Cout / 128) >= 7/8 of
    the CUs and the 256 x 256 im2col tiles would not cover them 15/8 times; all 256 channels
    where they would."""
    monkeypatch.delenv("SD_CONV_BIG", raising=False)
    ncu = _cus()
    if hbn == 128:
        need = -(-(ncu * 7 // 8) // 2)                 # 8 x 32 pixel tiles
        th = max(2, int(math.sqrt(need / 2.0)))
        tw = -(-need // th)
        H, W = 8 * (th - 1) + 1, 32 * (tw - 1) + 1     # ragged: one row / column into the last tile
        assert -(-(H * W) // 256) < ncu * 15 // 8
    else:
        H, W = _ragged_hw((ncu * 15 // 8 - 1) * 256 + 1)
    kw = dict(relu_in=True, res=1) if variant == "relu_res" else dict(epi="F32")
    _conv_case(gpu, 1, H, W, 64, 256, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,big", [("plain", False), ("shuf2", False), ("shuf4", False),
                                         ("res", False), ("plain", True), ("shuf2", True),
                                         ("shuf4", True)])
def test_hygiene_linear_nhwc(gpu, variant, big, monkeypatch):
    """1x1 convolution / ConvTranspose2d(k, stride k) rows through sd_gemm: small (k_gemm) and,
    for the routes k_conv_big takes (no residual), at its 128 x 64 threshold."""
    from scenedino_amd import _lib
    monkeypatch.delenv("SD_CONV_BIG", raising=False)
    shuf = {"shuf2": 2, "shuf4": 4}.get(variant)
    Cin, N = 64, 128
    if big:
        B, (H, W) = 1, _ragged_hw(_im2col_min_pixels(128, 64, N, _cus()))
    else:
        B, H, W = 2, 5, 3
    M = B * H * W
    g = torch.Generator().manual_seed(M + (shuf or 0))
    x = torch.randn(B, H, W, Cin, generator=g).to(BF)
    w = (torch.randn(N, Cin, generator=g) / 8).to(BF)
    bias = 0.1 * torch.randn(N, generator=g)
    res = torch.randn(B, H, W, N, generator=g).to(BF) if variant == "res" else None

    def body(ar):
        xv, wv, bv = ar.input("x", x, tile_rows=256), ar.input("w", w, tile_rows=256), ar.input("bias", bias)
        rv = ar.input("res", res, tile_rows=256) if res is not None else None
        if shuf:
            out = ar.output("out", (B, H * shuf, W * shuf, N // (shuf * shuf)), BF, tile_rows=256)
        else:
            out = ar.output("out", (B, H, W, N), BF, tile_rows=256)
        ar.arm()
        _lib.linear_nhwc(xv, wv, bv, out=out, shuf=shuf, res=rv)

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    y = x.double().view(M, Cin) @ w.double().t() + bias.double()
    if res is not None:
        y = y + res.double().view(M, N)
    if shuf:
        co = N // (shuf * shuf)
        y = y.view(B, H, W, shuf, shuf, co).permute(0, 1, 3, 2, 4, 5).reshape(B, H * shuf, W * shuf, co)
    got = plain["out"].cpu().double().reshape(y.shape)
    assert (got - y).abs().max() <= 8e-3 * y.abs().max()  # test_vit's bf16-epilogue bound


UP_SHAPES = [(1, 1, 1, 8), (2, 5, 3, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,C", UP_SHAPES)
def test_hygiene_upsample2x(gpu, B, H, W, C):
    """sd_upsample2x: |got - ref| <= 2^-8 |ref| + 2^-20 max|x| against F.interpolate(...,
    align_corners=True) in float64 (bf16 output rounding plus f32 interpolation error)."""
    from scenedino_amd import _lib
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(H * W + C)).to(BF)

    def body(ar):
        xv = ar.input("x", x)
        out = ar.output("out", (B, 2 * H, 2 * W, C), BF)
        ar.arm()
        _lib._check(_lib.load().sd_upsample2x(_p(xv), B, H, W, C, _p(out), _stream()), "sd_upsample2x")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    ref = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear",
                        align_corners=True).permute(0, 2, 3, 1)
    got = plain["out"].cpu().double()
    assert bool(((got - ref).abs() <= 2.0 ** -8 * ref.abs() + 2.0 ** -20 * x.double().abs().max()).all())


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,C", UP_SHAPES)
def test_hygiene_upsample2x_bwd(gpu, B, H, W, C):
    from scenedino_amd import _lib
    go = torch.randn(B, 2 * H, 2 * W, C, generator=torch.Generator().manual_seed(H + W + C)).to(BF)

    def body(ar):
        gv = ar.input("gout", go)
        gin = ar.output("gin", (B, H, W, C), BF)
        ar.arm()
        _lib._check(_lib.load().sd_upsample2x_bwd(_p(gv), B, H, W, C, _p(gin), _stream()),
                    "sd_upsample2x_bwd")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert torch.isfinite(plain["gin"].float()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 2048 + 8, 3 * 2048 + 1000])
@pytest.mark.parametrize("with_res", [False, True])
def test_hygiene_relu_bwd(gpu, n, with_res):
    """sd_relu_bwd with n not a multiple of its 2048-element blocks: bit-equal to torch."""
    from scenedino_amd import _lib
    g = torch.Generator().manual_seed(n)
    x, gr = torch.randn(n, generator=g).to(BF), torch.randn(n, generator=g).to(BF)
    res = torch.randn(n, generator=g).to(BF) if with_res else None

    def body(ar):
        xv, gv = ar.input("x", x), ar.input("g", gr)
        rv = ar.input("res", res) if with_res else None
        out = ar.output("out", (n,), BF)
        ar.arm()
        _lib._check(_lib.load().sd_relu_bwd(_p(xv), _p(gv), _p(rv), n, _p(out), _stream()), "sd_relu_bwd")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    ref = torch.where(x > 0, gr, torch.zeros_like(gr)).float()
    if with_res:
        ref = ref + res.float()
    assert torch.equal(plain["out"].cpu(), ref.to(BF))


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 5, 3, 64, 8), (2, 7, 9, 64, 128)])
@pytest.mark.parametrize("taps,stride", [(9, 1), (9, 2), (1, 1), (1, 2)])
@pytest.mark.parametrize("nparts", [None, 1])
def test_hygiene_conv_wgrad(gpu, B, H, W, Cin, Cout, taps, stride, nparts):
    """sd_conv_wgrad (the LDS-DMA weight-gradient kernel reads past the rows it uses, by its own
    account): dw and db written in full, work of exactly sd_conv_wgrad_work floats, NaN behind
    x and dy does not reach the sums."""
    from scenedino_amd import _lib
    lib = _lib.load()
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = torch.Generator().manual_seed(H * W + Cout + taps)
    x = torch.randn(B, H, W, Cin, generator=g).to(BF)
    dy = torch.randn(B, OH, OW, Cout, generator=g).to(BF)
    a0 = _lib.conv_wgrad_args(B, H, W, Cin, Cout, taps, stride, relu_in=True)
    a0.nparts = int(lib.sd_conv_wgrad_parts(ctypes.byref(a0))) if nparts is None else nparts
    assert a0.nparts >= 1
    nwork = int(lib.sd_conv_wgrad_work(ctypes.byref(a0)))
    assert nwork > 0

    def body(ar):
        xv, dv = ar.input("x", x), ar.input("dy", dy)
        dw, db = ar.output("dw", (Cout, taps * Cin), F32), ar.output("db", (Cout,), F32)
        work = ar.work("work", nwork)
        ar.arm()
        a = _lib.conv_wgrad_args(B, H, W, Cin, Cout, taps, stride, relu_in=True, nparts=a0.nparts)
        a.x, a.dy, a.work, a.dw, a.db = (xv.data_ptr(), dv.data_ptr(), work.data_ptr(),
                                         dw.data_ptr(), db.data_ptr())
        _lib._check(lib.sd_conv_wgrad(ctypes.byref(a), _stream()), "sd_conv_wgrad")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    ref = dy.double().sum((0, 1, 2))
    # db sums B OH OW bf16 values in f32: any order stays within n u sum |dy|
    bound = B * OH * OW * 2.0 ** -24 * dy.double().abs().sum((0, 1, 2)) + 1e-30
    assert bool(((plain["db"].cpu().double() - ref).abs() <= bound).all())
    assert torch.isfinite(plain["dw"]).all()
