"""Memory hygiene of the render / field / training-MLP kernels: outputs and scratch behind
guard bands, inputs between poisoned margins (tests/_arena.py), plus the direct references of
sd_pack_image and sd_cast_grid (bit-equal to the torch permute / cast).

The renders and the field query are awkward to set up by hand, so the model's own call is
used: the `_lib` function is monkeypatched for that one call, re-points the output, scratch
and ld_* fields of the struct to arena views and then calls the real function."""
import ctypes
import math

import pytest
import torch

from _arena import assert_clean, run3
from _helpers import build_net, load, net_from_fixture

F32, F16, BF = torch.float32, torch.float16, torch.bfloat16
KN = torch.tensor([[0.7849, 0.0, -0.0312], [0.0, 2.9391, 0.2701], [0.0, 0.0, 1.0]])


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


def T(a, dev="cuda"):
    return torch.as_tensor(a).to(dev)


# --------------------------------------------------------------------------- renders
def _render_case(gpu, monkeypatch, net, rays, z, sb, hard, proj):
    """net.render_fused(rays, z) with sd_render_proj / sd_render_fused writing into arena views:
    proj: depth / dino / rgb as one packed row per ray with at least four slack floats
    (ld = D + 1 + 3 nv + 4, rounded up to a multiple of 4) and work of exactly sd_render_proj_work_bytes(R, D); every optional
    output requested.  Returns (plain outputs, the NaN run's work buffer)."""
    from scenedino_amd import _lib
    name = "render_proj" if proj else "render_fused"
    real = getattr(_lib, name)
    R, K = z.shape
    keep = {}

    def body(ar):
        rv, zv = ar.input("rays", rays), ar.input("z", z)

        def patched(args, head, ref):
            D, nv = head.D, args.nv
            assert (args.R, args.K) == (R, K)
            if proj:
                wd = D + 1 + 3 * nv
                # four slack floats, rounded up so that ld_dino % 4 == 0 as the header requires
                # (nv = 1: exactly D + 1 + 3 nv + 4)
                ld = (wd + 4 + 3) // 4 * 4
                maps = ar.output("maps", (R, wd), F32, ld=ld)
                # (the plain run's tight rows are no multiple of 4 floats wide at nv = 2: it
                # renders into ordinary padded rows that are copied out below)
                rows = maps if ar.poison else torch.empty(R, ld, device=maps.device)
                args.dino, args.depth, args.rgb = (rows.data_ptr(), rows[:, D:].data_ptr(),
                                                   rows[:, D + 1:].data_ptr())
                args.ld_dino = args.ld_depth = args.ld_rgb = ld
                wb = _lib.render_proj_work_bytes(R, D)
                assert wb % 4 == 0
                if wb > 0:
                    work = ar.work("work", wb // 4)
                    args.work = work.data_ptr()
                    if ar.poison == "nan":
                        keep["work"] = work
            else:
                args.depth = ar.output("depth", (R,), F32).data_ptr()
                args.dino = ar.output("dino", (R, D), F32).data_ptr()
                args.rgb = ar.output("rgb", (R, 3 * nv), F32).data_ptr()
            args.weights = ar.output("weights", (R, K), F32).data_ptr()
            args.alphas = ar.output("alphas", (R, K), F32).data_ptr()
            args.invalid = ar.output("invalid", (R, K, nv), F32).data_ptr()
            args.invalid_f = ar.output("invalid_f", (R, K), torch.uint8).data_ptr()
            args.rgb_samps = ar.output("rgb_samps", (R, K, 3 * nv), F32).data_ptr()
            ar.arm()
            real(args, head, ref)
            if proj and not ar.poison:
                maps.copy_(rows[:, :wd])

        monkeypatch.setattr(_lib, name, patched)
        try:
            with torch.no_grad():
                net.render_fused(rv, zv, sb, hard, want_weights=True, want_alphas=True,
                                 want_rgb_samps=True)
        finally:
            monkeypatch.setattr(_lib, name, real)

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    for k, v in plain.items():
        assert torch.isfinite(v.float()).all(), k
    return plain, keep.get("work")


def _k16_case(precision, mode, n=762):
    from scenedino_amd import _lib
    d = load("render_sb2_nv2_k16.npz")
    net = net_from_fixture(d, precision, mode=mode)
    rays = T(d["rays"])[:, :n].reshape(2 * n, -1).contiguous()
    u = T(d["u"]).view(2, 768, -1)[:, :n].reshape(2 * n, -1).contiguous()
    z = _lib.sample_z(rays, int(d["K"]), True, u=u)
    return net, rays.cpu(), z.cpu(), bool(d["hard_cap"])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_hygiene_render_proj(gpu, monkeypatch, precision):
    """sd_render_proj on the k16 fixture (two super-batches, two colour views), R = 1524 (not a
    multiple of 64), packed rows with slack."""
    net, rays, z, hard = _k16_case(precision, "proj")
    plain, _ = _render_case(gpu, monkeypatch, net, rays, z, 2, hard, proj=True)
    assert plain["maps"].shape == (1524, 64 + 1 + 6)


def _synthetic_net(precision, D, H, W, seed, offset=False, grid_hw=None):
    from scenedino_amd.common.ray_sampler import ImageRaySampler
    g = torch.Generator().manual_seed(seed)
    C = 256
    images = torch.rand(1, 1, 3, H, W, generator=g) * 2 - 1
    gh, gw = grid_hw or (H // 2, W // 2)
    grid = torch.randn(1, C, gh, gw, generator=g)
    W_in = torch.randn(128, C + 39, generator=g) * 0.06
    b_in = torch.randn(128, generator=g) * 0.1
    W_out = torch.randn(1 + D, 128, generator=g) * 0.1
    b_out = torch.randn(1 + D, generator=g) * 0.1
    Kn = KN.view(1, 1, 3, 3)
    pose = torch.eye(4).view(1, 1, 4, 4)
    rpose = pose.clone()
    if offset:
        a = math.radians(2.0)
        rpose[0, 0, 0, 0] = math.cos(a); rpose[0, 0, 0, 2] = math.sin(a)
        rpose[0, 0, 2, 0] = -math.sin(a); rpose[0, 0, 2, 2] = math.cos(a)
        rpose[0, 0, 0, 3] = 0.5
    net = build_net(grid, W_in, b_in, W_out, b_out, precision, "cuda")
    net.encode(images.cuda(), Kn.cuda(), pose.cuda(), ids_encoder=[0], ids_render=[0])
    rays, _ = ImageRaySampler(3, 80, H, W).sample(None, rpose.cuda(), Kn.cuda())
    return net, rays[0].contiguous(), g


@pytest.mark.gpu
def test_hygiene_render_proj_wide_head(gpu, monkeypatch):
    """D = 384: the hidden-composite scratch in work (R = 12 x 37 = 444 rays)."""
    from scenedino_amd import _lib
    net, rays, g = _synthetic_net("bf16", 384, 12, 37 * 1 + 3, 5)
    rays = rays[:444]
    assert _lib.render_proj_work_bytes(444, 384) > 0
    z = _lib.sample_z(rays, 16, True, u=torch.rand(444, 16, generator=g).cuda())
    _render_case(gpu, monkeypatch, net, rays.cpu(), z.cpu(), 1, False, proj=True)


def _overflow_blocks(work, R):
    """4-ray blocks in the tile kernel's per-workgroup overflow lists: the tail of work is
    [ncu] counts, [ncu][cap] blocks (test_gpu_parity._overflow_blocks)."""
    w = work.view(torch.int32)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    cap = ((R + ncu - 1) // ncu + 64) // 4 + 1
    words = ((4 * (ncu + ncu * cap) + 15) // 16) * 16 // 4
    cnt = w[w.numel() - words:][:ncu]
    assert int(cnt.min()) >= 0 and int(cnt.max()) <= cap
    return int(cnt.sum())


@pytest.mark.gpu
def test_hygiene_render_proj_tile_overflow(gpu, monkeypatch):
    """K = 64 from an offset pose with the tile buffers capped at 16 KiB (sd_render_tile_cap):
    the tile kernel, its overflow list inside work and the per-ray fallback behind it.  The 24 x 80
    rays look into a 96 x 320 grid, four texels apart, so that a ray group's tap box outgrows the
    capped buffers."""
    from scenedino_amd import _lib
    net, rays, g = _synthetic_net("bf16", 64, 24, 80, 264, offset=True, grid_hw=(96, 320))
    R = rays.shape[0] - 10  # 1910: ragged
    rays = rays[:R]
    z = _lib.sample_z(rays, 64, True, u=torch.rand(R, 64, generator=g).cuda())
    prev = _lib.render_tile_cap(16 * 1024)
    try:
        _, work = _render_case(gpu, monkeypatch, net, rays.cpu(), z.cpu(), 1, True, proj=True)
    finally:
        _lib.render_tile_cap(prev)
    assert _overflow_blocks(work, R) > 0, "the cap did not force an overflow"


@pytest.mark.gpu
def test_hygiene_render_fused(gpu, monkeypatch):
    """sd_render_fused (f32) at K = 32, R = 1524."""
    from scenedino_amd import _lib
    d = load("render_sb2_nv2_k16.npz")
    net = net_from_fixture(d, "fp32")
    n = 762
    rays = T(d["rays"])[:, :n].reshape(2 * n, -1).contiguous()
    u = torch.rand(2 * n, 32, generator=torch.Generator().manual_seed(1)).cuda()
    z = _lib.sample_z(rays, 32, True, u=u)
    _render_case(gpu, monkeypatch, net, rays.cpu(), z.cpu(), 2, False, proj=False)


@pytest.mark.gpu
@pytest.mark.parametrize("precision,dino_dtype", [("fp32", F32), ("bf16", F32), ("bf16", BF)])
def test_hygiene_field_query(gpu, monkeypatch, precision, dino_dtype):
    """sd_field_query with P = 4001 (ragged 32-point tiles), f32 and bf16 dino."""
    from scenedino_amd import _lib
    d = load("field_query.npz")
    net = net_from_fixture(d, precision)
    xyz = torch.as_tensor(d["xyz"])[:, :4001].contiguous()
    P = 4001
    real = _lib.field_query

    def body(ar):
        xv = ar.input("xyz", xyz)

        def patched(args, mlp, ref):
            D, nv = mlp.D, args.nv
            args.sigma = ar.output("sigma", (1, P), F32).data_ptr()
            args.dino = ar.output("dino", (1, P, D), dino_dtype).data_ptr()
            args.rgb = ar.output("rgb", (1, P, 3 * nv), F32).data_ptr()
            args.invalid = ar.output("invalid", (1, P, nv), F32).data_ptr()
            args.invalid_f = ar.output("invalid_f", (1, P), torch.uint8).data_ptr()
            ar.arm()
            real(args, mlp, ref)

        monkeypatch.setattr(_lib, "field_query", patched)
        try:
            with torch.no_grad():
                net.query(xv, colors=True, dino_dtype=dino_dtype)
        finally:
            monkeypatch.setattr(_lib, "field_query", real)

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert torch.equal(plain["invalid"].cpu(), torch.from_numpy(d["invalid"])[:, :P])


# --------------------------------------------------------------------------- compositing
def _comp_inputs(R, K, F, Cc, seed):
    from test_train import _comp_inputs as ci
    return ci(R, K, F, Cc, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("hard", [False, True])
def test_hygiene_composite(gpu, hard):
    from scenedino_amd import _lib
    R, K, Fd, Cc = 37, 100, 30, 6
    z, sigma, feat, rgb, _ = (t.float() if torch.is_tensor(t) else t for t in _comp_inputs(R, K, Fd, Cc, 3))

    def body(ar):
        zv, sv, fv, cv = ar.input("z", z), ar.input("sigma", sigma), ar.input("feat", feat), ar.input("rgb", rgb)
        w, a = ar.output("weights", (R, K), F32), ar.output("alphas", (R, K), F32)
        dp, fo, ro = ar.output("depth", (R,), F32), ar.output("feat_out", (R, Fd), F32), ar.output("rgb_out", (R, Cc), F32)
        ar.arm()
        _lib._check(_lib.load().sd_composite(_p(zv), _p(sv), _p(fv), Fd, _p(cv), Cc, R, K, int(hard),
                                             _p(w), _p(a), _p(dp), _p(fo), _p(ro), _stream()), "sd_composite")

    findings, plain = run3(gpu, body)
    assert_clean(findings)


@pytest.mark.gpu
@pytest.mark.parametrize("hard", [False, True])
def test_hygiene_composite_bwd(gpu, hard):
    """sd_composite_bwd at K = 100, F = 30 (neither a multiple of the wave)."""
    from scenedino_amd import _lib
    R, K, Fd, Cc = 37, 100, 30, 6
    z, sigma, feat, rgb, gr = _comp_inputs(R, K, Fd, Cc, 4)
    ins = {"z": z, "sigma": sigma, "feat": feat, "rgb": rgb, "g_depth": gr["depth"], "g_feat": gr["dino"],
           "g_rgb": gr["rgb"], "g_weights": gr["weights"], "g_alphas": gr["alphas"]}
    ins = {k: v.float() for k, v in ins.items()}

    def body(ar):
        v = {k: ar.input(k, t) for k, t in ins.items()}
        ds, df, dc = ar.output("d_sigma", (R, K), F32), ar.output("d_feat", (R, K, Fd), F32), ar.output("d_rgb", (R, K, Cc), F32)
        ar.arm()
        _lib._check(_lib.load().sd_composite_bwd(
            _p(v["z"]), _p(v["sigma"]), _p(v["feat"]), Fd, _p(v["rgb"]), Cc, R, K, int(hard),
            _p(v["g_depth"]), _p(v["g_feat"]), _p(v["g_rgb"]), _p(v["g_weights"]), _p(v["g_alphas"]),
            _p(ds), _p(df), _p(dc), _stream()), "sd_composite_bwd")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert all(torch.isfinite(t).all() for t in plain.values())


# --------------------------------------------------------------------------- training gather
def _gather(seed, P):
    from test_train import _gather_case
    return _gather_case(seed, B=2, P=P, C=64, Hf=5, Wf=7)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, F16])
def test_hygiene_field_gather(gpu, dt):
    from scenedino_amd import _lib
    P = 333
    grid, xyz, w2c, Ks = _gather(5, P)
    B, C, Hf, Wf = grid.shape
    gn = grid.permute(0, 2, 3, 1).contiguous()
    cam = _lib.cam_records(w2c.cuda(), Ks.cuda()).cpu()
    img = torch.rand(B, 9, 11, 4, generator=torch.Generator().manual_seed(1))

    def body(ar):
        xv, gv, cv, iv = ar.input("xyz", xyz), ar.input("grid", gn), ar.input("cam", cam), ar.input("img", img)
        x = ar.output("x", (B, P, C + 40), dt)
        invf = ar.output("invalid_f", (B, P), torch.uint8)
        rgb, inv = ar.output("rgb", (B, P, 3), F32), ar.output("invalid", (B, P, 1), F32)
        ar.arm()
        _lib._check(_lib.load().sd_field_gather(
            _p(xv), B, P, _p(gv), C, Hf, Wf, _p(cv), _p(iv), 1, 9, 11, _p(cv), _p(x),
            _lib.SD_OF_TORCH[dt], _p(invf), _p(rgb), _p(inv), _stream()), "sd_field_gather")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert bool((plain["x"][..., -1] == 1).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, F16])
def test_hygiene_field_gather_bwd(gpu, dt):
    """sd_field_gather_bwd with ldx = C + 48 > C + 40; dgrid is zeroed by the caller and
    accumulated into with f32 atomics: the three runs agree within rel_l2 < 1e-5
    (test_field_gather_fwd_bwd_gpu's bound)."""
    from scenedino_amd import _lib
    P = 333
    grid, xyz, w2c, Ks = _gather(6, P)
    B, C, Hf, Wf = grid.shape
    cam = _lib.cam_records(w2c.cuda(), Ks.cuda()).cpu()
    dx = torch.randn(B, P, C, generator=torch.Generator().manual_seed(2)).to(dt)

    def body(ar):
        xv, cv = ar.input("xyz", xyz), ar.input("cam", cam)
        dv = ar.input("dx", dx, ld=C + 48)
        dg = ar.output("dgrid", (B, Hf, Wf, C), F32, preset=torch.zeros(B, Hf, Wf, C))
        ar.arm()
        _lib._check(_lib.load().sd_field_gather_bwd(
            _p(xv), B, P, _p(dv), _lib.SD_OF_TORCH[dt], dv.stride(1), C, Hf, Wf, _p(cv), _p(dg),
            _stream()), "sd_field_gather_bwd")

    findings, plain = run3(gpu, body, atomic_rel_l2=1e-5)
    assert_clean(findings)
    assert plain["dgrid"].abs().sum() > 0


# --------------------------------------------------------------------------- rays, z, patches
def _cams(n, seed):
    g = torch.Generator().manual_seed(seed)
    poses = torch.eye(4).repeat(n, 1, 1) + 0.1 * torch.randn(n, 4, 4, generator=g)
    poses[:, 3] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    return poses, KN.repeat(n, 1, 1) + 0.05 * torch.rand(n, 3, 3, generator=g)


@pytest.mark.gpu
def test_hygiene_gen_rays(gpu):
    from scenedino_amd import _lib
    n, H, W = 2, 5, 13
    poses, Ks = _cams(n, 1)
    ids = torch.arange(n, dtype=F32)

    def body(ar):
        pv, kv, iv = ar.input("poses", poses), ar.input("Ks", Ks), ar.input("ids", ids)
        out = ar.output("rays", (n, H, W, 11), F32)
        ar.arm()
        _lib._check(_lib.load().sd_gen_rays(_p(pv), _p(kv), _p(iv), n, H, W, 3.0, 80.0, _p(out), _stream()),
                    "sd_gen_rays")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert torch.equal(plain["rays"], _lib.gen_rays(poses.cuda(), Ks.cuda(), ids.cuda(), H, W, 3.0, 80.0))


@pytest.mark.gpu
@pytest.mark.parametrize("use_u", [False, True])
def test_hygiene_sample_z(gpu, use_u):
    """sd_sample_z with R K = 37 x 19 (not a multiple of 256), jitter from u and from the RNG."""
    from scenedino_amd import _lib
    R, K = 37, 19
    g = torch.Generator().manual_seed(9)
    rays = torch.randn(R, 11, generator=g)
    rays[:, 6], rays[:, 7] = 3.0, 80.0
    u = torch.rand(R, K, generator=g)

    def body(ar):
        rv = ar.input("rays", rays)
        uv = ar.input("u", u) if use_u else None
        out = ar.output("z", (R, K), F32)
        ar.arm()
        _lib.sample_z(rv, K, True, u=uv, seed=5, offset=3, out=out)

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    z = plain["z"]
    assert bool((z[:, 1:] > z[:, :-1]).all()) and float(z.min()) >= 3.0 and float(z.max()) <= 80.0


@pytest.mark.gpu
@pytest.mark.parametrize("upscaled", [False, True])
def test_hygiene_patch_rays(gpu, upscaled):
    from scenedino_amd import _lib
    B, V, H, W, npat, ph, pw, ch, dc = 2, 2, 16, 24, 5, 4, 4, 3, 20
    dh, dw = (H, W) if upscaled else (H // 4, W // 4)
    g = torch.Generator().manual_seed(11)
    poses, Ks = _cams(B * V, 2)
    ids = torch.arange(V, dtype=F32)
    images = torch.rand(B, V, ch, H, W, generator=g)
    dino = torch.randn(B, V, dc, dh, dw, generator=g)
    cy, cx = torch.randint(0, H // 4, (B, npat), generator=g), torch.randint(0, W // 4, (B, npat), generator=g)
    patches = torch.stack((torch.randint(0, V, (B, npat), generator=g), 4 * cy, 4 * cx,
                           cy * (W // 4) + cx), -1).to(torch.int32)
    npts = npat * ph * pw

    def body(ar):
        pv, kv, iv = ar.input("poses", poses), ar.input("Ks", Ks), ar.input("ids", ids)
        tv, mv, dv = ar.input("patches", patches), ar.input("images", images), ar.input("dino", dino)
        rays = ar.output("rays", (B, npts, 11), F32)
        rgb = ar.output("rgb", (B, npts, ch), F32)
        dout = ar.output("dino_out", (B, npts if upscaled else npat, dc), F32)
        ar.arm()
        a = _lib.SdPatchArgs(poses=pv.data_ptr(), Ks=kv.data_ptr(), frame_ids=iv.data_ptr(),
                             patches=tv.data_ptr(), images=mv.data_ptr(), dino=dv.data_ptr(),
                             rays=rays.data_ptr(), rgb_out=rgb.data_ptr(), dino_out=dout.data_ptr(),
                             B=B, V=V, H=H, W=W, n_patches=npat, ph=ph, pw=pw, channels=ch, dino_c=dc,
                             dino_h=dh, dino_w=dw, dino_upscaled=int(upscaled), z_near=3.0, z_far=80.0)
        _lib.patch_rays(a, rays)

    findings, plain = run3(gpu, body)
    assert_clean(findings)


# --------------------------------------------------------------------------- layout kernels
GRID_SHAPES = [(2, 100, 5, 132), (1, 30, 5, 7)]  # (B, C, H, W): both sd_pack_grid kernels


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,H,W", GRID_SHAPES)
@pytest.mark.parametrize("dt", [F32, F16, BF])
def test_hygiene_pack_grid(gpu, B, C, H, W, dt):
    from scenedino_amd import _lib
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(C))

    def body(ar):
        xv = ar.input("grid", x)
        out = ar.output("out", (B, H, W, C), dt)
        ar.arm()
        _lib._check(_lib.load().sd_pack_grid(_p(xv), B, C, H, W, _lib.SD_OF_TORCH[dt], _p(out), _stream()),
                    "sd_pack_grid")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert torch.equal(plain["out"].cpu(), x.permute(0, 2, 3, 1).to(dt))


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,H,W", GRID_SHAPES)
def test_hygiene_unpack_grid(gpu, B, C, H, W):
    from scenedino_amd import _lib
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(W))

    def body(ar):
        xv = ar.input("grid", x)
        out = ar.output("out", (B, C, H, W), F32)
        ar.arm()
        _lib._check(_lib.load().sd_unpack_grid(_p(xv), B, C, H, W, _p(out), _stream()), "sd_unpack_grid")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert torch.equal(plain["out"].cpu(), x.permute(0, 3, 1, 2).contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 1028, 2 * 5 * 7 * 36, 70000])
@pytest.mark.parametrize("dt", [F16, BF])
def test_hygiene_cast_grid(gpu, n, dt):
    """sd_cast_grid: bit-equal to the torch cast (round to nearest even)."""
    from scenedino_amd import _lib
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3

    def body(ar):
        xv = ar.input("grid", x)
        out = ar.output("out", (n,), dt)
        ar.arm()
        _lib._check(_lib.load().sd_cast_grid(_p(xv), n, _lib.SD_OF_TORCH[dt], _p(out), _stream()), "sd_cast_grid")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert torch.equal(plain["out"].cpu(), x.to(dt))


def _frame_operands(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.rand(n, 3, H, W, generator=g) * 2 - 1
    w2c = torch.linalg.inv(torch.eye(4).repeat(n, 1, 1) + 0.1 * torch.randn(n, 4, 4, generator=g))
    Ks = torch.eye(3).repeat(n, 1, 1) + 0.2 * torch.rand(n, 3, 3, generator=g)
    return imgs, w2c.contiguous(), Ks


@pytest.mark.gpu
@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (3, 5, 7), (2, 37, 53)])
def test_hygiene_pack_image(gpu, n, H, W):
    """sd_pack_image: bit-equal to the torch permute (rgb in channels 0..2; the pad channel is
    written too, its value is not part of the contract)."""
    from scenedino_amd import _lib
    imgs, _, _ = _frame_operands(n, H, W, 7)

    def body(ar):
        iv = ar.input("img", imgs)
        out = ar.output("out", (n, H, W, 4), F32)
        ar.arm()
        _lib._check(_lib.load().sd_pack_image(_p(iv), n, H, W, _p(out), _stream()), "sd_pack_image")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert torch.equal(plain["out"][..., :3].cpu(), imgs.permute(0, 2, 3, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
def test_hygiene_cam_records(gpu, n):
    """sd_cam_records with view strides s_w = 20 > 16 and s_k = 12 > 9."""
    from scenedino_amd import _lib
    _, w2c, Ks = _frame_operands(n, 2, 2, 8)

    def body(ar):
        wv = ar.input("w2c", w2c.view(n, 16), ld=20)
        kv = ar.input("Ks", Ks.view(n, 9), ld=12)
        out = ar.output("cam", (n, _lib.CAM_WORDS), F32)
        ar.arm()
        _lib._check(_lib.load().sd_cam_records(_p(wv), wv.stride(0), _p(kv), kv.stride(0), n, _p(out),
                                               _stream()), "sd_cam_records")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert torch.equal(plain["cam"], _lib.cam_records(w2c.cuda(), Ks.cuda()))


@pytest.mark.gpu
@pytest.mark.parametrize("n,H,W", [(1, 1, 1), (3, 5, 7)])
def test_hygiene_frame_inputs(gpu, n, H, W):
    from scenedino_amd import _lib
    imgs, w2c, Ks = _frame_operands(n, H, W, 9)

    def body(ar):
        iv, wv, kv = ar.input("img", imgs), ar.input("w2c", w2c), ar.input("Ks", Ks)
        out = ar.output("out", (n, H, W, 4), F32)
        cam = ar.output("cam", (n, _lib.CAM_WORDS), F32)
        ar.arm()
        _lib._check(_lib.load().sd_frame_inputs(_p(iv), n, H, W, _p(out), _p(wv), 16, _p(kv), 9, n, _p(cam),
                                                _stream()), "sd_frame_inputs")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    assert torch.equal(plain["out"][..., :3].cpu(), imgs.permute(0, 2, 3, 1))
    assert torch.equal(plain["cam"], _lib.cam_records(w2c.cuda(), Ks.cuda()))


def _packed_mlp(dtype, C=256):
    from scenedino_amd.mlp_pack import PackedMLP
    g = torch.Generator().manual_seed(C)
    return PackedMLP((torch.randn(128, C + 39, generator=g) * 0.06).cuda(),
                     (torch.randn(128, generator=g) * 0.1).cuda(),
                     (torch.randn(65, 128, generator=g) * 0.1).cuda(),
                     (torch.randn(65, generator=g) * 0.1).cuda(), dtype=dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("B,Hf,Wf", [(3, 5, 7), (1, 1, 1)])
@pytest.mark.parametrize("entry", ["nchw", "nhwc", "nhwc_inputs"])
@pytest.mark.parametrize("exact", [False, True])
def test_hygiene_project_grid(gpu, B, Hf, Wf, entry, exact):
    """sd_project_grid / _nhwc / _nhwc_inputs: the (B, Hf, Wf, 128) f16 projected grid (and the
    frame's packed image and camera records) and nothing around them; the three agree."""
    from scenedino_amd import _lib
    lib = _lib.load()
    C = 256
    m = _packed_mlp(_lib.SD_BF16, C)
    rec = _lib._with_flags(m.rec, exact)
    grid = torch.randn(B, C, Hf, Wf, generator=torch.Generator().manual_seed(Hf))
    imgs, w2c, Ks = _frame_operands(B, 6, 10, 3)

    def body(ar):
        gv = ar.input("grid", grid if entry == "nchw" else grid.permute(0, 2, 3, 1).contiguous())
        out = ar.output("P", (B, Hf, Wf, 128), F16)
        if entry == "nhwc_inputs":
            iv, wv, kv = ar.input("img", imgs), ar.input("w2c", w2c), ar.input("Ks", Ks)
            pim, cam = ar.output("img_out", (B, 6, 10, 4), F32), ar.output("cam", (B, _lib.CAM_WORDS), F32)
            fa = _lib.SdFrameArgs(img_nchw=iv.data_ptr(), N=B, H=6, W=10, out_nhwc4=pim.data_ptr(),
                                  w2c=wv.data_ptr(), s_w=16, Ks=kv.data_ptr(), s_k=9, n=B,
                                  out_cam=cam.data_ptr())
            ar.arm()
            _lib._check(lib.sd_project_grid_nhwc_inputs(_p(gv), B, Hf, Wf, ctypes.byref(rec), _p(out),
                                                        ctypes.byref(fa), _stream()),
                        "sd_project_grid_nhwc_inputs")
        else:
            ar.arm()
            fn = lib.sd_project_grid if entry == "nchw" else lib.sd_project_grid_nhwc
            _lib._check(fn(_p(gv), B, Hf, Wf, ctypes.byref(rec), _p(out), _stream()), "sd_project_grid")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    ref = _lib.project_grid(grid.cuda(), m.rec, m.dtype, exact_grid=exact)
    # (the channels-last kernels write the same bits:
    # test_projected_grid_channels_last_streaming_bit_equal)
    assert torch.equal(plain["P"].view(torch.int16), ref.view(torch.int16))
    if entry == "nhwc_inputs":
        assert torch.equal(plain["img_out"][..., :3].cpu(), imgs.permute(0, 2, 3, 1))
        assert torch.equal(plain["cam"], _lib.cam_records(w2c.cuda(), Ks.cuda()))


# --------------------------------------------------------------------------- training MLP
def _train_mlp(dt, N, seed):
    from scenedino_amd import _lib
    from scenedino_amd.mlp_pack import PackedTrainMLP
    g = torch.Generator().manual_seed(seed)
    W_in, b_in = torch.randn(128, 295, generator=g) * 0.08, torch.randn(128, generator=g) * 0.1
    W_out, b_out = torch.randn(65, 128, generator=g) * 0.1, torch.randn(65, generator=g) * 0.1
    p = PackedTrainMLP(W_in.cuda(), b_in.cuda(), W_out.cuda(), b_out.cuda(), _lib.SD_OF_TORCH[dt], 256)
    x = torch.randn(N, 296, generator=g)
    x[:, 295] = 1.0
    return p, x.to(dt), g


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F16, BF])
def test_hygiene_mlp_train_fwd_bwd(gpu, dt):
    """sd_mlp_train_fwd and sd_mlp_train_bwd at N = 37 (one ragged tile), ldx = 304 > kx = 296:
    h, sigma, dino, then dy, dh and f32 dx rows (lddx = C), written in full."""
    from scenedino_amd import _lib
    N, D, C, ldx = 37, 64, 256, 304
    p, x, g = _train_mlp(dt, N, 12)
    sd = _lib.SD_OF_TORCH[dt]

    def fwd(ar):
        xv = ar.input("x", x, ld=ldx)
        h, sig, dino = ar.output("h", (N, 136), dt), ar.output("sigma", (N,), F32), ar.output("dino", (N, D), F32)
        ar.arm()
        a = _lib.SdMlpTrainArgs(x=xv.data_ptr(), N=N, ldx=xv.stride(0), kx=296, dtype=sd, D=D, C=C,
                                w1f=p.w1f.data_ptr(), w2f=p.w2f.data_ptr(), b_out=p.b_out.data_ptr(),
                                h=h.data_ptr(), sigma=sig.data_ptr(), dino=dino.data_ptr())
        _lib.mlp_train_fwd(a, xv)

    findings, f = run3(gpu, fwd)
    assert_clean(findings)
    assert bool((f["h"][:, 128] == 1).all()) and not f["h"][:, 129:].any()
    gs, gd = torch.randn(N, generator=g), torch.randn(N, D, generator=g)

    def bwd(ar):
        xv = ar.input("x", x, ld=ldx)
        hv, sv = ar.input("h", f["h"].cpu()), ar.input("sigma", f["sigma"].cpu())
        gsv, gdv = ar.input("d_sigma", gs), ar.input("d_dino", gd)
        dy, dh = ar.output("dy", (N, 72), dt), ar.output("dh", (N, 128), dt)
        lddx = C
        dx = ar.output("dx", (N, lddx), F32)
        ar.arm()
        a = _lib.SdMlpTrainArgs(x=xv.data_ptr(), N=N, ldx=xv.stride(0), kx=296, dtype=sd, D=D, C=C,
                                h=hv.data_ptr(), sigma=sv.data_ptr(), d_sigma=gsv.data_ptr(),
                                d_dino=gdv.data_ptr(), wtf=p.wtf.data_ptr(), wxf=p.wxf.data_ptr(),
                                dy=dy.data_ptr(), dh=dh.data_ptr(), dx=dx.data_ptr(), lddx=lddx,
                                dx_dtype=_lib.SD_F32)
        _lib.mlp_train_bwd(a, xv)

    findings, b = run3(gpu, bwd)
    assert_clean(findings)
    assert not b["dy"][:, D + 1:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F16, BF])
def test_hygiene_wgrad(gpu, dt):
    """sd_wgrad at N = 37 with lda = 136 > Ma = 128 and ldb = 304 > Nb = 296."""
    from scenedino_amd import _lib
    N, Ma, Nb, nparts = 37, 128, 296, 2
    g = torch.Generator().manual_seed(13)
    a, b = torch.randn(N, Ma, generator=g).to(dt), torch.randn(N, Nb, generator=g).to(dt)
    MaP, NbP = (Ma + 31) // 32 * 32, (Nb + 31) // 32 * 32

    def body(ar):
        av, bv = ar.input("a", a, ld=136), ar.input("b", b, ld=304)
        part = ar.output("part", (nparts, MaP, NbP), F32)
        ar.arm()
        w = _lib.SdWgradArgs(a=av.data_ptr(), b=bv.data_ptr(), N=N, lda=av.stride(0), ldb=bv.stride(0),
                             Ma=Ma, Nb=Nb, dtype=_lib.SD_OF_TORCH[dt], nparts=nparts, part=part.data_ptr())
        _lib._check(_lib.load().sd_wgrad(ctypes.byref(w), _stream()), "sd_wgrad")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    got = plain["part"].sum(0)[:Ma, :Nb].cpu().double()
    ref = a.double().t() @ b.double()
    assert float((got - ref).norm() / ref.norm()) <= 1e-5  # test_wgrad_kernel_vs_matmul's bound


@pytest.mark.gpu
@pytest.mark.parametrize("N,ldx,kx,nparts", [(37, 296, 296, 2), (1000, 304, 296, 7), (64, 128, 104, 256)])
@pytest.mark.parametrize("dt", [F16, BF])
def test_hygiene_mlp_train_wgrad(gpu, N, ldx, kx, nparts, dt):
    """sd_mlp_train_wgrad: the four gradients written in full and nothing around them, work of
    exactly sd_mlp_train_wgrad_work(nparts) floats (test_mlp_wgrad_fused_vs_matmul has the
    NaN-behind-inputs half and the values)."""
    from scenedino_amd import _lib
    lib = _lib.load()
    D = 64
    g = torch.Generator().manual_seed(N + kx)
    x = torch.randn(N, kx, generator=g).to(dt)
    dh = torch.randn(N, 128, generator=g).to(dt)
    dy = torch.zeros(N, 72, dtype=dt)
    dy[:, :D + 1] = torch.randn(N, D + 1, generator=g).to(dt)
    h = torch.zeros(N, 136, dtype=dt)
    h[:, :128] = torch.randn(N, 128, generator=g).to(dt)
    h[:, 128] = 1
    nwork = int(lib.sd_mlp_train_wgrad_work(nparts))

    def body(ar):
        xv = ar.input("x", x, ld=ldx)
        dv, yv, hv = ar.input("dh", dh), ar.input("dy", dy), ar.input("h", h)
        o = {k: ar.output(k, s, F32) for k, s in (("dw_in", (128, kx - 1)), ("db_in", (128,)),
                                                  ("dw_out", (1 + D, 128)), ("db_out", (1 + D,)))}
        work = ar.work("work", nwork)
        ar.arm()
        a = _lib.SdMlpWgradArgs(x=xv.data_ptr(), dh=dv.data_ptr(), dy=yv.data_ptr(), h=hv.data_ptr(), N=N,
                                ldx=xv.stride(0), kx=kx, D=D, dtype=_lib.SD_OF_TORCH[dt], nparts=nparts,
                                work=work.data_ptr(), dw_in=o["dw_in"].data_ptr(),
                                db_in=o["db_in"].data_ptr(), dw_out=o["dw_out"].data_ptr(),
                                db_out=o["db_out"].data_ptr())
        _lib._check(lib.sd_mlp_train_wgrad(ctypes.byref(a), _stream()), "sd_mlp_train_wgrad")

    findings, plain = run3(gpu, body)
    assert_clean(findings)
    ref = dh.double().t() @ x.double()
    got = plain["dw_in"].cpu().double()
    assert float((got - ref[:, :kx - 1]).norm() / ref[:, :kx - 1].norm()) <= 1e-5
