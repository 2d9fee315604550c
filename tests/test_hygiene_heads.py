"""Memory hygiene of the segmentation / SSCBench / downstream-stage / loss kernels: outputs
and scratch behind guard bands, inputs between poisoned margins (tests/_arena.py); every work
pointer gets exactly what its size function promises."""
import ctypes

import numpy as np
import pytest
import torch

import _crop3d_inputs as c3
import _msc_inputs as mi
import _recon_inputs as ri
import _stego_corr_oracle as co
from _arena import assert_clean, run3
from _ssc_inputs import make_frame
from _stego_oracle import stego_inputs

F32, BF, I32, U8 = torch.float32, torch.bfloat16, torch.int32, torch.uint8


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


def _run_any(gpu, body, **kw):
    findings, plain = run3(gpu, body, **kw)
    assert_clean(findings)
    return plain


def _run(gpu, body, **kw):
    plain = _run_any(gpu, body, **kw)
    for k, v in plain.items():
        if v.is_floating_point():
            assert torch.isfinite(v.float()).all(), k
    return plain


# --------------------------------------------------------------------------- SSCBench
DIMS = (40, 200, 16)
ORIGIN = (0.0, -25.6, -2.0)
VOX = 0.2


def _host_T():
    T = np.eye(4)
    T[:3, 3] = (0.3, -0.1, 1.5)
    T[0, 1], T[1, 0] = -0.05, 0.05
    return T


@pytest.mark.gpu
def test_hygiene_voxel_points(gpu):
    from scenedino_amd import _lib
    nx, ny, nz = DIMS
    o = (ctypes.c_double * 3)(*ORIGIN)
    t = (ctypes.c_double * 12)(*_host_T()[:3].flatten().tolist())

    def body(ar):
        out = ar.output("pts", (nx * ny * nz, 3), F32)
        ar.arm()
        _lib._check(_lib.load().sd_voxel_points(o, VOX, nx, ny, nz, t, _p(out), _stream()), "sd_voxel_points")

    plain = _run(gpu, body)
    assert torch.equal(plain["pts"], _lib.voxel_points(ORIGIN, VOX, DIMS, _host_T(), gpu))


@pytest.mark.gpu
def test_hygiene_voxel_fov(gpu):
    from scenedino_amd import _lib
    nx, ny, nz = DIMS
    o = (ctypes.c_double * 3)(*ORIGIN)
    t = (ctypes.c_double * 12)(*np.linalg.inv(_host_T())[:3].flatten().tolist())
    k = (ctypes.c_double * 9)(552.55, 0.0, 682.05, 0.0, 552.55, 238.77, 0.0, 0.0, 1.0)

    def body(ar):
        out = ar.output("fov", (nx * ny * nz,), U8)
        ar.arm()
        _lib._check(_lib.load().sd_voxel_fov(o, VOX, nx, ny, nz, t, k, 1408, 376, _p(out), _stream()),
                    "sd_voxel_fov")

    plain = _run(gpu, body)
    assert int(plain["fov"].max()) <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [DIMS, (5, 7, 3), (1, 1, 1)])
def test_hygiene_grow3(gpu, dims):
    from scenedino_amd import _lib
    x = torch.rand(*dims, generator=torch.Generator().manual_seed(3))

    def body(ar):
        xv = ar.input("in", x)
        out = ar.output("out", dims, F32)
        ar.arm()
        _lib._check(_lib.load().sd_grow3(_p(xv), dims[0], dims[1], dims[2], _p(out), _stream()), "sd_grow3")

    plain = _run(gpu, body)
    ref = torch.nn.functional.max_pool3d(x[None, None], 3, 1, 1)[0, 0]
    assert torch.equal(plain["out"].cpu(), ref)


@pytest.mark.gpu
def test_hygiene_ssc_confusion(gpu):
    from scenedino_amd import _lib
    from scenedino_amd.sscbench import SSCBenchScores
    nx, ny, nz = DIMS
    sig, seg, gt = (torch.from_numpy(a) for a in make_frame(1, DIMS))
    fov = (torch.rand(DIMS, generator=torch.Generator().manual_seed(2)) > 0.2).to(U8)
    sc = SSCBenchScores(device=gpu)
    nb = len(sc.sizes) * 256 + 1

    def body(ar):
        pv, sv, tv, fv = ar.input("pred", seg), ar.input("sigma", sig), ar.input("target", gt), ar.input("fov", fov)
        conf = ar.output("conf", (nb,), I32)   # zeroed on the stream by the call itself
        ar.arm()
        _lib._check(_lib.load().sd_ssc_confusion(_p(pv), _p(sv), _p(tv), _p(fv), nx, ny, nz,
                                                 ctypes.byref(sc._args), _p(conf), _stream()),
                    "sd_ssc_confusion")

    plain = _run(gpu, body)
    assert torch.equal(plain["conf"], sc.frame_confusion(sig, seg, gt, fov))


# --------------------------------------------------------------------------- seg head
def _heads(d_full, n_cl=5, seed=0):
    from scenedino_amd.downstream_head import KMeansParamHead, StegoClusterHead
    from scenedino_amd.models.backbones.dino import MlpDimReduction
    torch.manual_seed(seed)
    return (MlpDimReduction(d_full, 64, 128).eval(), StegoClusterHead(d_full, 64).eval(),
            KMeansParamHead(n_cl, n_cl, 64).eval())


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, BF])
def test_hygiene_seg_query(gpu, dt):
    """sd_seg_query at P = 65 (one ragged tile) with 5 clusters: labels, seg and dino_full."""
    from scenedino_amd import _lib
    from scenedino_amd.seg_pack import PackedSegHead
    P, d_full = 65, 384
    dr, st, cl = _heads(d_full)
    pk = PackedSegHead(dr, st, cl, device=gpu)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(P, 64, generator=g).to(dt)
    sigma = torch.rand(P, generator=g) - 0.3

    def body(ar):
        xv, sv = ar.input("dino", x), ar.input("sigma", sigma)
        lab, seg = ar.output("labels", (P,), I32), ar.output("seg", (P,), U8)
        full = ar.output("full", (P, d_full), F32)
        ar.arm()
        _lib._check(_lib.load().sd_seg_query(_p(xv), _lib.SD_OF_TORCH[dt], P, ctypes.byref(pk.rec), _p(sv),
                                             0.2, _p(lab), _p(seg), _p(full), _stream()), "sd_seg_query")

    plain = _run(gpu, body)
    assert 0 <= int(plain["labels"].min()) and int(plain["labels"].max()) < 5


@pytest.mark.gpu
@pytest.mark.parametrize("P", [33, 130])
@pytest.mark.parametrize("dt", [F32, BF])
def test_hygiene_expand_bwd(gpu, P, dt):
    from scenedino_amd import _lib
    from scenedino_amd.seg_pack import PackedExpandBwd, PackedSegHead
    d_full = 384
    dr, _, _ = _heads(d_full, seed=1)
    rec, pack = PackedSegHead(dr, device=gpu), PackedExpandBwd(dr, device=gpu)
    g = torch.Generator().manual_seed(P)
    x = torch.randn(P, 64, generator=g).to(dt)
    dy = torch.randn(P, d_full, generator=g)

    def body(ar):
        xv, dv = ar.input("x", x), ar.input("dy", dy)
        dx = ar.output("dx", (P, 64), F32)
        h, de, dh = ar.output("h", (P, 128), BF), ar.output("de", (P, d_full), BF), ar.output("dh", (P, 128), BF)
        xb = ar.output("xb", (P, 64), BF) if dt == F32 else None
        ar.arm()
        a = _lib.SdExpandBwdArgs(x=xv.data_ptr(), dy=dv.data_ptr(), w1=pack.w1.data_ptr(),
                                 w2=pack.w2.data_ptr(), w1t=pack.w1t.data_ptr(), w2t=pack.w2t.data_ptr(),
                                 b1=pack.b1.data_ptr(), b2=pack.b2.data_ptr(), P=P,
                                 x_dtype=_lib.SD_OF_TORCH[dt], dx=dx.data_ptr(), h=h.data_ptr(),
                                 de=de.data_ptr(), dh=dh.data_ptr(), xb=_p(xb))
        _lib._check(_lib.load().sd_expand_bwd(ctypes.byref(a), ctypes.byref(rec.rec), _stream()),
                    "sd_expand_bwd")

    plain = _run(gpu, body)
    if dt == F32:
        assert torch.equal(plain["xb"].cpu(), x.to(BF))


@pytest.mark.gpu
@pytest.mark.parametrize("M", [33, 130])
@pytest.mark.parametrize("d_in", [384, 768])
def test_hygiene_stego_train(gpu, M, d_in):
    """sd_stego_train_fwd (y and the saved xh, mid, e) and sd_stego_train_bwd (dlin, dnon, dmid)
    with dropout scales, M = 33 and 130 (ragged 32-row tiles)."""
    from scenedino_amd import _lib
    from scenedino_amd.downstream_head import StegoClusterHead
    from scenedino_amd.seg_pack import PackedStegoTrain
    d = stego_inputs(M, d_in)
    st = StegoClusterHead(d_in, 64)
    st.load_state_dict({k: v for k, v in d.items() if k.endswith((".weight", ".bias"))})
    pack = PackedStegoTrain(st, device=gpu)
    rpg = d["rows_per_group"]
    lib = _lib.load()

    def fwd(ar):
        xv, ml, mn = ar.input("x", d["x"]), ar.input("m_lin", d["m_lin"]), ar.input("m_non", d["m_non"])
        y, e = ar.output("y", (M, 64), F32), ar.output("e", (M, 64), F32)
        xh, mid = ar.output("xh", (M, d_in), BF), ar.output("mid", (M, d_in), BF)
        ar.arm()
        a = _lib._stego_args(pack, M, ml, mn, rpg)
        a.x, a.y, a.normalize = xv.data_ptr(), y.data_ptr(), 1
        a.xh, a.mid, a.e = xh.data_ptr(), mid.data_ptr(), e.data_ptr()
        _lib._check(lib.sd_stego_train_fwd(ctypes.byref(a), _stream()), "sd_stego_train_fwd")

    f = _run(gpu, fwd)

    def bwd(ar):
        ml, mn = ar.input("m_lin", d["m_lin"]), ar.input("m_non", d["m_non"])
        ev, mv, dv = ar.input("e", f["e"].cpu()), ar.input("mid", f["mid"].cpu()), ar.input("dy", d["dy"])
        dlin, dnon = ar.output("dlin", (M, 64), BF), ar.output("dnon", (M, 64), BF)
        dmid = ar.output("dmid", (M, d_in), BF)
        ar.arm()
        a = _lib._stego_args(pack, M, ml, mn, rpg)
        a.e, a.mid, a.dy = ev.data_ptr(), mv.data_ptr(), dv.data_ptr()
        a.dlin, a.dnon, a.dmid = dlin.data_ptr(), dnon.data_ptr(), dmid.data_ptr()
        _lib._check(lib.sd_stego_train_bwd(ctypes.byref(a), _stream()), "sd_stego_train_bwd")

    _run(gpu, bwd)


@pytest.mark.gpu
@pytest.mark.parametrize("N,d,K", [(1, 64, 19), (65, 384, 32), (1000, 768, 19)])
@pytest.mark.parametrize("dt", [F32, BF])
def test_hygiene_cluster_probe(gpu, N, d, K, dt):
    """sd_cluster_probe: labels, S, counts in full; work of exactly sd_cluster_probe_work floats."""
    from scenedino_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(N + d)
    x = torch.randn(N, d, generator=g).to(dt)
    cen = torch.nn.functional.normalize(torch.randn(K, d, generator=g), dim=-1)
    w = torch.rand(N, generator=g)
    G = (N + 47) // 48
    m = (torch.rand(G, d, generator=g) > 0.1).float() / 0.9
    nwork = int(lib.sd_cluster_probe_work(N, d, K))
    assert nwork > 0

    def body(ar):
        xv, cv, wv, mv = ar.input("x", x), ar.input("centres", cen), ar.input("w", w), ar.input("m", m)
        lab, S, cnt = ar.output("labels", (N,), I32), ar.output("S", (K, d), F32), ar.output("counts", (K,), I32)
        work = ar.work("work", nwork)
        ar.arm()
        a = _lib.SdClusterProbeArgs(x=xv.data_ptr(), m=mv.data_ptr(), centres=cv.data_ptr(), w=wv.data_ptr(),
                                    N=N, rows_per_group=48, n_groups=G, d=d, K=K,
                                    x_dtype=_lib.SD_OF_TORCH[dt], work=work.data_ptr(),
                                    labels=lab.data_ptr(), S=S.data_ptr(), counts=cnt.data_ptr())
        _lib._check(lib.sd_cluster_probe(ctypes.byref(a), _stream()), "sd_cluster_probe")

    plain = _run(gpu, body)
    assert int(plain["counts"].sum()) == N
    assert torch.equal(torch.bincount(plain["labels"].long(), minlength=K).to(I32), plain["counts"])


# --------------------------------------------------------------------------- stego corr
@pytest.mark.gpu
@pytest.mark.parametrize("pointwise", [False, True])
@pytest.mark.parametrize("bf16", [False, True])
def test_hygiene_stego_corr(gpu, pointwise, bf16):
    """sd_stego_corr_fwd / _bwd on the smallest of test_stego_corr_gpu's SHAPES (1, 24, 24, 384),
    three pairs with the self pair: work of exactly sd_stego_corr_work bytes."""
    from scenedino_amd import _lib
    lib = _lib.load()
    nc, P, Q, dd = 1, 24, 24, 384
    rows = co.make_rows(nc, P, Q, dd, 3, True)
    dt = BF if bf16 else F32
    A, a_ = rows["A"].to(dt), rows["a"]
    Bs = [None if t is None else t.to(dt) for t in rows["Bs"]]
    w, s = co.YAML_WEIGHTS, co.YAML_SHIFTS
    nbytes = int(lib.sd_stego_corr_work(nc, P, Q, dd, 3, 1))
    assert nbytes > 0
    up = torch.tensor([0.7, -1.3, 0.4])
    keep = {}

    def operands(ar):
        Av, av = ar.input("A", A), ar.input("a", a_)
        part = [(None, None) if B is None else (ar.input(f"B{i}", B), ar.input(f"b{i}", b))
                for i, (B, b) in enumerate(zip(Bs, rows["bs"]))]
        return _lib._stego_corr_args(Av, av, part, w, s, pointwise)

    def fwd(ar):
        g = operands(ar)
        work = ar.work("work", nbytes, U8)
        loss = ar.output("loss", (3,), F32)
        ar.arm()
        g.work, g.work_bytes, g.loss = work.data_ptr(), nbytes, loss.data_ptr()
        _lib._check(lib.sd_stego_corr_fwd(ctypes.byref(g), _stream()), "sd_stego_corr_fwd")
        if ar.poison is None:
            keep["work"] = work

    _run(gpu, fwd)
    state = keep["work"].cpu()

    def bwd(ar):
        g = operands(ar)
        # the forward's state: read here (scratch inside it may be reused: in place)
        work = ar.input("work", state, inplace=True)
        uv = ar.input("up", up)
        d_a = ar.output("d_a", (nc, P, 64), F32)
        d_b = [None, ar.output("d_b1", (nc, Q, 64), F32), ar.output("d_b2", (nc, Q, 64), F32)]
        ar.arm()
        g.work, g.work_bytes, g.up, g.d_a = work.data_ptr(), nbytes, uv.data_ptr(), d_a.data_ptr()
        for i in (1, 2):
            g.d_b[i] = d_b[i].data_ptr()
        _lib._check(lib.sd_stego_corr_bwd(ctypes.byref(g), _stream()), "sd_stego_corr_bwd")

    _run(gpu, bwd)


# --------------------------------------------------------------------------- recon loss
@pytest.mark.gpu
@pytest.mark.parametrize("dino_bf16", [False, True])
def test_hygiene_recon_loss(gpu, dino_bf16):
    """sd_recon_loss_fwd / _bwd on _recon_inputs' "odd" shape (5 x 7 patches, two views): every
    state buffer and gradient in full, work of exactly sd_recon_loss_work floats."""
    from scenedino_amd import _lib
    lib = _lib.load()
    n, pc, h, w, nv, K = ri.SHAPES["odd"]
    C = 64
    data = ri.make_data(ri.SHAPES["odd"], seed=ri.SEEDS["odd"], C=C, artifacts=True)
    part = data["coarse"][0]
    P = n * pc
    ddt = BF if dino_bf16 else F32
    ins = {"rgb": part["rgb"].reshape(P, h, w, nv, 3), "rgb_gt": data["rgb_gt"].reshape(P, h, w, 3),
           "invalid": part["invalid"].reshape(P, h, w, K, nv), "weights": part["weights"].reshape(P, h, w, K),
           "depth": part["depth"].reshape(P, h, w),
           "dino": part["dino_features"].reshape(P, h, w, C).to(ddt),
           "down": part["dino_features_downsampled"].reshape(-1, C),
           "dino_gt": data["dino_gt"].reshape(-1, C), "art": data["dino_artifacts"].reshape(-1, C)}
    ins = {k: v.contiguous() for k, v in ins.items()}
    R = ins["down"].shape[0]
    cfg = dict(policy=_lib.SD_RL_POLICY_WEIGHT, lambda_coarse=1.0, lambda_dino=0.5, temperature=1.0,
               lambda_depth=0.01, lambda_dsmooth=0.25)
    nwork = int(lib.sd_recon_loss_work(P, C, R))
    assert nwork > 0
    npx = P * h * w

    def args(ar, v):
        return _lib._recon_args(v["rgb"], v["rgb_gt"], v["invalid"], v["weights"], v["depth"], v["dino"],
                                v["down"], v["dino_gt"], v["art"], cfg)

    def fwd(ar):
        v = {k: ar.input(k, t) for k, t in ins.items()}
        g = args(ar, v)
        o = {"rec": ar.output("rec", (1,), F32), "terms": ar.output("terms", (4,), F32),
             "sel": ar.output("sel", (npx,), I32), "edge": ar.output("edge", (npx, 2), F32),
             "dmean": ar.output("dmean", (P,), F32), "count": ar.output("count", (1,), F32)}
        work = ar.work("work", nwork)
        ar.arm()
        for k, t in o.items():
            setattr(g, k, t.data_ptr())
        g.work = work.data_ptr()
        _lib._check(lib.sd_recon_loss_fwd(ctypes.byref(g), _stream()), "sd_recon_loss_fwd")

    f = _run(gpu, fwd)
    g_rec = torch.tensor([1.7])

    def bwd(ar):
        v = {k: ar.input(k, t) for k, t in ins.items()}
        g = args(ar, v)
        for k in ("sel", "edge", "dmean", "count"):
            setattr(g, k, ar.input("s_" + k, f[k].cpu()).data_ptr())
        g.g_rec = ar.input("g_rec", g_rec).data_ptr()
        g.work = ar.work("work", nwork).data_ptr()
        o = {"d_rgb": ar.output("d_rgb", (P, h, w, nv, 3), F32), "d_depth": ar.output("d_depth", (P, h, w), F32),
             "d_dino": ar.output("d_dino", (P, h, w, C), ddt), "d_down": ar.output("d_down", (R, C), F32)}
        ar.arm()
        for k, t in o.items():
            setattr(g, k, t.data_ptr())
        _lib._check(lib.sd_recon_loss_bwd(ctypes.byref(g), _stream()), "sd_recon_loss_bwd")

    _run(gpu, bwd)


# --------------------------------------------------------------------------- msc gt
@pytest.mark.gpu
@pytest.mark.parametrize("C", [8, 1024])
@pytest.mark.parametrize("normalize", [False, True])
def test_hygiene_msc_gt(gpu, C, normalize):
    """sd_msc_gt on _msc_inputs' golden geometry (B 2, V 4, 3 x 5 token grids, 24 x 40 pixels);
    the augmented views' homographies are their crop boxes."""
    from scenedino_amd import _lib
    c = mi.GOLDEN
    B, V, hp, wp, H, W = c["B"], c["V"], c["hp"], c["wp"], c["H"], c["W"]
    feat = torch.randn(B, V, C, hp, wp, generator=torch.Generator().manual_seed(C))
    T = torch.zeros(B, V - 2, 3, 3)
    for b in range(B):
        for k, (x0, y0, x1, y1) in enumerate(mi.GOLDEN_BOXES[b]):
            sx, sy = W / (x1 - x0), H / (y1 - y0)
            T[b, k] = torch.tensor([[sx, 0, -x0 * sx], [0, sy, -y0 * sy], [0, 0, 1.0]])

    def body(ar):
        fv, tv = ar.input("feat", feat), ar.input("T", T)
        out = ar.output("out", (B, C, H, W), F32)
        ar.arm()
        a = _lib.SdMscGtArgs(feat=fv.data_ptr(), T=tv.data_ptr(), out=out.data_ptr(), B=B, V=V, C=C,
                             hp=hp, wp=wp, H=H, W=W, normalize=int(normalize))
        _lib._check(_lib.load().sd_msc_gt(ctypes.byref(a), _stream()), "sd_msc_gt")

    _run(gpu, body)


# --------------------------------------------------------------------------- 3-D crops
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["batch2", "plateau"])
def test_hygiene_crop3d_centres(gpu, name):
    """sd_crop3d_centres: view 0 of two-view operands (the frame strides skip view 1, which is
    other data), every output in full."""
    from scenedino_amd import _lib
    d = c3.make_case(name, 5)
    n, _, h, w = d["depth"].shape
    nc, S = c3.N_CROPS, c3.S
    shift = c3.shift_of(d["unit"], d["rad"]).contiguous()

    def body(ar):
        dv, pv, kv = ar.input("depth", d["depth"]), ar.input("poses", d["poses"]), ar.input("projs", d["projs"])
        uv, sv = ar.input("pick", d["pick"]), ar.input("shift", shift)
        o = {"limits": ar.output("limits", (n, nc + 1), F32), "count": ar.output("count", (n, nc), I32),
             "pixel": ar.output("pixel", (n, nc, 2), I32), "centre": ar.output("centre", (n, nc, 3), F32),
             "points": ar.output("points", (n, nc, S, 3), F32)}
        ar.arm()
        a = _lib.SdCrop3dArgs(depth=dv.data_ptr(), poses=pv.data_ptr(), projs=kv.data_ptr(),
                              u_pick=uv.data_ptr(), shift=sv.data_ptr(),
                              depth_stride=2 * h * w, pose_stride=32, proj_stride=18, n=n, h=h, w=w,
                              n_crops=nc, S=S, z_far=c3.Z_FAR,
                              **{k: t.data_ptr() for k, t in o.items()})
        _lib._check(_lib.load().sd_crop3d_centres(ctypes.byref(a), _stream()), "sd_crop3d_centres")

    plain = _run(gpu, body)
    assert int(plain["count"].sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, BF])
def test_hygiene_crop3d_compact(gpu, dt):
    """sd_crop3d_compact at (C, S, D) = (7, 64, 16), n_samples 16: kept, dropped (crop_ok 0)
    and too-sparse crops; the crops past n_valid are zero."""
    from scenedino_amd import _lib
    C, S, D, ns = 7, 64, 16, 16
    g = torch.Generator().manual_seed(8)
    sigma = torch.rand(C, S, generator=g)
    sigma[2] *= 0.3          # too few samples above thr
    codes = torch.randn(C, S, D, generator=g).to(dt)
    ok = torch.tensor([3, 1, 5, 0, 2, 9, 1], dtype=I32)

    def body(ar):
        sv, cv, kv = ar.input("sigma", sigma), ar.input("codes", codes), ar.input("crop_ok", ok)
        co_, oc = ar.output("codes_out", (C, ns, D), dt), ar.output("occ_out", (C, ns), F32)
        nvld, slot = ar.output("n_valid", (1,), I32), ar.output("slot", (C,), I32)
        ar.arm()
        a = _lib.SdCrop3dCompactArgs(sigma=sv.data_ptr(), codes=cv.data_ptr(), crop_ok=kv.data_ptr(),
                                     codes_out=co_.data_ptr(), occ_out=oc.data_ptr(),
                                     n_valid=nvld.data_ptr(), slot=slot.data_ptr(), C=C, S=S, D=D,
                                     n_samples=ns, codes_dtype=_lib.SD_OF_TORCH[dt], thr=0.5)
        _lib._check(_lib.load().sd_crop3d_compact(ctypes.byref(a), _stream()), "sd_crop3d_compact")

    plain = _run(gpu, body)
    keep = [c for c in range(C) if ok[c] > 0 and int((sigma[c] > 0.5).sum()) > ns]
    assert int(plain["n_valid"]) == len(keep) and 0 < len(keep) < C
    assert not plain["codes_out"][len(keep):].any() and not plain["occ_out"][len(keep):].any()
    for i, c in enumerate(keep):
        assert torch.equal(plain["codes_out"][i].cpu(), codes[c][sigma[c] > 0.5][:ns])


# --------------------------------------------------------------------------- salience
@pytest.mark.gpu
@pytest.mark.parametrize("N,S,C", [(3, 25, 68), (2, 64, 384)])
@pytest.mark.parametrize("normalize", [False, True])
def test_hygiene_salience(gpu, N, S, C, normalize):
    """sd_salience_fwd (out, sal, wmap, ynorm) and sd_salience_bwd (gx and the per-patch
    partial parameter gradients)."""
    from scenedino_amd import _lib
    g = torch.Generator().manual_seed(S + C)
    x = torch.randn(N, S, C, generator=g)
    w, b = torch.randn(C, generator=g) / C ** 0.5, torch.randn(1, generator=g)
    pw, pb = 1 + 0.1 * torch.randn(S, generator=g), 0.1 * torch.randn(S, generator=g)
    base = {"x": x, "w": w, "b": b, "pw": pw, "pb": pb}

    def fwd(ar):
        v = {k: ar.input(k, t) for k, t in base.items()}
        o = {"out": ar.output("out", (N, C), F32), "sal": ar.output("sal", (N, S), F32),
             "wmap": ar.output("wmap", (N, S), F32),
             # (written only when normalising, as the header says)
             "ynorm": ar.output("ynorm", (N,), F32, full=bool(normalize))}
        ar.arm()
        a = _lib.SdSalienceArgs(N=N, S=S, C=C, normalize=int(normalize),
                                **{k: t.data_ptr() for k, t in {**v, **o}.items()})
        _lib.salience_fwd(a, v["x"])

    f = _run_any(gpu, fwd)
    assert torch.isfinite(f["out"]).all() and torch.isfinite(f["ynorm"]).all() == bool(normalize)
    gr = {"g_out": torch.randn(N, C, generator=g), "g_sal": torch.randn(N, S, generator=g),
          "g_wmap": torch.randn(N, S, generator=g)}

    def bwd(ar):
        v = {k: ar.input(k, t) for k, t in base.items() if k != "b"}
        v.update({k: ar.input(k, f[k].cpu()) for k in ("out", "sal", "wmap", "ynorm")})
        v.update({k: ar.input(k, t) for k, t in gr.items()})
        o = {"gx": ar.output("gx", (N, S, C), F32), "gw_part": ar.output("gw_part", (N, C), F32),
             "gpw_part": ar.output("gpw_part", (N, S), F32), "gpb_part": ar.output("gpb_part", (N, S), F32),
             "gb_part": ar.output("gb_part", (N,), F32)}
        ar.arm()
        a = _lib.SdSalienceArgs(N=N, S=S, C=C, normalize=int(normalize),
                                **{k: t.data_ptr() for k, t in {**v, **o}.items()})
        _lib.salience_bwd(a, v["x"])

    _run(gpu, bwd)
