"""GPU: the 3-D crop kernels (csrc/sdhip_crop3d.hip) against the torch route of
scenedino_amd/training/crop3d.py on the device, and the whole sampler on a small BTSNet.

sd_crop3d_centres: the limits against torch.quantile (1 ulp, inside their bracketing order
statistics, exact ends); counts and picks against the torch route handed the kernel's own limits
(self-consistent: a 1-ulp lerp difference cannot hide a wrong scan); centres and points bit-equal
to sd_gen_rays' ray at the picked pixel followed by torch's separate multiply and add.
sd_crop3d_compact: codes, n_valid and slot exact; occupancy within 4 * 2^-23 of the f64 value
(an exp good to 2 ulp of a value <= 0.61, plus one rounding of a value < 1)."""
from __future__ import annotations

import pytest
import torch

import _crop3d_inputs as ci

Z_FAR = 100.0
LAST_U = 1.0 - 2.0 ** -24


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _big_case():
    """192 x 640, n = 2: 30 % of each map on a plateau at the maximum of the selection and a band
    of rows at or beyond z_far."""
    g = torch.Generator().manual_seed(7)
    n, h, w = 2, 192, 640
    c = ci.make_case("batch2", 5)
    depth = (3.0 + 77.0 * torch.rand(n, 2, h, w, generator=g)).clamp_max(79.99)
    for f in range(n):
        idx = torch.randperm(h * w, generator=g)[:int(0.3 * h * w)]
        depth[f, 0].view(-1)[idx] = 80.0
        depth[f, 0, 5 + f:15] = 150.0
        depth[f, 0, 15, ::2] = Z_FAR
    c["depth"] = depth
    return c


MAPS = {"small": lambda: ci.make_case("full", 0),        # fewer pixels than a workgroup has lanes
        "ragged": lambda: ci.make_case("plateau", 3),    # 37 x 83, the last bin empty
        "big": _big_case}
PLATEAU = {"small": False, "ragged": True, "big": True}


@pytest.fixture(scope="module")
def maps(gpu):
    out = {}
    for name, make in MAPS.items():
        c = {k: v.to(gpu) for k, v in make().items()}
        c["shift"] = ci.shift_of(c["unit"], c["rad"])
        out[name] = c
    return out


def _ulps(a, b):
    return (a.view(torch.int32).long() - b.view(torch.int32).long()).abs()


@pytest.mark.gpu
@pytest.mark.parametrize("pick", ["random", "first", "last"])
@pytest.mark.parametrize("name", list(MAPS))
def test_centres_kernel(gpu, maps, name, pick):
    from scenedino_amd import _lib
    from scenedino_amd.training import crop3d
    c = maps[name]
    n, _, h, w = c["depth"].shape
    u = {"random": c["pick"], "first": torch.zeros_like(c["pick"]),
         "last": torch.full_like(c["pick"], LAST_U)}[pick]
    limits, count, pixel, centre, points = _lib.crop3d_centres(
        c["depth"], c["poses"], c["projs"], Z_FAR, u, c["shift"])
    torch.cuda.synchronize()
    nc = ci.N_CROPS
    q = (torch.arange(nc + 1, dtype=torch.float64) / nc).float().to(gpu)
    for f in range(n):
        d = c["depth"][f, 0]
        sel = d[d < Z_FAR].sort().values
        want = torch.quantile(sel, q)
        m = sel.numel()
        rank = q * float(m - 1)
        lo, hi = sel[rank.floor().long()], sel[rank.ceil().long()]
        print(name, pick, f, "limit ulps", _ulps(limits[f], want).tolist())
        assert int(_ulps(limits[f], want).max()) <= 1
        assert bool(((limits[f] >= lo) & (limits[f] <= hi)).all())
        assert limits[f, 0] == sel[0] and limits[f, nc] == sel[-1]
    # counts and picks against the torch route on the kernel's own limits
    _, count_t, pixel_t, _, _ = crop3d.centres_torch(c["depth"], c["poses"], c["projs"], Z_FAR, u,
                                                     c["shift"], limits=limits)
    assert torch.equal(count, count_t)
    assert torch.equal(pixel, pixel_t)
    if PLATEAU[name]:
        assert not count[:, -1].any() and bool((pixel[:, -1] == -1).all())
    assert bool((count[:, :-1] > 0).all())
    if pick != "random":  # the first / last pixel of each bin in torch.nonzero order
        for f in range(n):
            d = c["depth"][f, 0]
            for i in range(nc):
                pos = torch.nonzero((d > limits[f, i]) & (d < limits[f, i + 1]))
                assert pos.shape[0] == int(count[f, i])
                if pos.shape[0]:
                    assert torch.equal(pixel[f, i].long(), pos[0 if pick == "first" else -1])
    # centres and points: sd_gen_rays' ray at the pixel, then torch's multiply and add
    rays = _lib.gen_rays(c["poses"][:, 0].contiguous(), c["projs"][:, 0].contiguous(),
                         torch.zeros(n, device=gpu), h, w, 0.0, 0.0)
    ok = count > 0
    row, col = pixel[..., 0].long().clamp_min(0), pixel[..., 1].long().clamp_min(0)
    fi = torch.arange(n, device=gpu)[:, None].expand(-1, nc)
    r = rays[fi, row, col]
    want_c = r[..., :3] + r[..., 3:6] * c["depth"][:, 0][fi, row, col][..., None]
    want_c = torch.where(ok[..., None], want_c, torch.zeros_like(want_c))
    assert torch.equal(centre, want_c)
    want_p = torch.where(ok[..., None, None], want_c[:, :, None] + c["shift"],
                         torch.zeros_like(c["shift"]))
    assert torch.equal(points, want_p)


@pytest.mark.gpu
def test_centres_frame_without_selection(gpu, maps):
    from scenedino_amd import _lib
    c = maps["ragged"]
    depth = c["depth"].repeat(2, 1, 1, 1)
    depth[0] = 150.0
    rep = lambda t: t.repeat(2, *([1] * (t.dim() - 1))).contiguous()  # noqa: E731
    limits, count, pixel, centre, points = _lib.crop3d_centres(
        depth, rep(c["poses"]), rep(c["projs"]), Z_FAR, rep(c["pick"]), rep(c["shift"]))
    one = _lib.crop3d_centres(c["depth"], c["poses"], c["projs"], Z_FAR, c["pick"], c["shift"])
    assert bool(torch.isnan(limits[0]).all()) and not count[0].any()
    assert bool((pixel[0] == -1).all()) and not centre[0].any() and not points[0].any()
    for got, want in zip((limits, count, pixel, centre, points), one):
        assert torch.equal(got[1:], want)


def _compact_case(C, S, ns, dtype, variant, dev):
    g = torch.Generator().manual_seed(C * 1000 + S)
    thr = 0.5
    sigma = torch.rand(C, S, generator=g)
    sigma[sigma == thr] = 0.25
    crop_ok = torch.ones(C, dtype=torch.int32)

    def exactly(c, k, fill=0.25):
        """crop c: k samples above thr at random places, the rest at ``fill``."""
        idx = torch.randperm(S, generator=g)
        sigma[c, idx[:k]] = 0.5 + 0.5 * torch.rand(k, generator=g).clamp_min(1e-3)
        sigma[c, idx[k:]] = fill

    patterns = [lambda c: exactly(c, ns + 1), lambda c: exactly(c, ns),
                lambda c: crop_ok.__setitem__(c, 0), lambda c: exactly(c, ns, fill=thr)]
    for c, p in enumerate(patterns[:C]):
        p(c)
    if C > 2:
        sigma[2] = 0.9  # plenty of occupancy, but crop_ok = 0
    if variant == "all_invalid":
        crop_ok[:] = 0
    codes = torch.randn(C, S, 64, generator=g).to(dtype)
    return sigma.to(dev), codes.to(dev), crop_ok.to(dev), thr


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["mixed", "all_invalid"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C, S, ns", [(1, 64, 16), (7, 64, 16), (20, 2304, 576)])
def test_compact_kernel(gpu, C, S, ns, dtype, variant):
    from scenedino_amd import _lib
    from scenedino_amd.training import crop3d
    sigma, codes, crop_ok, thr = _compact_case(C, S, ns, dtype, variant, gpu)
    out, occ, n_valid, slot = _lib.crop3d_compact(sigma, codes, crop_ok, thr, ns)
    out_t, _, n_valid_t, slot_t = crop3d.compact_torch(sigma, codes, crop_ok, thr, ns)
    k = int(n_valid)
    assert k == int(n_valid_t) and torch.equal(slot, slot_t)
    n_occ = (sigma > thr).sum(1)
    want_kept = (crop_ok > 0) & (n_occ > ns)
    assert torch.equal(slot >= 0, want_kept)
    if variant == "all_invalid":
        assert k == 0
    else:
        assert slot[0] == 0 and k == int(want_kept.sum())
        if C > 1:
            assert n_occ[1] == ns and slot[1] == -1          # exactly n_samples: dropped
        if C > 3:
            assert slot[2] == -1 and n_occ[2] == S           # crop_ok = 0
            assert n_occ[3] == ns and slot[3] == -1          # sigma == thr is not occupied
            assert k == C - 3
    assert out.dtype == dtype and torch.equal(out.view(torch.uint8), out_t.view(torch.uint8))
    assert not out[k:].any() and not occ[k:].any()
    # occupancy against f64 on the rows the torch route picks
    cum = (sigma > thr).cumsum(1, dtype=torch.int32)
    want = torch.arange(1, ns + 1, device=gpu, dtype=torch.int32).expand(C, -1).contiguous()
    rows = sigma.gather(1, torch.searchsorted(cum, want).clamp_max(S - 1)).double()
    occ64 = 1 - torch.exp(-rows)
    kept = torch.nonzero(slot >= 0).flatten()
    err = (occ[:k].double() - occ64[kept]).abs().max() if k else torch.zeros(())
    print(C, S, ns, dtype, variant, "occupancy err", float(err))
    assert float(err) <= 4 * 2.0 ** -23


# ------------------------------------------------------------------ the whole sampler
@pytest.fixture(scope="module")
def scene(gpu):
    """A small real BTSNet (the field_query fixture's weights, two frames) with an
    MlpDimReduction, and depth maps whose crops land inside the frustum."""
    from _helpers import build_net, load
    from test_seg import modules_from, seg_params
    fq = load("field_query.npz")
    grid = torch.as_tensor(fq["grid"]).repeat(2, 1, 1, 1)
    net = build_net(grid, fq["W_in"], fq["b_in"], fq["W_out"], fq["b_out"], "fp32", gpu)
    net.encoder.dim_reduction = modules_from(seg_params(load("seg_head.npz"), "_768"))[0].to(gpu)
    net.encoder.expand_dim = net.encoder.dim_reduction.transform_expand
    T = lambda k: torch.as_tensor(fq[k]).repeat(2, *([1] * (fq[k].ndim - 1))).to(gpu)  # noqa: E731
    poses, projs = T("poses"), T("Ks")
    net.encode(T("images"), projs, poses, ids_encoder=[0], ids_render=[0])
    g = torch.Generator().manual_seed(3)
    depth = (4.0 + 30.0 * torch.rand(2, 1, 24, 80, generator=g)).to(gpu)
    S = 4 * 16
    draws = {"pick": torch.rand(2, 5, generator=g).to(gpu),
             "shift": ci.shift_of(torch.randn(2, 5, S, 3, generator=g),
                                  torch.rand(2, 5, S, 1, generator=g)).to(gpu)}
    return net, poses, projs, depth, draws


def _sample(scene, native, monkeypatch, draws=True, **kw):
    from scenedino_amd.training import crop3d
    net, poses, projs, depth, d = scene
    monkeypatch.setattr(crop3d, "_NATIVE", native)
    return crop3d._sample_3d_crop_padded(net, poses, projs, depth, z_far=Z_FAR, n_crops=5,
                                         n_samples=16, sigma_threshold=kw.pop("thr", 0.5),
                                         draws=d if draws else None, **kw)


@pytest.mark.gpu
def test_query_without_the_colour_gather_is_bit_equal(gpu, scene):
    net = scene[0]
    g = torch.Generator().manual_seed(1)
    xyz = torch.rand(2, 640, 3, generator=g)
    xyz = (xyz * torch.tensor([16.0, 4.0, 30.0]) + torch.tensor([-8.0, -2.0, 3.0])).to(gpu)
    with torch.no_grad():
        a = net.query(xyz, colors=True)
        b = net.query(xyz, colors=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert float((a[0] > 0.5).float().mean()) > 0.05  # not an empty comparison


@pytest.mark.gpu
def test_native_route_equals_torch_route(gpu, scene, monkeypatch):
    """Same draws: bit-equal points into the same net.query and expand_dim kernels, so the same
    kept crops and bit-equal outputs (a row's result does not depend on its place in the
    batch)."""
    from scenedino_amd.training import sample_3d_crop
    dino_n, occ_n, nv_n, aux_n = _sample(scene, True, monkeypatch)
    dino_t, occ_t, nv_t, aux_t = _sample(scene, False, monkeypatch)
    for k in ("count", "pixel", "centre", "points", "sigma", "codes", "slot", "codes_out"):
        assert torch.equal(aux_n[k], aux_t[k]), k
    assert _ulps(aux_n["limits"], aux_t["limits"]).max() <= 1
    k = int(nv_n)
    print("kept crops", k, "of", aux_n["slot"].numel(),
          "dino diff", float((dino_n[:k] - dino_t[:k]).abs().max()),
          "occ diff", float((occ_n[:k] - occ_t[:k]).abs().max()))
    assert k == int(nv_t) and 0 < k < aux_n["slot"].numel()
    assert torch.equal(dino_n[:k], dino_t[:k])
    assert torch.equal(occ_n[:k], occ_t[:k])
    assert dino_n.shape == (10, 16, 768)
    # the public function: the reference's return contract
    monkeypatch.undo()
    net, poses, projs, depth, draws = scene
    dino, occ = sample_3d_crop(net, poses, projs, depth, z_far=Z_FAR, n_crops=5, n_samples=16,
                               draws=draws)
    assert dino.shape == (1, k, 16, 768) and occ.shape == (1, k, 16, 1)
    assert torch.equal(dino[0], dino_n[:k]) and torch.equal(occ[0, ..., 0], occ_n[:k])
    assert sample_3d_crop(net, poses, projs, depth, z_far=Z_FAR, n_crops=5, n_samples=16,
                          sigma_threshold=1e6, draws=draws) == (None, None)


@pytest.mark.gpu
def test_padded_sampler_has_no_host_sync(gpu, scene, monkeypatch):
    _sample(scene, True, monkeypatch, draws=False)  # packs the weights once
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    honoured = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        dino, occ, n_valid, _ = _sample(scene, True, monkeypatch, draws=False)
        try:
            n_valid.item()
        except RuntimeError:
            honoured = True
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    if not honoured:
        pytest.skip("this torch build does not raise on a synchronising call in sync debug mode")
    assert 0 <= int(n_valid) <= 10
