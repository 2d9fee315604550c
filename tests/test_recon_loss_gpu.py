"""GPU: ReconstructionLoss's native route (sd_recon_loss_fwd / _bwd, csrc/sdhip_recon_loss.hip)
against the same class's torch route in float64 on the CPU, on tests/_recon_inputs.py's inputs.

Tolerance: every metric and every gradient tensor within 1e-5 rel-L2 of the float64 oracle, the
bar of the other fp32 training kernels against the same kind of oracle.
The float32 CPU torch route's own error is printed beside each number.  No element is masked
out: tests/test_recon_loss.py asserts that the inputs' argmin and threshold margins are >= 1e-5,
so no branch can flip in float32.

Measured on MI355X: see DESIGN §4 (reconstruction loss)."""
from __future__ import annotations

import functools

import pytest
import torch

import _recon_inputs as ri
from _helpers import rel_l2

BF = torch.bfloat16
BOUND = 1e-5
# (shape key, C, dino dtype): the three shapes, two channel chunks, bf16 features
NATIVE_CASES = [("p16", 64, None), ("p8", 64, None), ("odd", 64, None), ("p8", 128, None),
                ("odd", 64, BF), ("p16", 128, BF)]


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _loss(cfg, native=True):
    from scenedino_amd.losses import make_loss
    loss = make_loss(cfg)
    loss.native = native
    return loss


def _raw(key, C=64, **kw):
    return ri.make_data(ri.SHAPES[key], seed=ri.SEEDS[key], C=C, **kw)


def _grads(data):
    return {n: t.grad for n, t in ri.leaves(data) if t.grad is not None}


@functools.lru_cache(maxsize=None)
def _oracle(key, C, dino_dtype, policy="weight_guided", dtype=torch.float64):
    """The torch route on the CPU (computed once per case and shared)."""
    data = ri.convert(_raw(key, C), dtype=dtype, dino_dtype=dino_dtype)
    res = _loss(ri.shipped(invalid_policy=policy), native=False)(data)
    res["rec_loss"].backward()
    return {k: v.detach() for k, v in res.items()}, _grads(data)


def _native(gpu, key, C=64, dino_dtype=None, cfg=None, raw=None, upstream=None):
    data = ri.convert(raw if raw is not None else _raw(key, C), device=gpu, dtype=torch.float32,
                      dino_dtype=dino_dtype)
    loss = _loss(cfg or ri.shipped())
    res = loss(data)
    res["rec_loss"].backward(upstream)
    return loss, data, res


def _compare(what, got_m, got_g, key, C, dino_dtype, policy="weight_guided"):
    m64, g64 = _oracle(key, C, dino_dtype, policy)
    m32, g32 = _oracle(key, C, dino_dtype, policy, torch.float32)
    rows = [(k, rel_l2(got_m[k], m64[k]), rel_l2(m32[k], m64[k])) for k in m64]
    assert set(got_g) == set(g64)
    rows += [(k, rel_l2(got_g[k].float(), g64[k]), rel_l2(g32[k], g64[k])) for k in g64]
    for k, r, e in rows:
        print(f"{what} {k}: native rel-L2 {r:.3e}, f32 torch route {e:.3e}")
    for k, r, e in rows:
        if k in got_g and got_g[k].dtype == BF:
            _compare_bf16(f"{what} {k}", got_g[k], g64[k])
        else:
            assert r <= BOUND, f"{what} {k}: rel-L2 {r:.3e} > {BOUND}"


def _compare_bf16(what, got, want64):
    """A gradient stored in bf16 (d dino of bf16 features, the leaf's own type: autograd would
    cast an f32 one) carries the format's rounding, up to 2^-9 per element, so BOUND cannot hold
    against the unrounded oracle (measured 1.6e-3 on MI355X).  It is held to the oracle rounded
    the same way instead: an element can differ only if the exact value lies within the f32
    kernel's error (BOUND, relative) of a rounding boundary; boundaries are at least 2^-8
    apart in relative terms, so at most a share 2 * BOUND / 2^-8 of the elements may differ
    (plus one element of slack), each by one bf16 step."""
    got = got.detach().cpu()
    want = want64.to(BF)
    diff = got != want
    n_diff = int(diff.sum())
    print(f"{what}: {n_diff} of {got.numel()} bf16 elements differ from the rounded oracle")
    assert n_diff <= 1 + int(2 * BOUND / 2.0 ** -8 * got.numel()), what
    if n_diff:
        step = (got[diff].double() - want[diff].double()).abs() / want64[diff].abs()
        assert float(step.max()) <= 2.0 ** -7, what


@pytest.mark.gpu
@pytest.mark.parametrize("key,C,dino_dtype", NATIVE_CASES)
def test_native_route_against_float64(gpu, key, C, dino_dtype):
    loss, data, res = _native(gpu, key, C, dino_dtype)
    assert loss.last_route == "native"
    assert type(res["rec_loss"].grad_fn).__name__ == "_NativeReconLossBackward"
    assert list(res) == loss.get_loss_metric_names()
    for k, v in res.items():
        assert v.dim() == 0 and v.dtype == torch.float32 and (k == "rec_loss" or not v.requires_grad)
    g = _grads(data)
    assert g["coarse0.dino_features"].dtype == (dino_dtype or torch.float32)
    _compare(f"{key} C={C} {dino_dtype}", res, g, key, C, dino_dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("policy", ["strict", "none"])
def test_other_native_policies(gpu, policy):
    cfg = ri.shipped(invalid_policy=policy)
    kw = {"invalid_above": 0.9} if policy == "strict" else {}
    raw = _raw("odd", **kw)
    loss, data, res = _native(gpu, "odd", cfg=cfg, raw=raw)
    assert loss.last_route == "native"
    ref = ri.convert(raw)
    want = _loss(cfg, native=False)(ref)
    want["rec_loss"].backward()
    g64 = _grads(ref)
    for k in want:
        r = rel_l2(res[k], want[k])
        print(f"{policy} {k}: {r:.3e}")
        assert r <= BOUND, k
    for k, t in _grads(data).items():
        r = rel_l2(t, g64[k])
        print(f"{policy} {k}: {r:.3e}")
        assert r <= BOUND, k


@pytest.mark.gpu
def test_two_scales_and_grid_targets_with_artifacts(gpu):
    for name in ("two_scales", "p8_grid_artifacts"):
        cfg, raw = ri.case(name)
        loss, data, res = _native(gpu, None, cfg=cfg, raw=raw)
        assert loss.last_route == "native"
        ref = ri.convert(raw)
        want = _loss(cfg, native=False)(ref)
        want["rec_loss"].backward()
        for k in want:
            assert rel_l2(res[k], want[k]) <= BOUND, (name, k)
        g64 = _grads(ref)
        got = _grads(data)
        assert set(got) == set(g64)
        for k in g64:
            assert rel_l2(got[k], g64[k]) <= BOUND, (name, k)


@pytest.mark.gpu
def test_median_thresholding_takes_the_torch_route(gpu):
    import numpy as np
    import os
    from conftest import GOLDEN
    golden = np.load(os.path.join(GOLDEN, "recon_loss.npz"))
    cfg, raw = ri.case("median")
    loss, data, res = _native(gpu, None, cfg=cfg, raw=raw)
    assert loss.last_route == "torch"
    assert type(res["rec_loss"].grad_fn).__name__ != "_NativeReconLossBackward"
    for k, v in res.items():
        ref = float(golden[f"median/metric/{k}"])
        assert abs(v.item() - ref) <= 1e-5 * abs(ref), k
    for lname, t in ri.leaves(data):
        sub = torch.from_numpy(golden[f"median/sub/{lname}"])
        assert rel_l2(ri.subset(t.grad.reshape(-1)), sub) <= 1e-5, lname


@pytest.mark.gpu
def test_masks_and_branches(gpu):
    """d rgb is exactly zero wherever no pixel of the 3 x 3 neighbourhood (the SSIM window)
    selected the view while valid -- masked pixels and non-argmin views included; a view built
    as 1 - rgb_gt drives 1 - SSIM past 1 (zero SSIM gradient, the L1 gradient stays); depth
    outside [1e-3, 80] gets a zero depth gradient."""
    from scenedino_amd.losses import reconstruction_loss as rl
    raw = _raw("p8")
    n, pc, h, w, nv, K = ri.SHAPES["p8"]
    c = raw["coarse"][0]
    c["rgb"][:, 0, :, :, 0] = 1 - raw["rgb_gt"][:, 0]      # patch 0, view 0: anti-correlated
    c["rgb"][:, 0, :, :, 1:] += 2.0                          # ... and the only candidate there
    c["depth"][0, 1, 0, :4] = torch.tensor([5e-4, 90.0, 0.0, 81.0])
    loss, data, res = _native(gpu, None, raw=raw)
    assert loss.last_route == "native"
    ref = ri.convert(raw)
    want = _loss(ri.shipped(), native=False)(ref)
    want["rec_loss"].backward()
    g64, got = _grads(ref), _grads(data)
    for k in g64:
        assert rel_l2(got[k], g64[k]) <= BOUND, k
    d_rgb = got["coarse0.rgb"].cpu()
    r0 = ref["coarse"][0]
    invalid = rl.POLICIES["weight_guided"](r0["invalid"], weights=r0["weights"])[..., 0]
    gt = ref["rgb_gt"].unsqueeze(-2).expand(r0["rgb"].shape)
    e = rl.l1_ssim(r0["rgb"].detach().permute(0, 1, 4, 5, 2, 3).reshape(-1, 3, h, w),
                   gt.permute(0, 1, 4, 5, 2, 3).reshape(-1, 3, h, w)).view(n, pc, nv, h, w)
    active = torch.nn.functional.one_hot(e.argmin(2), nv).permute(0, 1, 4, 2, 3).bool() \
        & ~invalid.unsqueeze(2)
    assert 0.05 < float(invalid.float().mean()) < 0.6
    touched = torch.nn.functional.max_pool2d(active.float().reshape(-1, 1, h, w), 3, 1, 1)
    touched = touched.view(n, pc, nv, h, w).permute(0, 1, 3, 4, 2).bool()
    assert bool((~touched).any()) and bool(touched.any())
    assert not d_rgb[~touched].any()
    # the anti-correlated view where it is selected and 1 - SSIM is clamped at 1 in the whole
    # 3 x 3 neighbourhood and every channel: the pure L1 gradient
    x, y = r0["rgb"].detach()[0, 0, :, :, 0], ref["rgb_gt"][0, 0]
    clamped = (rl.ssim_term(x.permute(2, 0, 1)[None], y.permute(2, 0, 1)[None]) == 0.5).all(1)
    clamped = 1 - torch.nn.functional.max_pool2d(1 - clamped.float()[None], 3, 1, 1)[0, 0]
    sel = active[0, 0, 0] & clamped.bool()
    assert int(sel.sum()) >= 8
    l1 = (0.15 / 3) * torch.sign(x - y) / (n * pc * h * w)
    assert rel_l2(d_rgb[0, 0, :, :, 0][sel], l1[sel]) <= BOUND
    d_depth = got["coarse0.depth"].cpu()
    assert not d_depth[0, 1, 0, :4].any() and bool(d_depth[0, 1, 1].all())


@pytest.mark.gpu
def test_upstream_scale_and_repeat(gpu):
    """A GradScaler-sized upstream gradient (read from device memory) scales every gradient;
    two runs give the same bits."""
    _, d1, r1 = _native(gpu, "p8")
    _, d2, r2 = _native(gpu, "p8")
    _, d3, _ = _native(gpu, "p8", upstream=torch.tensor(65536.0, device=gpu))
    for k in r1:
        assert torch.equal(r1[k], r2[k]), k
    g1, g2, g3 = _grads(d1), _grads(d2), _grads(d3)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
        assert rel_l2(g3[k], g1[k] * 65536.0) <= 4 * 2.0 ** -24, k


@pytest.mark.gpu
def test_validation_call_and_requires_grad_subsets(gpu):
    loss = _loss(ri.shipped())
    data = ri.convert(_raw("odd"), device=gpu, dtype=torch.float32, grad=False)
    res = loss(data)
    assert loss.last_route == "native" and res["rec_loss"].grad_fn is None
    full = _native(gpu, "odd")
    data = ri.convert(_raw("odd"), device=gpu, dtype=torch.float32, grad=False)
    data["coarse"][0]["dino_features_downsampled"].requires_grad_(True)
    res = loss(data)
    assert torch.equal(res["rec_loss"], full[2]["rec_loss"])
    res["rec_loss"].backward()
    c, f = data["coarse"][0], full[1]["coarse"][0]
    assert c["rgb"].grad is None and c["depth"].grad is None and c["dino_features"].grad is None
    assert torch.equal(c["dino_features_downsampled"].grad, f["dino_features_downsampled"].grad)


@pytest.mark.gpu
def test_no_host_sync(gpu):
    _native(gpu, "p8")  # library load, allocator warm-up
    data = ri.convert(_raw("p8"), device=gpu, dtype=torch.float32)
    loss = _loss(ri.shipped())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = loss(data)
        res["rec_loss"].backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert loss.last_route == "native" and bool(torch.isfinite(res["rec_loss"]))
    assert all(t.grad is not None for _, t in ri.leaves(data))


@pytest.mark.gpu
def test_graph_replay_equals_eager(gpu):
    _, d_eager, r_eager = _native(gpu, "p8")
    data = ri.convert(_raw("p8"), device=gpu, dtype=torch.float32)
    loss = _loss(ri.shipped())
    leaves = [t for _, t in ri.leaves(data)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            torch.autograd.grad(loss(data)["rec_loss"], leaves)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = loss(data)
        grads = torch.autograd.grad(res["rec_loss"], leaves)
    for t in list(res.values()) + list(grads):
        t.detach().zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in r_eager:
        assert torch.equal(res[k], r_eager[k]), k
    for (name, _), g in zip(ri.leaves(data), grads):
        assert torch.equal(g, dict(ri.leaves(d_eager))[name].grad), name


# ------------------------------------------------------------------------ the whole step
@pytest.mark.gpu
def test_end_to_end_training_step(gpu):
    """encode -> PatchRaySampler -> train-mode render -> reconstruct -> expand_dim ->
    downsample("patch") -> ReconstructionLoss (shipped config) -> backward -> Adam
    (trainer.py:180-300 on the small BTSNet of tests/test_expand_train.py's fixture)."""
    from test_dpt_train import _module as dino_module
    from test_expand_train import KN
    from scenedino_amd.common.positional_encoding import PositionalEncoding
    from scenedino_amd.common.ray_sampler import PatchRaySampler
    from scenedino_amd.models import BTSNet
    from scenedino_amd.models.prediction_heads import ResnetFC
    from scenedino_amd.renderer import NeRFRenderer
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
    sampler = PatchRaySampler(3, 80, 512, 16, snap_to_grid=True, dino_upscaled=False)
    torch.manual_seed(7)
    rays, rgb_gt, dino_gt = sampler.sample(images * 0.5 + 0.5, poses, Ks,
                                           dino_features=net.grid_l_loss_features[0])
    r = NeRFRenderer(n_coarse=32, lindisp=True, hard_alpha_cap=True)
    r.z_jitter = torch.rand(512, 32, generator=torch.Generator().manual_seed(3)).to(gpu)
    rd = r.bind_parallel(net).train()(rays, want_weights=True, want_alphas=True,
                                      want_rgb_samps=True)
    rd["rgb_gt"], rd["rays"], rd["dino_gt"] = rgb_gt, rays, dino_gt.float()
    rd = sampler.reconstruct(rd, channels=3, dino_channels=64)
    coarse = rd["coarse"]
    coarse["dino_features"] = enc.expand_dim(coarse["dino_features"])
    down = enc.downsample(coarse["dino_features"], "patch")
    coarse["dino_features_downsampled"] = down[0] if isinstance(down, tuple) else down
    data = {"coarse": [coarse], "fine": [], "rgb_gt": rd["rgb_gt"], "dino_gt": rd["dino_gt"]}
    trained = [(n, p) for n, p in net.named_parameters()
               if n.startswith(("encoder.dim_reduction.", "heads.normal_head.", "encoder.decoder."))]
    assert len(trained) > 8
    opt = torch.optim.Adam([p for _, p in trained], lr=1e-4)
    opt.zero_grad(set_to_none=True)
    loss = _loss(ri.shipped())
    res = loss(data)
    assert loss.last_route == "native", loss.native_domain(data)
    with torch.no_grad():
        want = _loss(ri.shipped(), native=False)(data)
    for k in res:
        print(f"step {k}: native {res[k].item():.7f} torch route {want[k].item():.7f}")
    assert rel_l2(res["rec_loss"], want["rec_loss"]) <= 1e-5
    res["rec_loss"].backward()
    for n, p in trained:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        assert float(p.grad.abs().max()) > 0, n
    before = [p.detach().clone() for _, p in trained]
    opt.step()
    assert all(not torch.equal(p.detach(), b) for (_, p), b in zip(trained, before))
