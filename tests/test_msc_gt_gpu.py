"""GPU: the multi-scale-crop target kernel (sd_msc_gt, csrc/sdhip_msc.hip) against the torch
route of MultiScaleCropGT evaluated in float64 on the same inputs.

Bar: the kernel's rel-L2 error against the float64 route is at most twice the error of the
float32 torch route against the same float64 result (the fused kernel sums up to 16 products per
view in another order).  Both are printed per case; DESIGN §4 holds the measured values.
Pixels whose float64 source coordinate lies within 1e-3 of a rounding boundary of the validity
test (-0.5 and W - 0.5 in x, -0.5 and H - 0.5 in y) are left out of both errors; the tests
assert on the inputs, before any GPU call, that these are at most 0.1 % of a case's pixels.
"""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from test_dpt import det_fill
from test_encoder import CONF
from test_vit import init_vit

# (B, V, C, (hp, wp), (H, W))
SHAPES = [(2, 4, 24, (3, 5), (24, 40)),
          (1, 4, 20, (3, 4), (18, 52)),    # non-integer scales, a partial wave, C % 16 != 0
          (1, 3, 8, (2, 2), (7, 9)),
          (1, 2, 8, (2, 3), (16, 24)),     # no augmented view
          (1, 4, 768, (2, 40), (32, 640))]  # the production row width and channel count
KINDS = ["identity", "zoom", "flipcrop", "outside", "projective"]
CASES = [(s, k) for s in SHAPES for k in (KINDS if s[1] > 2 else ["none"])]
UP = dict(CONF, mode="upsample-gt", downsampler_arch=None, upsampler_arch="multiscale-crop",
          separate_gt_version=None, image_size=[32, 64])


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.load()
    return "cuda"


def _up():
    from scenedino_amd.models.backbones.dino import upsampler
    return upsampler


def transform(kind, H, W, j):
    """Fixed transform number j of a kind, image -> view pixel coordinates (float32)."""
    up = _up()
    if kind == "identity":
        return torch.eye(3)
    if kind in ("zoom", "flipcrop"):  # a crop that leaves a border invalid
        w, h = max(2, round(0.61 * W) - j), max(2, round(0.57 * H) - j)
        box = [min(round(0.17 * W) + j, W - w), min(round(0.22 * H), H - h), w, h]
        return up.view_transforms(torch.tensor([[box]]), torch.tensor([[kind == "flipcrop"]]),
                                  (H, W))[0, 0]
    if kind == "outside":
        return torch.tensor([[1.0, 0, 10.0 * W + j], [0, 1, 0], [0, 0, 1]])
    if kind == "projective":  # p2 != 1
        return torch.tensor([[1.31, 0.02, -0.083 * W - j], [0.01, 1.23, -0.071 * H],
                             [0.13 / W, 0.09 / H, 1.07]])
    raise KeyError(kind)


def case_inputs(shape, kind, seed=0):
    B, V, C, (hp, wp), (H, W) = shape
    g = torch.Generator().manual_seed(100 + seed + C)
    feat = torch.randn(B, V, C, hp, wp, generator=g)
    T = torch.stack([torch.stack([transform(kind, H, W, b * (V - 2) + k) for k in range(V - 2)])
                     for b in range(B)]) if V > 2 else torch.zeros(B, 0, 3, 3)
    return feat, T.float().contiguous()


def keep_mask(T, H, W):
    """(B, 1, H, W) bool on the CPU: False within 1e-3 of a rounding boundary of any view."""
    B, k = T.shape[:2]
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64),
                          torch.arange(W, dtype=torch.float64), indexing="ij")
    p = torch.stack([u, v, torch.ones_like(u)], -1).view(1, 1, H * W, 3) @ \
        T.double().cpu().transpose(-1, -2).view(B, k, 3, 3)
    x, y = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
    near = ((x + 0.5).abs() < 1e-3) | ((x - (W - 0.5)).abs() < 1e-3) | \
           ((y + 0.5).abs() < 1e-3) | ((y - (H - 0.5)).abs() < 1e-3)
    keep = ~near.any(1).view(B, 1, H, W)
    assert (~keep).double().mean().item() <= 1e-3, "fixed transforms sit on a rounding boundary"
    return keep


def rel(a, ref, keep):
    k = keep.to(ref.device)
    return (((a.double() - ref) * k).norm() / (ref * k).norm()).item()


def check(native, f32, f64, keep, what):
    e_n, e_t = rel(native, f64, keep), rel(f32, f64, keep)
    print(f"{what}: kernel rel-L2 {e_n:.3e}, f32 torch route {e_t:.3e}")
    assert bool(torch.isfinite(native).all())
    assert e_t > 0 and e_n <= 2 * e_t, f"{what}: kernel {e_n:.3e} > 2 x {e_t:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind", CASES, ids=[f"{s[2]}c{s[4][0]}x{s[4][1]}-{k}" for s, k in CASES])
def test_kernel_against_float64_route(gpu, shape, kind):
    from scenedino_amd import _lib
    B, V, C, _, (H, W) = shape
    feat, T = case_inputs(shape, kind)
    keep = keep_mask(T, H, W)  # asserts on the inputs before any GPU call
    w = _up().MultiScaleCropGT(None, num_views=V, image_size=(H, W))
    feat, T = feat.to(gpu), T.to(gpu)
    f64 = w.accumulate(feat.double(), T.double(), H, W)
    f32 = w.accumulate(feat, T, H, W)
    out = _lib.msc_gt(feat, T, H, W)
    assert out.shape == (B, C, H, W) and out.dtype == torch.float32
    check(out, f32, f64, keep, f"{shape} {kind}")
    assert torch.equal(out, w.combine(feat, T, H, W)) and w.last_route == "native"


@pytest.mark.gpu
def test_validity_shows_in_one_hot_grids(gpu):
    """View k's grid is one in channel k and zero elsewhere, no normalisation: channel k of the
    output is view k's weight over the number of valid views."""
    from scenedino_amd import _lib
    B, V, (hp, wp), (H, W) = 2, 5, (3, 5), (24, 40)
    feat = torch.zeros(B, V, V, hp, wp)
    for k in range(V):
        feat[:, k, k] = 1.0
    kinds = ["zoom", "flipcrop", "projective", "outside", "zoom", "identity"]
    T = torch.stack([transform(k, H, W, j) for j, k in enumerate(kinds)]).view(B, 3, 3, 3)
    keep = keep_mask(T, H, W).to(gpu)
    w = _up().MultiScaleCropGT(None, num_views=V, image_size=(H, W))
    feat, T = feat.to(gpu), T.contiguous().to(gpu)
    want = w.accumulate(feat.double(), T.double(), H, W, normalize=False)
    got = _lib.msc_gt(feat, T, H, W, normalize=False)
    assert ((got.double() - want) * keep).abs().max().item() <= 1e-5
    counts = (want[:, :3] > 0).sum(1)  # every number of valid augmented views occurs
    assert set(counts.unique().tolist()) >= {0, 1, 2}
    assert ((got[:, 3:].sum(1).double() * (2 + (want[:, :3] > 0).sum(1)) - 2) * keep[:, 0]
            ).abs().max().item() <= 1e-5


@pytest.mark.gpu
def test_repeat_stream_and_graph_are_bit_equal(gpu):
    from scenedino_amd import _lib
    shape = SHAPES[0]
    (H, W) = shape[4]
    feat, T = case_inputs(shape, "zoom")
    feat, T = feat.to(gpu), T.to(gpu)
    a = _lib.msc_gt(feat, T, H, W)
    assert torch.equal(a, _lib.msc_gt(feat, T, H, W))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b = _lib.msc_gt(feat, T, H, W)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(a, b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = _lib.msc_gt(feat, T, H, W)
    for _ in range(2):
        c.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, c)


@pytest.mark.gpu
def test_rejections_take_the_torch_route(gpu):
    from scenedino_amd import _lib
    shape = SHAPES[0]
    B, V, C, (hp, wp), (H, W) = shape
    feat, T = case_inputs(shape, "zoom")
    feat, T = feat.to(gpu), T.to(gpu)
    w = _up().MultiScaleCropGT(None, num_views=V, image_size=(H, W))
    want = w.combine(feat, T, H, W)
    assert w.last_route == "native" and w.last_reason is None
    strided = feat.transpose(-1, -2).contiguous().transpose(-1, -2)
    with pytest.raises(ValueError, match="feat must be contiguous"):
        _lib.msc_gt(strided, T, H, W)
    with pytest.raises(TypeError, match="feat must be torch.float32"):
        _lib.msc_gt(feat.half(), T, H, W)
    many = torch.randn(1, 9, 4, hp, wp, device=gpu)
    T9 = torch.eye(3, device=gpu).expand(1, 7, 3, 3).contiguous()
    with pytest.raises(RuntimeError, match="sd_msc_gt: invalid argument"):
        _lib.msc_gt(many, T9, H, W)
    got = w.combine(strided, T, H, W)
    assert w.last_route == "torch" and "contiguous" in w.last_reason
    assert (got - want).abs().max().item() <= 1e-5
    got = w.combine(feat.double(), T.double(), H, W)
    assert w.last_route == "torch" and got.dtype == torch.float64
    w9 = _up().MultiScaleCropGT(None, num_views=9, image_size=(H, W))
    assert w9.combine(many, T9, H, W).shape == (1, 4, H, W) and w9.last_route == "torch"
    w.native = False
    w.combine(feat, T, H, W)
    assert w.last_route == "torch" and w.last_reason == "native = False"


# ------------------------------------------------------------------- module and step
BOXES = [[[6, 3, 44, 22], [14, 8, 40, 20]], [[0, 2, 50, 28], [20, 5, 36, 18]]]
FLIPS = [[False, True], [True, False]]


def _module(flip_avg_gt=False):
    from scenedino_amd.models.backbones import make_backbone
    m = make_backbone(dict(UP, flip_avg_gt=flip_avg_gt), upsample_gt=True).eval()
    init_vit(m.encoder.model.vit, 21)
    det_fill(m.decoder, 22)
    m.gt_wrapper.sample_views = lambda n: (torch.tensor(BOXES)[:n], torch.tensor(FLIPS)[:n])
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("flip_avg_gt", [False, True])
def test_module_ground_truth_pass(gpu, flip_avg_gt):
    m = _module(flip_avg_gt).to(gpu)
    wr = m.gt_wrapper
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(2, 3, 32, 64, generator=g) * 2 - 1).to(gpu)
    T = _up().view_transforms(torch.tensor(BOXES), torch.tensor(FLIPS), (32, 64))
    keep = keep_mask(T, 32, 64)
    if flip_avg_gt:
        keep = keep & keep.flip(-1)
    seen, combine = [], wr.combine
    wr.combine = lambda f, t, h, w: (seen.append((f, t)), combine(f, t, h, w))[1]
    out = m(x, ground_truth=True)
    assert wr.last_route == "native" and len(out) == 1 and len(seen) == 1 + flip_avg_gt
    assert out[0].shape == (2, 384, 32, 64) and out[0].dtype == torch.float32
    assert (out[0].norm(dim=1) - 1).abs().max().item() <= 1e-5
    wr.native = False
    f32 = m(x, ground_truth=True)[0]
    assert wr.last_route == "torch"

    def route(dtype):
        r = [wr.accumulate(f.to(dtype), t.to(dtype), 32, 64) for f, t in seen[:1 + flip_avg_gt]]
        return F.normalize(r[1].flip([-1]) + r[0], dim=1) if flip_avg_gt else r[0]

    assert torch.equal(route(torch.float32), f32)  # the encoder's grids repeat bit for bit
    check(out[0], f32, route(torch.float64), keep, f"module flip_avg_gt={flip_avg_gt}")


@pytest.mark.gpu
def test_one_training_step_on_upsampled_targets(gpu):
    """encode(ids_loss=[0, 1]) -> PatchRaySampler(dino_upscaled=True) -> train-mode render ->
    reconstruct -> expand_dim -> ReconstructionLoss -> backward: the per-pixel targets reach the
    loss and the field head gets gradients."""
    import _recon_inputs as ri
    from test_expand_train import KN
    from scenedino_amd.common.positional_encoding import PositionalEncoding
    from scenedino_amd.common.ray_sampler import PatchRaySampler
    from scenedino_amd.losses import make_loss
    from scenedino_amd.models import BTSNet
    from scenedino_amd.models.prediction_heads import ResnetFC
    from scenedino_amd.renderer import NeRFRenderer
    enc = _module()
    torch.manual_seed(2)
    head = ResnetFC(d_in=256 + 39, d_out=65, n_blocks=0, d_hidden=128)
    conf = {"predict_dino": True, "dino_dims": 64, "learn_empty": False, "code_mode": "z",
            "inv_z": True, "z_near": 3, "z_far": 80, "sample_color": True, "precision": "fp32"}
    net = BTSNet(conf, enc, PositionalEncoding(6, 3, 1.5, True), {"normal_head": head},
                 final_pred_head="normal_head").to(gpu).train()
    for p in enc.decoder.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(0)
    images = (torch.rand(1, 2, 3, 32, 64, generator=g) * 2 - 1).to(gpu)
    Ks = KN.view(1, 1, 3, 3).expand(1, 2, 3, 3).contiguous().to(gpu)
    poses = torch.eye(4).view(1, 1, 4, 4).repeat(1, 2, 1, 1)
    poses[0, 1, 0, 3] = 0.3
    poses = poses.to(gpu)
    net.encode(images, Ks, poses, ids_encoder=[0], ids_render=[0, 1], ids_loss=[0, 1])
    targets = net.grid_l_loss_features
    assert enc.gt_wrapper.last_route == "native"
    assert len(targets) == 1 and targets[0].shape == (1, 2, 384, 32, 64)
    sampler = PatchRaySampler(3, 80, 512, 16, snap_to_grid=True, dino_upscaled=True)
    torch.manual_seed(7)
    rays, rgb_gt, dino_gt = sampler.sample(images * 0.5 + 0.5, poses, Ks, dino_features=targets[0])
    assert dino_gt.shape == (1, 512, 384)
    r = NeRFRenderer(n_coarse=32, lindisp=True, hard_alpha_cap=True)
    r.z_jitter = torch.rand(512, 32, generator=torch.Generator().manual_seed(3)).to(gpu)
    rd = r.bind_parallel(net).train()(rays, want_weights=True, want_alphas=True,
                                      want_rgb_samps=True)
    rd["rgb_gt"], rd["rays"], rd["dino_gt"] = rgb_gt, rays, dino_gt.float()
    rd = sampler.reconstruct(rd, channels=3, dino_channels=64)
    assert rd["dino_gt"].shape == (1, 2, 16, 16, 384)
    coarse = rd["coarse"]
    coarse["dino_features"] = enc.expand_dim(coarse["dino_features"])
    assert enc.downsample(coarse["dino_features"], "patch") is None
    data = {"coarse": [coarse], "fine": [], "rgb_gt": rd["rgb_gt"], "dino_gt": rd["dino_gt"]}
    loss = make_loss(ri.shipped())
    res = loss(data)
    assert loss.last_route in ("native", "torch")
    print("loss route", loss.last_route, "rec_loss", res["rec_loss"].item())
    assert bool(torch.isfinite(res["rec_loss"]))
    res["rec_loss"].backward()
    for n, p in net.heads["normal_head"].named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert float(net.heads["normal_head"].lin_in.weight.grad.abs().max()) > 0
