"""The tile render kernel's late step order (k_render_tile<.., LATE>, csrc/sdhip_tile.hip):
128-sample wave steps -- K = 64 two rays per wave, K = 128 one -- on one record buffer per
wave, the next group's tap boxes from a box pass over its part endpoints, the ray pass behind
the epilogue with every sample verified against the staged box (a miss sends the group to the
per-ray fallback).  Small scenes (the helpers of test_gpu_parity.py); tolerances: those of
test_gpu_parity.py for the same precision mode (check_lowp, alphas 2e-3, rgb_samps as
test_render_lowp_vs_reference, masks exact).
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

from _helpers import build_net
from test_gpu_parity import FP32_ATOL, check_lowp, close

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import tile_stats  # noqa: E402  (CPU arithmetic of the tap boxes)

pytestmark = pytest.mark.gpu

DEV = "cuda"
LATE, EARLY = 3, 4  # sd_render_tile_order
H, W, C = 24, 80, 256
GRID = (12, 40)       # feature grid (Hf, Wf)
GRID_BIG = (36, 120)  # the split-staging test: tap boxes past a 16-KiB tile buffer
KN = [[0.7849, 0.0, -0.0312], [0.0, 2.9391, 0.2701], [0.0, 0.0, 1.0]]
HEAD_D = {64: 64, 128: 384}
KEYS = ("depth", "dino", "rgb", "weights", "alphas", "invalid", "invalid_f", "rgb_samps")


@pytest.fixture(autouse=True)
def _hooks():
    """Every test starts at the default routing with no tile cap and leaves it so."""
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.render_tile_order(0)
    _lib.render_tile_cap(0)
    yield
    _lib.render_tile_order(0)
    _lib.render_tile_cap(0)


@functools.lru_cache(maxsize=None)
def _scene(K, grid=GRID):
    g = torch.Generator().manual_seed(300 + K)
    D = HEAD_D[K]
    return {
        "images": torch.rand(1, 1, 3, H, W, generator=g) * 2 - 1,
        "grid": torch.randn(1, C, grid[0], grid[1], generator=g),
        "W_in": torch.randn(128, C + 39, generator=g) * 0.06,
        "b_in": torch.randn(128, generator=g) * 0.1,
        "W_out": torch.randn(1 + D, 128, generator=g) * 0.1,
        "b_out": torch.randn(1 + D, generator=g) * 0.1,
        "Kn": torch.tensor(KN).view(1, 1, 3, 3),
        "pose": torch.eye(4).view(1, 1, 4, 4),
        "u": torch.rand(H * W, K, generator=g),
    }


def _render_pose(offset):
    rpose = torch.eye(4).view(1, 1, 4, 4).clone()
    if offset:  # the offset pose of test_tile_two_rays_per_wave_vs_oracle
        a = math.radians(2.0)
        rpose[0, 0, 0, 0] = math.cos(a); rpose[0, 0, 0, 2] = math.sin(a)
        rpose[0, 0, 2, 0] = -math.sin(a); rpose[0, 0, 2, 2] = math.cos(a)
        rpose[0, 0, 0, 3] = 0.5
    return rpose


@functools.lru_cache(maxsize=None)
def _rays(K, offset):
    """(H W, ray_dim) rays of the frame on the GPU."""
    from scenedino_amd.common.ray_sampler import ImageRaySampler
    s = _scene(K)
    rays, _ = ImageRaySampler(3, 80, H, W).sample(None, _render_pose(offset).to(DEV), s["Kn"].to(DEV))
    return rays[0].contiguous()


@functools.lru_cache(maxsize=None)
def _net(K, precision, grid=GRID):
    s = _scene(K, grid)
    net = build_net(s["grid"], s["W_in"], s["b_in"], s["W_out"], s["b_out"], precision, DEV)
    net.encode(s["images"].to(DEV), s["Kn"].to(DEV), s["pose"].to(DEV), ids_encoder=[0], ids_render=[0])
    return net


@functools.lru_cache(maxsize=None)
def _oracle(K, offset, R):
    from oracle import render_oracle as O
    s = _scene(K)
    w2c = torch.inverse(s["pose"])
    return O.render(_rays(K, offset)[:R].cpu(), s["u"][:R], s["grid"], w2c[:, 0], s["Kn"][:, 0],
                    s["images"] * 0.5 + 0.5, w2c, s["Kn"], s["W_in"], s["b_in"], s["W_out"],
                    s["b_out"], sb=1, hard_alpha_cap=True)


def _z(K, offset, R):
    from scenedino_amd import _lib
    return _lib.sample_z(_rays(K, offset)[:R].contiguous(), K, True, u=_scene(K)["u"][:R].to(DEV).contiguous())


def _render(net, rays, z, K, order, **kw):
    """One fused render under a step order -> (outputs, ray indices in the overflow lists)."""
    from scenedino_amd import _lib
    _lib.render_tile_order(order)
    with torch.no_grad():
        out = net.render_fused(rays.contiguous(), z, 1, True, want_weights=True, want_alphas=True,
                               want_rgb_samps=True, K=K, **kw)
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in KEYS}, _listed(net, rays.shape[0])


def _listed(net, R):
    """Rays (< R) of the 4-ray blocks in the tile kernel's overflow lists of net's last render
    (the tail of its work buffer: [ncu] counts, [ncu][cap] blocks, csrc/sdhip_render.h)."""
    work = net._last_render_work.view(torch.int32).cpu()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    cap = ((R + ncu - 1) // ncu + 64) // 4 + 1
    words = ((4 * (ncu + ncu * cap) + 15) // 16) * 16 // 4
    ovf = work[work.numel() - words:]
    cnt = ovf[:ncu]
    assert int(cnt.min()) >= 0 and int(cnt.max()) <= cap
    blocks = [int(b) for i in range(ncu) for b in ovf[ncu + i * cap: ncu + i * cap + int(cnt[i])]]
    rays = sorted({4 * b + i for b in blocks for i in range(4) if 4 * b + i < R})
    return torch.tensor(rays, dtype=torch.long)


def _mask(R, listed):
    m = torch.zeros(R, dtype=torch.bool)
    m[listed] = True
    return m


def _assert_equal(a, b, rows=None, what=""):
    for k in KEYS:
        x, y = a[k].cpu(), b[k].cpu()
        if rows is not None:
            x, y = x[rows], y[rows]
        assert torch.equal(x, y), f"{what}{k}: {int((x != y).sum())} elements differ, max |d| " \
                                  f"{float((x.double() - y.double()).abs().max()):.3g}"


def _assert_parity(c, ref, precision, rows=None):
    """c against ref (both in render_fused's layout) within test_gpu_parity.py's 16-bit contract."""
    sel = (lambda t: t.cpu()) if rows is None else (lambda t: t.cpu()[rows])
    cc = {"depth": sel(c["depth"]), "dino_features": sel(c["dino"]), "rgb": sel(c["rgb"]),
          "weights": sel(c["weights"])}
    rr = {"depth": sel(ref["depth"]), "dino_features": sel(ref["dino"]), "rgb": sel(ref["rgb"]),
          "weights": sel(ref["weights"])}
    da = float((sel(c["alphas"]).double() - sel(ref["alphas"]).double()).abs().max())
    print(f"parity {precision}: weights {float((cc['weights'].double() - rr['weights'].double()).abs().max()):.3g}"
          f" depth {float((cc['depth'].double() - rr['depth'].double()).abs().max()):.3g} alphas {da:.3g}"
          f" rgb_samps {float((sel(c['rgb_samps']).double() - sel(ref['rgb_samps']).double()).abs().max()):.3g}")
    check_lowp(cc, rr, precision)
    assert da <= 2e-3
    assert torch.equal(sel(c["invalid"]), sel(ref["invalid"]))
    assert torch.equal(sel(c["invalid_f"]), sel(ref["invalid_f"]))
    close(sel(c["rgb_samps"]), sel(ref["rgb_samps"]).numpy(), 1e-5, FP32_ATOL["rgb_samps"], "rgb_samps")


def _oracle_fused(K, offset, R):
    """The oracle's outputs in render_fused's layout."""
    ref = _oracle(K, offset, R)
    return {"depth": ref["depth"][0], "dino": ref["dino_features"][0], "rgb": ref["rgb"][0],
            "weights": ref["weights"][0], "alphas": ref["alphas"][0], "invalid": ref["invalid"][0],
            "invalid_f": ref["invalid_features"][0, ..., 0], "rgb_samps": ref["rgb_samps"][0]}


# K = 64: 3 whole 16-ray groups and a tail group of 5 rays (waves 5..7 without a ray, waves
# 0..4 with one); K = 128: 3 whole 8-ray groups and a tail of 5
SHAPES = [(64, 16 * 3 + 5), (128, 8 * 3 + 5)]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("offset", [False, True], ids=["encoder_pose", "offset_pose"])
@pytest.mark.parametrize("K,R", SHAPES)
def test_late_order_given_depths_vs_oracle(K, R, offset, precision):
    """Given depths (the ZIN kernels), a ragged ray count, both poses: every output against the
    CPU oracle."""
    c, listed = _render(_net(K, precision), _rays(K, offset)[:R], _z(K, offset, R), K, LATE)
    assert listed.numel() == 0, "sorted depths: no group may fail its verification"
    _assert_parity(c, _oracle_fused(K, offset, R), precision)


@pytest.mark.parametrize("K", [64, 128])
def test_late_order_bit_equal_to_early_order(K):
    """In-kernel depths, same seed and offset: the late order computes every sample with the
    early order's arithmetic and composites each ray's items in the same order."""
    net, rays = _net(K, "bf16"), _rays(K, True)
    kw = dict(z_seed=1234, z_offset=77)
    a, la = _render(net, rays, None, K, EARLY, **kw)
    b, lb = _render(net, rays, None, K, LATE, **kw)
    assert la.numel() == 0 and lb.numel() == 0, "a group went to the fallback kernel"
    _assert_equal(a, b)


@pytest.mark.parametrize("K", [64, 128])
def test_late_order_repeat_launch_bit_equal(K):
    net, rays = _net(K, "bf16"), _rays(K, True)
    kw = dict(z_seed=99, z_offset=0)
    a, _ = _render(net, rays, None, K, LATE, **kw)
    b, _ = _render(net, rays, None, K, LATE, **kw)
    _assert_equal(a, b)


def _cpu_taps(K, offset, R, z, grid=GRID):
    return tile_stats.taps(_rays(K, offset)[:R].cpu().numpy(), z.cpu().numpy(), np.array(KN, np.float32),
                           grid[1], grid[0], frac=True)


@pytest.mark.parametrize("K", [64, 128])
def test_late_order_verification_sends_unsorted_groups_to_fallback(K):
    """Depths not sorted along the ray (every 32-sample part of rays 16..31 and 64..79 shuffled
    by a seeded permutation): interior samples leave the box of their part's endpoints, the
    late ray pass flags those groups and the per-ray kernel renders them.  Rays of groups that
    were not flagged: bit-equal to the early order (which stages the boxes of all samples);
    flagged rays: the per-ray kernel's result, within the 16-bit contract of the early order's."""
    R = 16 * 6  # whole groups: the early order of the comparison takes the tile kernel too
    z = _z(K, True, R).clone()
    g = torch.Generator().manual_seed(7)
    shuffled = list(range(16, 32)) + list(range(64, 80))
    for r in shuffled:
        for p in range(K // 32):
            z[r, 32 * p: 32 * p + 32] = z[r, 32 * p: 32 * p + 32][torch.randperm(32, generator=g).to(DEV)]
    # CPU: the permutation leaves taps outside the endpoint boxes -- of the rays' own parts
    # and of their whole groups (the union the kernel verifies against)
    x0, y0, fx, fy = _cpu_taps(K, True, R, z)
    assert tile_stats.endpoint_misses(x0, y0)[shuffled].any()
    GR = 16 if K == 64 else 8
    cpu_flag = tile_stats.groups_flagged(x0, y0, fx, fy, GR)
    assert cpu_flag[[r // GR for r in shuffled]].any()
    net, rays = _net(K, "bf16"), _rays(K, True)[:R]
    a, la = _render(net, rays, z, K, EARLY)
    b, lb = _render(net, rays, z, K, LATE)
    assert la.numel() == 0
    assert lb.numel() > 0, "no group was sent to the fallback: the verification path did not run"
    flagged = _mask(R, lb)
    assert flagged[shuffled].any() and not bool(flagged.all())
    _assert_equal(a, b, rows=~flagged, what="unflagged ")
    _assert_parity(b, a, "bf16", rows=flagged)


@pytest.mark.parametrize("K,caps", [(64, (24, 16)), (128, (24, 16))])
def test_late_order_split_staging_bit_equal(K, caps):
    """Tile buffers capped (sd_render_tile_cap) so that groups are staged by halves and by
    quarters: rays rendered from the tiles are bit-equal to the uncapped launch's (rays of
    groups whose quarters do not fit either are the fallback kernel's)."""
    from scenedino_amd import _lib
    R = H * W
    z = _z(K, True, R)
    x0, y0, _, _ = _cpu_taps(K, True, R, z, GRID_BIG)
    GR = 16 if K == 64 else 8
    shares = np.array([tile_stats.split_shares(x0, y0, GR, c * 1024) for c in caps])
    print("caps KiB", caps, "whole / halves / quarters / fallback", shares.round(3).tolist())
    assert shares[:, 1].max() > 0 and shares[:, 2].max() > 0, "the caps split no group by halves / quarters"
    net, rays = _net(K, "bf16", GRID_BIG), _rays(K, True)
    u, lu = _render(net, rays, z, K, LATE)
    assert lu.numel() == 0
    for cap in caps:
        _lib.render_tile_cap(cap * 1024)
        c, lc = _render(net, rays, z, K, LATE)
        _lib.render_tile_cap(0)
        flagged = _mask(R, lc)
        assert float(flagged.float().mean()) < 0.5, f"cap {cap} KiB: most rays went to the fallback"
        _assert_equal(u, c, rows=~flagged, what=f"cap {cap} KiB ")
