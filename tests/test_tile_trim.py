"""The instruction trims of the tile render kernel's item (k_render_tile, csrc/sdhip_tile.hip;
sd_softplus_fast / sd_code_frags, csrc/sdhip_render.h), each pinned against the per-ray kernel
k_render_proj, which shares the two helpers but neither the LDS tap addresses nor the
block-diagonal blend fragments.  A render goes to k_render_proj alone when the tile buffers
are capped below the tile kernel's minimum (sd_render_tile_cap(1024): sd_render_tile_ok says
no, as for any shape the tile kernel does not take).

Tolerances: the 16-bit contract of test_gpu_parity.py (check_lowp; alphas 2e-3, as
test_tile_late.py), masks exact; where both kernels run the same arithmetic on the same
inputs -- (a): alpha and weight of a constant sigma -- bit equality.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from _helpers import build_net
from test_gpu_parity import check_lowp
from test_tile_late import KN, _render_pose

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import tile_stats  # noqa: E402  (CPU arithmetic of the tap boxes)

pytestmark = pytest.mark.gpu

DEV = "cuda"
K, C, D = 64, 256, 64
GR = 16  # rays per group of the K = 64 route (two per wave)
KEYS = ("depth", "dino", "rgb", "weights", "alphas", "invalid", "invalid_f")

# LDS image of the K = 64 kernel (sdhip_tile.hip: st_l_rec(2), st_rec_bytes(128, late),
# st_tile_bytes): the tile buffers' first byte and their size
TILE0 = 512 + 16 * 272 + 64 + 8 * 2 * 32 * 2 + 8 * 128 * 40 + 16
TILE_BYTES = ((160 * 1024 - TILE0) // 2 // 1024) * 1024
TEX = 288


@pytest.fixture(autouse=True)
def _hooks():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib
    _lib.render_tile_order(0)
    _lib.render_tile_cap(0)
    yield
    _lib.render_tile_order(0)
    _lib.render_tile_cap(0)


@functools.lru_cache(maxsize=None)
def _weights():
    g = torch.Generator().manual_seed(511)
    return {"W_in": torch.randn(128, C + 39, generator=g) * 0.06, "b_in": torch.randn(128, generator=g) * 0.1,
            "W_out": torch.randn(1 + D, 128, generator=g) * 0.1, "b_out": torch.randn(1 + D, generator=g) * 0.1}


@functools.lru_cache(maxsize=None)
def _frame(H, W, grid, offset):
    """Images, feature grid, the frame's rays and given depths (seeded)."""
    from scenedino_amd import _lib
    from scenedino_amd.common.ray_sampler import ImageRaySampler
    g = torch.Generator().manual_seed(97 + H + grid[1])
    Kn = torch.tensor(KN).view(1, 1, 3, 3)
    rays, _ = ImageRaySampler(3, 80, H, W).sample(None, _render_pose(offset).to(DEV), Kn.to(DEV))
    rays = rays[0].contiguous()
    u = torch.rand(H * W, K, generator=g)
    return {"images": torch.rand(1, 1, 3, H, W, generator=g) * 2 - 1,
            "grid": torch.randn(1, C, grid[0], grid[1], generator=g), "Kn": Kn, "rays": rays,
            "z": _lib.sample_z(rays, K, True, u=u.to(DEV).contiguous())}


def _net(f, w, precision):
    net = build_net(f["grid"], w["W_in"], w["b_in"], w["W_out"], w["b_out"], precision, DEV)
    net.encode(f["images"].to(DEV), f["Kn"].to(DEV), torch.eye(4).view(1, 1, 4, 4).to(DEV), ids_encoder=[0],
               ids_render=[0])
    return net


def _render(net, rays, z, tile):
    """One fused render: by the tile kernel (tile) or by k_render_proj alone."""
    from scenedino_amd import _lib
    _lib.render_tile_cap(0 if tile else 1024)
    try:
        with torch.no_grad():
            out = net.render_fused(rays.contiguous(), z.contiguous(), 1, True, want_weights=True,
                                   want_alphas=True, K=K)
        torch.cuda.synchronize()
        return {k: out[k].clone().cpu() for k in KEYS}
    finally:
        _lib.render_tile_cap(0)


def _overflow_blocks(net, R):
    work = net._last_render_work.view(torch.int32)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    cap = ((R + ncu - 1) // ncu + 64) // 4 + 1
    words = ((4 * (ncu + ncu * cap) + 15) // 16) * 16 // 4
    return int(work[work.numel() - words:][:ncu].sum())


def _assert_contract(t, p, what):
    """Tile kernel t against per-ray kernel p, as test_tile_overflow_fallback_full_offset
    compares a capped frame with the uncapped one."""
    da = float((t["alphas"].double() - p["alphas"].double()).abs().max())
    dw = float((t["weights"].double() - p["weights"].double()).abs().max())
    dd = float((t["depth"].double() - p["depth"].double()).abs().max())
    print(f"{what}: tile against per-ray kernel: alphas {da:.3g} weights {dw:.3g} depth {dd:.3g}")
    for k in ("invalid", "invalid_f"):
        assert torch.equal(t[k], p[k]), k
    ren = lambda o: {"depth": o["depth"], "dino_features": o["dino"], "rgb": o["rgb"], "weights": o["weights"]}
    check_lowp(ren(t), {k: v.numpy() for k, v in ren(p).items()}, "bf16")
    assert da <= 2e-3


# ------------------------------------------------------------------ (a) softplus / alpha
SMALL = (24, 80, (6, 8))  # the frame whose first group is rendered: a grid a few texels wide
X_SIGMA = [-120.0, -20.0, 0.0, 19.999, 20.0, 20.001, 60.0, 89.0, 120.0]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("x", X_SIGMA)
def test_constant_sigma_preactivation(x, precision):
    """W_in = 0 and W_sigma = 0: every sample's sigma pre-activation is b_sigma = x, on both
    sides of softplus' threshold, where e^x underflows (-120) and where it overflows (89, 120:
    the guard-free log sees an infinite argument, its result is discarded).  Alphas and weights
    are finite, within the 16-bit tolerance of the float64 formula 1 - exp(-delta softplus(x))
    composited, and bit-equal to k_render_proj's (the same sd_softplus_fast on the same
    depths).  The last sample's alpha is the hard cap's 1, as in every render of the package:
    its delta is the reference's 1e10 pad, under which the f32 form's absolute error -- 1 + e^x
    rounds to 1 below x = -16.6, softplus = 0 for 2e-9 at x = -20 -- would be the whole alpha."""
    f = _frame(*SMALL, False)
    w = {k: v.clone() for k, v in _weights().items()}
    w["W_in"].zero_()
    w["W_out"][0].zero_()
    w["b_out"][0] = x
    net = _net(f, w, precision)
    rays, z = f["rays"][:GR], f["z"][:GR]
    t = _render(net, rays, z, True)
    assert _overflow_blocks(net, GR) == 0, "the group went to the fallback: the tile kernel did not render it"
    p = _render(net, rays, z, False)
    assert bool(torch.isfinite(t["alphas"]).all()) and bool(torch.isfinite(t["weights"]).all())
    zd = z.double().cpu()
    delta = torch.cat((zd[:, 1:] - zd[:, :-1], torch.full((GR, 1), 1e10, dtype=torch.float64)), 1)
    xs = torch.tensor(x, dtype=torch.float32).double()  # b_sigma as the kernel receives it
    sp = xs if x > 20 else torch.log1p(torch.exp(xs))
    alpha = 1 - torch.exp(-delta * sp)
    alpha[:, -1] = 1.0  # hard_alpha_cap
    T = torch.cumprod(torch.cat((torch.ones(GR, 1, dtype=torch.float64), (1 - alpha + 1e-10)[:, :-1]), 1), 1)
    da = float((t["alphas"].double().reshape(GR, K) - alpha).abs().max())
    dw = float((t["weights"].double().reshape(GR, K) - alpha * T).abs().max())
    print(f"x = {x} {precision}: against float64: alphas {da:.3g} weights {dw:.3g}; against the per-ray kernel: "
          f"alphas differ {int((t['alphas'] != p['alphas']).sum())} weights differ "
          f"{int((t['weights'] != p['weights']).sum())}")
    assert da <= 2e-3 and dw <= 2e-3
    assert torch.equal(t["alphas"], p["alphas"])
    assert torch.equal(t["weights"], p["weights"])


# ------------------------------------------------------------------ (b) tap addresses
BIG = (48, 96, (72, 240))  # 288 groups: 36 per XCD, so the first 4 workgroups of an XCD take 2 steps


def test_tap_addresses_to_the_top_of_both_tile_buffers():
    """The tap base of a lane is the 18-bit LDS address field of record word q0.x plus the
    lane's offset, with the invalid flags in bits 30 / 31 of the same word.  Offset pose on a
    72 x 240 grid: the groups' tap boxes fill up to 198 of the 202 texels a tile buffer holds,
    and the groups a workgroup renders in its second step are staged in the upper buffer, so
    staged addresses run to the top of both buffers -- past 2^17 in the upper one -- under
    samples inside and outside the encoder frustum.  (Addresses: CPU model of the boxes,
    tools/tile_stats.py; flags: the kernel's invalid_features.)  The frame equals the per-ray
    kernel's within the 16-bit contract."""
    H, W, grid = BIG
    f = _frame(H, W, grid, True)
    R = H * W
    net = _net(f, _weights(), "bf16")
    t = _render(net, f["rays"], f["z"], True)
    assert _overflow_blocks(net, R) == 0, "a group went to the fallback kernel"
    # the staged LDS byte address one past the south-east tap of every sample
    x0, y0 = tile_stats.taps(f["rays"].cpu().numpy(), f["z"].cpu().numpy(), np.array(KN, np.float32), grid[1], grid[0])
    G = R // GR
    xg, yg = x0.reshape(G, -1), y0.reshape(G, -1)
    bx0, by0 = xg.min(1), yg.min(1)
    pitch = tile_stats.pitch(xg.max(1) + 2 - bx0)
    assert ((yg.max(1) + 2 - by0) * pitch * TEX <= TILE_BYTES).all(), "a box does not fit: staged by parts"
    lo = (G * np.arange(9)) // 8  # XCD x renders groups [lo[x], lo[x + 1]), workgroup b of 32 every 32nd
    xcd = np.searchsorted(lo, np.arange(G), side="right") - 1
    upper = ((np.arange(G) - lo[xcd]) // 32) % 2 == 1
    end = TILE0 + upper[:, None] * TILE_BYTES + ((yg - by0[:, None] + 1) * pitch[:, None] + (xg - bx0[:, None] + 2)) * TEX
    inv = t["invalid_f"].numpy().reshape(G, -1) != 0
    top0, top1 = int(end[~upper].max()), int(end[upper].max())
    hi = end > (1 << 17)
    print(f"tile buffers at {TILE0} and {TILE0 + TILE_BYTES}, {TILE_BYTES} B each; highest staged tap end "
          f"{top0} (lower) {top1} (upper); samples past 2^17: {int((hi & inv).sum())} flagged "
          f"{int((hi & ~inv).sum())} not")
    assert top0 <= TILE0 + TILE_BYTES and top1 <= TILE0 + 2 * TILE_BYTES
    # "the top": the last quarter of either buffer (the upper one's begins past 2^17)
    assert top0 >= TILE0 + TILE_BYTES - TILE_BYTES // 4 and top1 >= TILE0 + 2 * TILE_BYTES - TILE_BYTES // 4
    assert TILE0 + 2 * TILE_BYTES - TILE_BYTES // 4 > 1 << 17
    assert (hi & inv).any() and (hi & ~inv).any()
    _assert_contract(t, _render(net, f["rays"], f["z"], False), "tap addresses")


# ------------------------------------------------------------------ (c) B fragments
@pytest.mark.parametrize("offset", [False, True], ids=["encoder_pose", "offset_pose"])
def test_blend_fragment_positions(offset):
    """One 16-ray group on a random grid: the 16 samples of every item take each of the four
    (K-chunk, r) positions of the block-diagonal blend-weight fragments four times, and a
    weight word at a wrong position blends a sample with another sample's weights -- far
    outside the contract against the per-ray kernel, which blends with v_dot2."""
    f = _frame(*SMALL, offset)
    net = _net(f, _weights(), "bf16")
    rays, z = f["rays"][:GR], f["z"][:GR]
    t = _render(net, rays, z, True)
    assert _overflow_blocks(net, GR) == 0, "the group went to the fallback: the tile kernel did not render it"
    _assert_contract(t, _render(net, rays, z, False), "blend fragments")
