"""The per-step phases of the tile render kernel (k_render_tile, csrc/sdhip_tile.hip) after
their round-11 trims: the box pass packed onto the upper four waves (each takes a wave pair's
part endpoints), the late ray pass with slot 1's colour loads in flight under slot 0's
geometry, and the ray sums' first butterfly level on the packed f16 pairs (v_fma_mix_f32).

GPU tests: the tile kernel against the per-ray kernel k_render_proj on the same inputs (a
render goes to k_render_proj alone when the tile buffers are capped below the tile kernel's
minimum, as in test_tile_trim.py), with that file's comparison: masks bit-equal, every other
array within the 16-bit contract of test_gpu_parity.py (check_lowp; alphas 2e-3) -- the two
kernels blend the taps differently (MFMA against v_dot2), so only the masks are the same
bits; where both run the same arithmetic (capped against uncapped tile renders) the rays are
bit-equal.  Frames of 12 x 40 rays on a 16 x 48 grid, rendered once by 8 workgroups
(sd_reserve_cus: 3-4 steps per workgroup at K = 64 / 32, 7-8 at K = 128: first, middle and
last steps) and once by every CU (single-step workgroups, and most workgroups without a
group).

CPU tests (no GPU): the rewritten routines in numpy -- the f16 pair sum of the butterfly's
first level in both forms over every f16 value against the range ends and random pairs, the
butterfly's index maps, and the packed box pass's lane -> LDS word map against the per-wave
one.
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

DEV = "cuda"
C = 256
FRAME = (12, 40, (16, 48))      # H, W, feature grid (Hf, Wf)
FRAME_BIG = (24, 80, (36, 120))  # tap boxes past a 16-KiB tile buffer (test_tile_late.py)
GROUP = {32: 16, 64: 16, 128: 8}  # rays per group of the default routing
KEYS = ("depth", "dino", "rgb", "weights", "alphas", "invalid", "invalid_f")
TEX = 288


@pytest.fixture
def hooks():
    """Default routing, no tile cap, no CU reservation, before and after."""
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from scenedino_amd import _lib

    def reset():
        _lib.render_tile_order(0)
        _lib.render_tile_cap(0)
        _lib.reserve_cus(0)
    reset()
    yield
    reset()


@functools.lru_cache(maxsize=None)
def _scene(K, D, frame):
    H, W, grid = frame
    g = torch.Generator().manual_seed(1100 + K + D + grid[1])
    return {"images": torch.rand(1, 1, 3, H, W, generator=g) * 2 - 1,
            "grid": torch.randn(1, C, grid[0], grid[1], generator=g),
            "W_in": torch.randn(128, C + 39, generator=g) * 0.06, "b_in": torch.randn(128, generator=g) * 0.1,
            "W_out": torch.randn(1 + D, 128, generator=g) * 0.1, "b_out": torch.randn(1 + D, generator=g) * 0.1,
            "Kn": torch.tensor(KN).view(1, 1, 3, 3), "u": torch.rand(H * W, K, generator=g)}


@functools.lru_cache(maxsize=None)
def _net(K, D, precision, frame):
    s = _scene(K, D, frame)
    net = build_net(s["grid"], s["W_in"], s["b_in"], s["W_out"], s["b_out"], precision, DEV)
    net.encode(s["images"].to(DEV), s["Kn"].to(DEV), torch.eye(4).view(1, 1, 4, 4).to(DEV), ids_encoder=[0],
               ids_render=[0])
    return net


@functools.lru_cache(maxsize=None)
def _rays(offset, frame):
    from scenedino_amd.common.ray_sampler import ImageRaySampler
    H, W, _ = frame
    Kn = torch.tensor(KN).view(1, 1, 3, 3)
    rays, _ = ImageRaySampler(3, 80, H, W).sample(None, _render_pose(offset).to(DEV), Kn.to(DEV))
    return rays[0].contiguous()


@functools.lru_cache(maxsize=None)
def _z(K, D, offset, frame):
    """Given depths of the frame, sorted along every ray (seeded jitter)."""
    from scenedino_amd import _lib
    return _lib.sample_z(_rays(offset, frame), K, True, u=_scene(K, D, frame)["u"].to(DEV).contiguous())


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _listed(net, R, slots):
    """Rays (< R) of the 4-ray blocks in the tile kernel's overflow lists of net's last render
    (the tail of its work buffer: [slots] counts, [slots][cap] blocks, csrc/sdhip_render.h;
    slots = the tile grid, one workgroup per unreserved CU)."""
    work = net._last_render_work.view(torch.int32).cpu()
    cap = ((R + slots - 1) // slots + 64) // 4 + 1
    words = ((4 * (slots + slots * cap) + 15) // 16) * 16 // 4
    ovf = work[work.numel() - words:]
    cnt = ovf[:slots]
    assert int(cnt.min()) >= 0 and int(cnt.max()) <= cap
    blocks = [int(b) for i in range(slots) for b in ovf[slots + i * cap: slots + i * cap + int(cnt[i])]]
    assert len(blocks) == len(set(blocks)), "a block is listed twice"
    return sorted({4 * b + i for b in blocks for i in range(4) if 4 * b + i < R})


def _render(net, rays, z, K, route="tile", cap=0, slots=None, **kw):
    """One fused render by the tile kernel (route "tile", its buffers capped at cap bytes) or by
    k_render_proj alone ("ray") -> (outputs on the CPU, rays in the overflow lists)."""
    from scenedino_amd import _lib
    _lib.render_tile_cap(cap if route == "tile" else 1024)
    try:
        with torch.no_grad():
            out = net.render_fused(rays.contiguous(), None if z is None else z.contiguous(), 1, True,
                                   want_weights=True, want_alphas=True, K=K, **kw)
        torch.cuda.synchronize()
        listed = _listed(net, rays.shape[0], slots or _ncu()) if route == "tile" else []
        return {k: out[k].clone().cpu() for k in KEYS}, listed
    finally:
        _lib.render_tile_cap(0)


def _rows(o, rows):
    return o if rows is None else {k: v[rows] for k, v in o.items()}


def _assert_contract(t, p, precision, what, rows=None):
    """test_tile_trim.py's comparison of the tile kernel with the per-ray kernel: masks equal,
    the rest within the 16-bit contract.  Figures printed before the assertions."""
    t, p = _rows(t, rows), _rows(p, rows)
    d = {k: float((t[k].double() - p[k].double()).abs().max()) for k in ("alphas", "weights", "depth", "rgb", "dino")}
    print(f"{what}: max |d| " + " ".join(f"{k} {v:.3g}" for k, v in d.items()) +
          f"; masks differ {int((t['invalid'] != p['invalid']).sum())} / {int((t['invalid_f'] != p['invalid_f']).sum())}")
    for k in ("invalid", "invalid_f"):
        assert torch.equal(t[k], p[k]), f"{what}: {k}"
    ren = lambda o: {"depth": o["depth"], "dino_features": o["dino"], "rgb": o["rgb"], "weights": o["weights"]}
    check_lowp(ren(t), {k: v.numpy() for k, v in ren(p).items()}, precision)
    assert d["alphas"] <= 2e-3, f"{what}: alphas {d['alphas']:.3g}"


def _assert_equal(a, b, rows, what):
    for k in KEYS:
        x, y = a[k][rows], b[k][rows]
        assert torch.equal(x, y), f"{what}{k}: {int((x != y).sum())} elements differ"


# ------------------------------------------------------------------ tile against per-ray route
@pytest.mark.gpu
@pytest.mark.usefixtures("hooks")
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("offset", [False, True], ids=["encoder_pose", "offset_pose"])
@pytest.mark.parametrize("K,D", [(64, 64), (64, 384), (32, 64), (128, 384)])
def test_tile_route_against_per_ray_route(K, D, offset, precision):
    """Every launched shape that shares the per-step routines -- K = 64 (late order, two rays
    per wave; D = 64: the head on waves 0..3 beside the box pass on waves 4..7; D = 384: every
    wave runs head tiles first), K = 32 and K = 128 (early order) -- at both render poses, with
    given depths and with depths drawn in the kernel, on 8 workgroups (several steps each) and
    on every CU (one step or none).  No group may go to the fallback: the tile kernel itself
    is compared."""
    from scenedino_amd import _lib
    net, rays = _net(K, D, precision, FRAME), _rays(offset, FRAME)
    R = rays.shape[0]
    assert R % GROUP[K] == 0 and R // GROUP[K] >= 24
    for slots in (8, _ncu()):
        _lib.reserve_cus(_ncu() - slots)
        for z, kw in ((_z(K, D, offset, FRAME), {}), (None, dict(z_seed=4321, z_offset=5))):
            what = f"K={K} D={D} {precision} slots={slots} {'given' if z is not None else 'drawn'} z"
            t, listed = _render(net, rays, z, K, "tile", slots=slots, **kw)
            assert not listed, f"{what}: rays {listed[:8]}.. went to the fallback"
            p, _ = _render(net, rays, z, K, "ray", **kw)
            _assert_contract(t, p, precision, what)
    _lib.reserve_cus(0)


# ------------------------------------------------------------------ boundary cases
@pytest.mark.gpu
@pytest.mark.usefixtures("hooks")
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("R", [5, 21, 16 * 29 + 5])
def test_partial_last_group(R, precision):
    """K = 64 with a ray count that is no multiple of the 16-ray group: the last group has 5
    rays (waves 0..4 one ray each, waves 5..7 none -- the packed box pass takes the endpoints
    of waves whose rays are past R, and of waves 0..3 whose partner has none); R = 5 and 21
    are frames of one and two groups on a grid of one workgroup per CU, where every other
    workgroup leaves at once.  Drawn and given depths."""
    K, D = 64, 64
    net, rays = _net(K, D, precision, FRAME), _rays(True, FRAME)[:R]
    for z, kw in ((_z(K, D, True, FRAME)[:R], {}), (None, dict(z_seed=77, z_offset=3))):
        what = f"R={R} {precision} {'given' if z is not None else 'drawn'} z"
        t, listed = _render(net, rays, z, K, "tile", **kw)
        assert not listed, f"{what}: rays {listed[:8]}.. went to the fallback"
        for k in KEYS:
            assert bool(torch.isfinite(t[k].double()).all()), f"{what}: {k} not finite"
        p, _ = _render(net, rays, z, K, "ray", **kw)
        _assert_contract(t, p, precision, what)


# ------------------------------------------------------------------ box pass packing
def _nofit_groups(x0, y0, group, cap_bytes, margin):
    """Groups whose whole box, halves and quarters all miss a tile buffer of cap_bytes, the
    boxes around every tap widened by `margin` texels on each side (0: the taps' own boxes,
    inside the kernel's; 1: past the box pass's border margin, around the kernel's)."""
    R, K = x0.shape
    G = R // group
    x = x0.reshape(G, 2, 8, 2, K // 2).transpose(0, 1, 3, 2, 4) if group == 16 else \
        x0.reshape(G, group, 4, K // 4).transpose(0, 2, 1, 3)
    y = y0.reshape(G, 2, 8, 2, K // 2).transpose(0, 1, 3, 2, 4) if group == 16 else \
        y0.reshape(G, group, 4, K // 4).transpose(0, 2, 1, 3)
    fits = []
    for n in (1, 2, 4):
        xs, ys = x.reshape(G * n, -1), y.reshape(G * n, -1)
        tw = xs.max(1) + 2 - xs.min(1) + 2 * margin
        th = ys.max(1) + 2 - ys.min(1) + 2 * margin
        fits.append(((th * tile_stats.pitch(tw)).reshape(G, n) <= cap_bytes // TEX).all(1))
    return ~fits[0] & ~fits[1] & ~fits[2]


@pytest.mark.gpu
@pytest.mark.usefixtures("hooks")
@pytest.mark.parametrize("K", [64, 32])
def test_capped_tiles_lists_and_output(K):
    """Tile buffers capped so that groups are staged whole, by halves, by quarters, or listed
    for the fallback (the boxes the packed box pass writes for both waves of a pair decide
    which).  List contents: whole groups; every group whose own tap boxes miss the buffer in
    quarters is listed, no group whose boxes fit with a texel of margin on each side is.
    Output: rays rendered from the tiles bit-equal to the uncapped render's, listed rays (the
    per-ray kernel's) within the contract of it, and the whole capped frame within the
    contract of the per-ray route."""
    D, GR = 64, GROUP[K]
    H, W, grid = FRAME_BIG
    net, rays, z = _net(K, D, "bf16", FRAME_BIG), _rays(True, FRAME_BIG), _z(K, D, True, FRAME_BIG)
    R = rays.shape[0]
    x0, y0 = tile_stats.taps(rays.cpu().numpy(), z.cpu().numpy(), np.array(KN, np.float32), grid[1], grid[0])
    caps = (24, 20, 16)
    shares = np.array([tile_stats.split_shares(x0, y0, GR, c * 1024) for c in caps])
    print(f"K={K} caps KiB {caps}: whole / halves / quarters / fallback {shares.round(3).tolist()}")
    assert shares[:, 1].max() > 0 and shares[:, 2].max() > 0 and shares[:, 3].max() > 0, \
        "the caps do not split groups by halves and quarters and overflow some"
    u, lu = _render(net, rays, z, K, "tile")
    assert not lu
    p, _ = _render(net, rays, z, K, "ray")
    for cap in caps:
        c, lc = _render(net, rays, z, K, "tile", cap=cap * 1024)
        flagged = torch.zeros(R, dtype=torch.bool)
        flagged[lc] = True
        fg = flagged.reshape(-1, GR)
        assert bool((fg.all(1) | ~fg.any(1)).all()), f"cap {cap} KiB: a group is listed in part"
        listed_g = fg.any(1).numpy()
        must, may = _nofit_groups(x0, y0, GR, cap * 1024, 0), _nofit_groups(x0, y0, GR, cap * 1024, 1)
        print(f"cap {cap} KiB: groups listed {int(listed_g.sum())}, boxes miss {int(must.sum())}, "
              f"miss with margin {int(may.sum())} of {listed_g.size}")
        assert not (must & ~listed_g).any(), f"cap {cap} KiB: a group that cannot be staged is not listed"
        assert not (listed_g & ~may).any(), f"cap {cap} KiB: a group that fits is listed"
        assert float(flagged.float().mean()) < 0.5, f"cap {cap} KiB: most rays went to the fallback"
        _assert_equal(u, c, ~flagged, f"cap {cap} KiB ")
        if flagged.any():
            _assert_contract(c, u, "bf16", f"K={K} cap {cap} KiB listed rays", rows=flagged)
        _assert_contract(c, p, "bf16", f"K={K} cap {cap} KiB against the per-ray route")


@pytest.mark.gpu
@pytest.mark.usefixtures("hooks")
def test_unsorted_depths_flag_the_group():
    """Depths not sorted along the ray (every 32-sample part of the rays of groups 1 and 4
    shuffled, test_tile_late.py's permutation): interior samples leave the boxes the packed
    box pass took from the part endpoints, the late ray pass flags those groups -- and only
    those -- and the frame still matches the per-ray route."""
    K, D, GR = 64, 64, 16
    rays = _rays(True, FRAME)
    R = rays.shape[0]
    z = _z(K, D, True, FRAME).clone()
    g = torch.Generator().manual_seed(7)
    shuffled = list(range(16, 32)) + list(range(64, 80))
    for r in shuffled:
        for q in range(K // 32):
            z[r, 32 * q: 32 * q + 32] = z[r, 32 * q: 32 * q + 32][torch.randperm(32, generator=g).to(DEV)]
    x0, y0 = tile_stats.taps(rays.cpu().numpy(), z.cpu().numpy(), np.array(KN, np.float32), FRAME[2][1], FRAME[2][0])
    assert tile_stats.endpoint_misses(x0, y0)[shuffled].any()
    net = _net(K, D, "bf16", FRAME)
    t, listed = _render(net, rays, z, K, "tile")
    assert listed, "no group was sent to the fallback: the verification did not run"
    groups = sorted({r // GR for r in listed})
    print(f"unsorted depths: groups listed {groups}")
    assert set(groups) <= {1, 4}, "a group with sorted depths was flagged"
    assert listed == [r for gi in groups for r in range(GR * gi, GR * gi + GR)]
    p, _ = _render(net, rays, z, K, "ray")
    _assert_contract(t, p, "bf16", "unsorted depths")


# ------------------------------------------------------------------ exactness on the CPU
def _f32_add(a16, b16):
    """v_add_f32 of the two v_cvt_f32_f16 results: numpy float32 addition (IEEE, RNE)."""
    return a16.astype(np.float32) + b16.astype(np.float32)


def _fma_mix(a16, b16):
    """v_fma_mix_f32 a, 1.0, b with f16 a, b: the real a * 1 + b rounded once to f32.  The sum
    of two f16 values (multiples of 2^-24 below 2^17) is exact in float64, so rounding that to
    float32 is the single rounding of the fused operation."""
    return (a16.astype(np.float64) * np.float64(1.0) + b16.astype(np.float64)).astype(np.float32)


def _same_bits(x, y):
    nan = np.isnan(x) & np.isnan(y)
    return bool(((x.view(np.uint32) == y.view(np.uint32)) | nan).all())


def test_f16_pair_sum_forms_bit_equal():
    """Level 1 of the ray sums' butterfly adds two f16 partial sums in f32: before, v_add_f32 of
    two converted values; now one v_fma_mix_f32 (own * 1.0 + rot).  Every f16 bit pattern
    against the range ends (zeros, smallest and largest denormal, smallest normal, 65504,
    infinities, both signs), and 2^20 random pairs of bit patterns: the same f32 bits (NaN for
    NaN), in either operand order."""
    every = np.arange(65536, dtype=np.uint16).view(np.float16)
    ends = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x0400, 0x8400, 0x3c00, 0xbc00,
                     0x7bff, 0xfbff, 0x7c00, 0xfc00, 0x7e00], dtype=np.uint16).view(np.float16)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in ends:
            b = np.full_like(every, e)
            assert _same_bits(_f32_add(every, b), _fma_mix(every, b))
            assert _same_bits(_f32_add(every, b), _fma_mix(b, every))
        rng = np.random.default_rng(11)
        a = rng.integers(0, 65536, 1 << 20).astype(np.uint16).view(np.float16)
        b = rng.integers(0, 65536, 1 << 20).astype(np.uint16).view(np.float16)
        assert _same_bits(_f32_add(a, b), _fma_mix(a, b))
        assert _same_bits(_f32_add(a, b), _fma_mix(b, a))
        # one rounding, not none: a pair whose sum needs more than 24 bits
        big, tiny = np.array([65504.0], np.float16), np.array([2.0 ** -24], np.float16)
        assert _fma_mix(big, tiny)[0] == np.float32(65504.0) and _same_bits(_f32_add(big, tiny), _fma_mix(big, tiny))


def test_butterfly_level1_index_maps():
    """ray_sums, level 1, on one 16-lane row.  Before: hacc[t][r] = half (r & 1) of pair
    hacc16[4 s2 + q], t = 2 s2 + (q >> 1), r = 2 (q & 1) + half, converted to f32, then
    u[i] = x + x(lane - 8) with x = hacc[i >> 2][i & 3] on banks 0, 1 (lanes 0..7) and
    hacc[(i + 16) >> 2][i & 3] on banks 2, 3.  Now: per s2 < 2, q: own = pair a = [4 s2 + q] on
    banks 0, 1, pair b = [4 (s2 + 2) + q] on banks 2, 3; rot = the same pair of lane - 8;
    u[4 (2 s2 + (q >> 1)) + 2 (q & 1) + half] = own.half * 1 + rot.half.  Same bits for every
    u[i] and lane."""
    rng = np.random.default_rng(5)
    h16 = rng.standard_normal((16, 16, 2)).astype(np.float16)  # [pair index][lane][half]
    lanes = np.arange(16)
    low = lanes < 8           # banks 0, 1
    src = (lanes + 8) % 16    # row_ror:8 (= lane - 8 in a 16-lane row)
    hacc = np.zeros((8, 4, 16), np.float32)
    for s2 in range(4):
        for q in range(4):
            t, r = 2 * s2 + (q >> 1), 2 * (q & 1)
            hacc[t][r] = h16[4 * s2 + q, :, 0].astype(np.float32)
            hacc[t][r + 1] = h16[4 * s2 + q, :, 1].astype(np.float32)
    old = np.zeros((16, 16), np.float32)
    for i in range(16):
        a, b = hacc[i >> 2][i & 3], hacc[(i + 16) >> 2][i & 3]
        old[i] = np.where(low, a[src] + a, b[src] + b)
    new = np.zeros((16, 16), np.float32)
    for s2 in range(2):
        for q in range(4):
            pa, pb = h16[4 * s2 + q], h16[4 * (s2 + 2) + q]
            own = np.where(low[:, None], pa, pb)
            rot = np.where(low[:, None], pa[src], pb[src])
            i = 4 * (2 * s2 + (q >> 1)) + 2 * (q & 1)
            new[i] = _fma_mix(own[:, 0], rot[:, 0])
            new[i + 1] = _fma_mix(own[:, 1], rot[:, 1])
    assert _same_bits(old, new)


def test_packed_box_pass_lane_map():
    """The box pass writes, per wave w and part q < 4, the words (min, max) of the part's two
    endpoint records 32 q and 32 q + 31 at byte 32 w + 8 q of the slot's box area.  Before:
    wave w, lane e < 8 = endpoint (q = e >> 1, end = e & 1), lane 0 stores the wave's 32 B.
    Packed: wave w >= 4, lane l < 16 takes wave w - 4 + 4 (l >> 3), endpoint l & 7; even lanes
    store their part's 8 B.  The same (wave, part, record pair) at the same byte, every byte
    of the area once."""
    NW = 8
    before = {}
    for w in range(NW):
        for q in range(4):
            before[32 * w + 8 * q] = (w, (32 * q, 32 * q + 31))
    packed = {}
    for w in range(NW // 2, NW):
        recs = {}
        for l in range(16):
            e = l & 7
            tw = w - NW // 2 + (NW // 2) * ((l >> 3) & 1)
            recs[l] = (tw, 32 * (e >> 1) + (31 if e & 1 else 0))
        for l in range(0, 16, 2):  # the pair (l, l ^ 1) is reduced by quad_perm [1, 0, 3, 2]
            (tw, r0), (tw1, r1) = recs[l], recs[l ^ 1]
            assert tw == tw1
            off = 32 * tw + 8 * ((l & 7) >> 1)
            assert off not in packed
            packed[off] = (tw, (r0, r1))
    assert packed == before
    assert sorted(packed) == list(range(0, 32 * NW, 8))
