"""The downstream stage's 3-D surface crops, MI355X build.

``sample_3d_crop`` mirrors ``BTSDownstreamWrapper.sample_3d_crop``
(scenedino/training/trainer_downstream.py:216-292): per frame, ``n_crops`` depth-quantile bins of
view 0's depth map (the depths below ``z_far``), one random pixel per bin, its back-projected
point as the crop centre, ``oversampling * n_samples`` points in a ball around it, the field's
sigma and DINO codes there; a crop is kept when more than ``n_samples`` of its points have
``sigma > sigma_threshold``, and contributes its first ``n_samples`` such rows, expanded to the
full DINO width, with ``1 - exp(-sigma)`` beside them.  In ``downstream.mode: "3d"`` these are
the rows the STEGO correlation loss reads.

On the GPU the route is ``sd_crop3d_centres`` (limits, counts, pixel picks, centres and points of
every frame in one launch) -> ``net.query`` -> ``sd_crop3d_compact`` -> ``expand_dim`` on the
padded rows, with one host read (``n_valid``) where the reference has roughly ninety per batch-4
step.  CPU tensors, ``_NATIVE = False`` and ``n_crops`` > 8 run the same arithmetic in torch ops.

Random numbers: the pixel picks and the ball offsets are drawn on the device with torch's RNG
(``rand`` for the picks; ``randn`` normalised times ``sample_radius * rand ** (1 / 3)`` for the
offsets), one call each for the whole batch.  The stream is therefore torch's, not the reference's
sequence of ``randint`` / ``randn`` / ``rand`` calls; ``draws`` supplies both instead (tests).

Where this differs from the reference on purpose: frames are independent, and an empty bin (for
instance the last one once more than a fifth of a frame sits on one far depth) invalidates that
crop only.  That equals the reference for n = 1, which skips the bin, and for any n without an
empty bin.  It differs exactly where the reference's ``n_crops = len(sampled_positions)`` rebinds
the loop bound for the following frames or makes its ``torch.stack`` fail.  A frame without any
depth below ``z_far``, where the reference raises inside ``torch.quantile``, loses its crops.
"""
from __future__ import annotations

import torch

from .. import _lib

_NATIVE = True
MAX_NATIVE_CROPS = 8


def _draw(n, n_crops, S, sample_radius, device, draws):
    """(pick (n, n_crops) in [0, 1), shift (n, n_crops, S, 3)) from ``draws`` or torch's RNG."""
    pick = draws.get("pick") if draws else None
    shift = draws.get("shift") if draws else None
    if pick is None:
        pick = torch.rand(n, n_crops, device=device)
    if shift is None:
        v = torch.randn(n, n_crops, S, 3, device=device)
        v = v / torch.norm(v, dim=-1, keepdim=True)
        shift = v * (sample_radius * torch.rand(n, n_crops, S, 1, device=device) ** (1 / 3))
    pick = pick.to(device=device, dtype=torch.float32).contiguous()
    shift = shift.to(device=device, dtype=torch.float32).contiguous()
    if tuple(pick.shape) != (n, n_crops) or tuple(shift.shape) != (n, n_crops, S, 3):
        raise ValueError(f"draws: pick must be ({n}, {n_crops}) and shift ({n}, {n_crops}, {S}, 3)")
    return pick, shift


def quantile_limits(depth0, z_far, n_crops):
    """depth0 (n, h, w) -> (limits (n, n_crops + 1), m (n)): torch.quantile of each frame's
    depths below z_far at i / n_crops (linear), without a host read; NaN where m = 0."""
    n = depth0.shape[0]
    flat = depth0.reshape(n, -1)
    sel = flat < z_far
    m = sel.sum(1)
    srt = torch.sort(torch.where(sel, flat, torch.full_like(flat, float("inf"))), dim=1).values
    q = (torch.arange(n_crops + 1, dtype=torch.float64) / n_crops).to(
        device=flat.device, dtype=torch.float32)
    rank = q[None] * (m - 1).clamp_min(0).to(torch.float32)[:, None]
    lo, hi = rank.floor(), rank.ceil()
    a, b = srt.gather(1, lo.long()), srt.gather(1, hi.long())
    lim = torch.maximum(torch.minimum(torch.lerp(a, b, rank - lo), b), a)
    return torch.where((m > 0)[:, None], lim, torch.full_like(lim, float("nan"))), m


def centres_torch(depth, poses, projs, z_far, pick, shift, limits=None):
    """sd_crop3d_centres in torch ops (the same outputs); ``limits`` overrides the quantiles."""
    n, _, h, w = depth.shape
    n_crops = pick.shape[1]
    dev = depth.device
    depth0 = depth[:, 0].float()
    flat = depth0.reshape(n, 1, h * w)
    if limits is None:
        limits, _ = quantile_limits(depth0, z_far, n_crops)
    inb = (flat > limits[:, :-1, None]) & (flat < limits[:, 1:, None])  # (n, n_crops, h w)
    cum = inb.cumsum(-1, dtype=torch.int32)
    count = cum[..., -1]
    ok = count > 0
    r = torch.minimum((pick * count.float()).to(torch.int32), count - 1).clamp_min(0)
    p = torch.searchsorted(cum, (r + 1)[..., None]).squeeze(-1).clamp_max(h * w - 1)
    row, col = p // w, p % w
    # the pixel's unit ray, in the operation order of util.unproj_map / gen_rays (sd_gen_rays)
    xi = torch.linspace(-1 + .5 * (2 / w), 1 - .5 * (2 / w), w, dtype=torch.float32, device=dev)[col]
    yi = torch.linspace(-1 + .5 * (2 / h), 1 - .5 * (2 / h), h, dtype=torch.float32, device=dev)[row]
    K, P = projs[:, 0].float(), poses[:, 0].float()
    ux = (xi - K[:, 0, 2, None]) / K[:, 0, 0, None]
    uy = (yi - K[:, 1, 2, None]) / K[:, 1, 1, None]
    u = torch.stack((ux, uy, torch.ones_like(ux)), -1)
    u = u / torch.norm(u, dim=-1).unsqueeze(-1)
    ray = torch.stack([(P[:, i, 0, None] * u[..., 0] + P[:, i, 1, None] * u[..., 1])
                       + P[:, i, 2, None] * u[..., 2] for i in range(3)], -1)
    dd = flat[:, 0].gather(1, p)
    centre = P[:, None, :3, 3] + ray * dd[..., None]
    centre = torch.where(ok[..., None], centre, torch.zeros_like(centre))
    points = torch.where(ok[..., None, None], centre[:, :, None] + shift, torch.zeros_like(shift))
    pixel = torch.where(ok[..., None], torch.stack((row, col), -1), torch.full_like(row, -1)[..., None])
    return limits, count, pixel.to(torch.int32), centre, points


def compact_torch(sigma, codes, crop_ok, thr, n_samples):
    """sd_crop3d_compact in torch ops (the same outputs), without a host read."""
    C, S, D = codes.shape
    occ = sigma > thr
    cum = occ.cumsum(1, dtype=torch.int32)
    kept = (crop_ok > 0) & (cum[:, -1] > n_samples)
    kc = kept.cumsum(0, dtype=torch.int32)
    slot = torch.where(kept, kc - 1, torch.full_like(kc, -1))
    n_valid = kc[-1:].clone()
    want = torch.arange(1, n_samples + 1, device=sigma.device, dtype=torch.int32).expand(C, -1)
    idx = torch.searchsorted(cum, want.contiguous()).clamp_max(S - 1)  # j-th occupied row
    rows = codes.gather(1, idx[..., None].expand(-1, -1, D))
    occ_rows = 1 - torch.exp(-sigma.gather(1, idx))
    dest = torch.where(kept, slot, torch.full_like(slot, C)).long()  # dropped crops: a spare row
    codes_out = codes.new_zeros(C + 1, n_samples, D).index_copy_(0, dest, rows)[:C]
    occ_out = sigma.new_zeros(C + 1, n_samples).index_copy_(0, dest, occ_rows)[:C]
    return codes_out.contiguous(), occ_out.contiguous(), n_valid, slot


def _field(net, points):
    """sigma (n, P) and DINO codes (n, P, D) of the field at points (n, P, 3).  This package's
    BTSNet answers through ``query`` without the colour gather (sigma and the codes are
    bit-equal without it); any other net through its forward, as the reference calls it."""
    if hasattr(net, "query"):
        sigma, dino = net.query(points, colors=False)[:2]
        return sigma, dino
    _, _, sigma, _, state = net(points)
    return sigma.squeeze(-1), state["dino_features"]


def _sample_3d_crop_padded(net, poses, projs, depth, z_far=100, n_crops=5, n_samples=576,
                           sample_radius=0.5, sigma_threshold=0.5, oversampling=4, draws=None):
    """sample_3d_crop without its host read: (dino (C, n_samples, d_full), occupancy
    (C, n_samples), n_valid (1) i32 on the device, aux) with C = n n_crops; the first n_valid
    crops are the kept ones, in order.  aux: the intermediate tensors (tests)."""
    n = projs.size(0)
    S = oversampling * n_samples
    dev = depth.device
    pick, shift = _draw(n, n_crops, S, sample_radius, dev, draws)
    depth = depth.float().contiguous()
    native = _NATIVE and depth.is_cuda and n_crops <= MAX_NATIVE_CROPS
    with torch.no_grad():
        if native:
            limits, count, pixel, centre, points = _lib.crop3d_centres(
                depth, poses.float().contiguous(), projs.float().contiguous(), z_far, pick, shift)
        else:
            limits, count, pixel, centre, points = centres_torch(depth, poses, projs, z_far, pick,
                                                                 shift)
        sigma, codes = _field(net, points.view(n, n_crops * S, 3))
        sigma = sigma.reshape(n * n_crops, S).float().contiguous()
        codes = codes.reshape(n * n_crops, S, -1).contiguous()
        crop_ok = count.reshape(-1).to(torch.int32)
        if native and n * n_crops <= 64:
            codes_out, occ, n_valid, slot = _lib.crop3d_compact(sigma, codes, crop_ok,
                                                                sigma_threshold, n_samples)
        else:
            codes_out, occ, n_valid, slot = compact_torch(sigma, codes, crop_ok, sigma_threshold,
                                                          n_samples)
        # expand every padded row: cheaper than a second host read to learn how many are kept
        dino = net.encoder.expand_dim(codes_out)
    aux = {"limits": limits, "count": count, "pixel": pixel, "centre": centre, "points": points,
           "sigma": sigma, "codes": codes, "codes_out": codes_out, "slot": slot}
    return dino, occ, n_valid, aux


def sample_3d_crop(net, poses, projs, depth, z_far=100, n_crops=5, n_samples=576,
                   sample_radius=0.5, sigma_threshold=0.5, oversampling=4, draws=None):
    """BTSDownstreamWrapper.sample_3d_crop (trainer_downstream.py:216-292) on ``net``:
    poses (n, V, 4, 4) c2w, projs (n, V, 3, 3), depth (n, V, h, w) (view 0 of each is read) ->
    (dino (1, n_valid, n_samples, d_full), occupancy (1, n_valid, n_samples, 1)), or
    (None, None) when no crop survives.  ``draws``: {"pick": (n, n_crops) in [0, 1), "shift":
    (n, n_crops, oversampling n_samples, 3)} instead of torch's RNG (the module docstring: the
    default stream is torch's, not the reference's sequence of calls)."""
    dino, occ, n_valid, _ = _sample_3d_crop_padded(net, poses, projs, depth, z_far, n_crops,
                                                   n_samples, sample_radius, sigma_threshold,
                                                   oversampling, draws)
    k = int(n_valid.item())  # the one host read
    if k == 0:
        return None, None
    return dino[:k].unsqueeze(0), occ[:k].unsqueeze(0).unsqueeze(-1)
