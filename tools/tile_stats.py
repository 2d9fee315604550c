"""Tap-box statistics of the tile render kernel (k_render_tile, sdhip_tile.hip) for the
C2 bench frame: per ray group, the staged texel count th * pitch(tw) of the union of its
bilinear tap boxes, the share of groups that fit a given tile buffer whole, by halves or by
quarters (the kernel's split staging), and -- for the late step order -- the share of
32-sample parts whose taps leave the box spanned by the part's two endpoint samples.
CPU only; the depths use numpy's RNG in place of the kernel's counter RNG, so the shares are
estimates of the kernel's.

usage: tile_stats.py [--group 8|16] [--caps KIB,KIB,...]
  --group 8   8-ray groups, one ray per wave: halves / quarters = 32 / 16 samples of every ray
  --group 16  16-ray groups, two rays per wave: halves = the group's first / last 8 rays,
              quarters = their 32-sample half boxes

The functions are importable (tests/test_tile_late.py checks its unsorted depths with them)."""
import argparse
import sys

import numpy as np

TEX = 288  # LDS bytes per staged texel (ST_TEX)


def pitch(tw):
    r = tw & 7
    return tw + np.where(r == 7, 3, np.where(r == 0, 2, np.where(r == 1, 1, 0)))


def taps(rays, z, Kn, Wf, Hf, frac=False):
    """(x0, y0) of the north-west bilinear tap of every sample (sd_taps on the encoder view's
    normalised projection; the encoder camera is the world frame).  rays (R, >= 6), z (R, K).
    frac: also the fractional positions (ix - x0, iy - y0)."""
    p = rays[:, None, :3] + z[..., None] * rays[:, None, 3:6]
    i = p @ np.asarray(Kn, np.float32).T
    zd = np.maximum(i[..., 2], 1e-3)
    x = np.clip(i[..., 0] / zd, -2, 2)
    y = np.clip(i[..., 1] / zd, -2, 2)
    ix = np.clip(((x + 1) * Wf - 1) / 2, 0, Wf - 1)
    iy = np.clip(((y + 1) * Hf - 1) / 2, 0, Hf - 1)
    x0, y0 = np.floor(ix).astype(np.int32), np.floor(iy).astype(np.int32)
    if frac:
        return x0, y0, ix - x0, iy - y0
    return x0, y0


def groups_flagged(x0, y0, fx, fy, group, eps=1.0 / 1024, part=32):
    """Per group: True where the late order's verification would flag it when staged whole --
    a sample's tap outside the union of the group's part-endpoint boxes (box pass: the first
    and last sample of every `part` samples of every ray, an endpoint within eps texels of a
    texel border also claiming the texel across it)."""
    R, K = x0.shape
    G = R // group
    out = np.zeros(G, bool)
    for v, f in ((x0, fx), (y0, fy)):
        v = v[:G * group].reshape(G, group, K // part, part)
        f = f[:G * group].reshape(G, group, K // part, part)
        ends = v[..., [0, -1]]
        fe = f[..., [0, -1]]
        lo = (ends - (fe < eps)).reshape(G, -1).min(1)
        hi = (ends + (fe > 1 - eps)).reshape(G, -1).max(1)
        vv = v.reshape(G, -1)
        out |= ((vv < lo[:, None]) | (vv > hi[:, None])).any(1)
    return out


def box_texels(x0, y0):
    """Staged texels th * pitch(tw) of the box around all taps of each row of x0 / y0."""
    tw = x0.max(1) + 2 - x0.min(1)
    th = y0.max(1) + 2 - y0.min(1)
    return th * pitch(tw)


def group_parts(x0, y0, group):
    """Texel counts (G, 1), (G, 2), (G, 4) of every group's whole box, halves and quarters, as
    the kernel partitions them (module docstring).  Rays past a multiple of `group` are dropped."""
    R, K = x0.shape
    G = R // group
    x = x0[:G * group].reshape(G, group, K)
    y = y0[:G * group].reshape(G, group, K)
    if group == 16:  # parts: (ray set, sample half)
        x = x.reshape(G, 2, 8, 2, K // 2).transpose(0, 1, 3, 2, 4)
        y = y.reshape(G, 2, 8, 2, K // 2).transpose(0, 1, 3, 2, 4)
    else:  # parts: sample quarters
        x = x.reshape(G, group, 4, K // 4).transpose(0, 2, 1, 3)
        y = y.reshape(G, group, 4, K // 4).transpose(0, 2, 1, 3)
    out = []
    for n in (1, 2, 4):
        out.append(box_texels(x.reshape(G * n, -1), y.reshape(G * n, -1)).reshape(G, n))
    return out


def split_shares(x0, y0, group, cap_bytes):
    """Shares of groups staged whole, by halves, by quarters, and sent to the fallback."""
    cap = cap_bytes // TEX
    fit = [(n <= cap).all(1) for n in group_parts(x0, y0, group)]
    whole = fit[0]
    halves = ~whole & fit[1]
    quarters = ~whole & ~fit[1] & fit[2]
    return whole.mean(), halves.mean(), quarters.mean(), (~whole & ~halves & ~quarters).mean()


def endpoint_misses(x0, y0, part=32):
    """Per (ray, part of `part` consecutive samples): True where a sample's tap lies outside
    the box spanned by the part's first and last sample (the late order's box pass)."""
    R, K = x0.shape
    x = x0.reshape(R, K // part, part)
    y = y0.reshape(R, K // part, part)
    out = np.zeros(x.shape[:2], bool)
    for v in (x, y):
        lo = np.minimum(v[..., 0], v[..., -1])[..., None]
        hi = np.maximum(v[..., 0], v[..., -1])[..., None]
        out |= ((v < lo) | (v > hi)).any(-1)
    return out


def bench_taps(offset):
    import torch
    sys.path.insert(0, ".")
    import bench
    from oracle import render_oracle as O
    pose = torch.eye(4)
    rp = bench.offset_render_pose(pose) if offset else pose
    K = torch.tensor(bench.KITTI_K)
    rays = O.gen_rays(rp.view(1, 4, 4), K.view(1, 3, 3), bench.H, bench.W).numpy()
    Ks = bench.K_SAMPLES
    g = np.random.default_rng(0)
    t = np.linspace(0, 1 - 1 / Ks, Ks, dtype=np.float32)[None] + g.random((len(rays), Ks), dtype=np.float32) / Ks
    near, far = rays[:, 6:7], rays[:, 7:8]
    z = 1 / ((1 / near) * (1 - t) + (1 / far) * t)
    return taps(rays, z, K.numpy(), bench.WF, bench.HF, frac=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", type=int, default=8, choices=[8, 16])
    ap.add_argument("--caps", default="37,45,51,57,67", help="tile buffer sizes in KiB")
    a = ap.parse_args()
    for off in (False, True):
        x0, y0, fx, fy = bench_taps(off)
        n = group_parts(x0, y0, a.group)[0][:, 0]
        print("offset" if off else "identity", f"{a.group}-ray groups: texels p50/p90/p99/max",
              np.percentile(n, [50, 90, 99]).astype(int), n.max(),
              f" endpoint-box misses: {endpoint_misses(x0, y0).any(1).mean() * 100:.4f}% of rays,"
              f" groups flagged: {groups_flagged(x0, y0, fx, fy, a.group).mean() * 100:.4f}%"
              f" (no border margin: {groups_flagged(x0, y0, fx, fy, a.group, eps=0).mean() * 100:.4f}%)")
        for c in (int(v) for v in a.caps.split(",")):
            w, h, q, o = split_shares(x0, y0, a.group, c * 1024)
            print(f"  {c:3d} KiB: not whole {100 * (1 - w):5.1f}%  (halves {100 * h:5.1f}%, quarters "
                  f"{100 * q:5.1f}%, fallback {100 * o:5.1f}%)")


if __name__ == "__main__":
    main()
