#!/usr/bin/env python3
"""Diagnostic: the supersampled SSCBench voxel query (scenedino_amd/sscbench.py::query_voxels at
factor 1, 2 and 4: VOXEL_SIZE 0.2, 0.1, 0.05) on the synthetic encoded frame of
``bench.py --config c5`` (ViT-B/8-shaped 256 x 384 x 1280 grid, 256 x 256 x 32 scored voxels).

  native   the chunked driver as shipped: sd_field_query + sd_seg_query per chunk of coarse
           x-planes, sd_ssc_pool, sd_grow3;
  torch    the same driver and the same native per-point query with the pooling's torch route on
           the device instead of sd_ssc_pool (sscbench.pool_voxels(native=False): the reference's
           lines 727-745 -- per-class avg_pool3d of the alpha votes, argmax, max_pool3d).  At
           factor 1 nothing is pooled and only the native route exists.

HIP events around whole frames after a warm-up frame, RUNS runs of each route, alternated in one
process; every run is reported with the median and the spread max - min.  ``pool_kernel`` is
sd_ssc_pool alone on the frame's whole fine grid (ms, and GB/s against the 5 bytes per fine voxel
it must read), ``pool_share`` that time over the native frame's median.  ``peak_bytes`` is each
route's peak allocated memory above what is resident before the frame (the points included in
neither).  ``native_not_slower_in_any_run`` compares the alternated runs pairwise.  This is eager
time on a shared host, not kernel time.  Writes profiles/ssc_supersample/bench.json and prints it
as one JSON line."""
import functools
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from scenedino_amd import _lib, sscbench  # noqa: E402
from stego_train_bench import RUNS, timed  # noqa: E402

dev = "cuda"
FRAMES = {1: 10, 2: 3, 4: 1}  # frames per timed run


def _stats(ts):
    return {"runs": [round(t, 4) for t in ts], "median": round(statistics.median(ts), 4),
            "spread": round(max(ts) - min(ts), 4)}


def _peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def _row(net, dims, f):
    pts = sscbench.generate_point_grid(sscbench.read_calib()["Tr"], voxel_size=0.2 / f, device=dev)
    torch_pool = functools.partial(sscbench.pool_voxels, native=False)

    def frame(pool_fn=None):
        net._grid_cache = None  # a new frame: the grid is packed again, as in bench.py
        return sscbench.query_voxels(net, pts, dims, factor=f, pool_fn=pool_fn)
    routes = [("native", frame)] + ([("torch", lambda: frame(torch_pool))] if f > 1 else [])
    out = {"fine_voxels": int(pts.shape[0]), "frames_per_run": FRAMES[f]}
    res = {}
    for name, fn in routes:
        res[name] = fn()  # warm-up
    torch.cuda.synchronize()
    times = {name: [] for name, _ in routes}
    for _ in range(RUNS):
        for name, fn in routes:
            times[name].append(timed(fn, FRAMES[f]))
    for name, fn in routes:
        out[name] = _stats(times[name])
        out[name]["peak_bytes"] = _peak(fn)
    if f > 1:
        out["native_not_slower_in_any_run"] = all(n <= t for n, t in zip(times["native"], times["torch"]))
        out["labels_differing_between_routes"] = int((res["native"][1] != res["torch"][1]).sum())
        out["sigmas_bit_equal_between_routes"] = bool(torch.equal(
            res["native"][0].view(torch.int32), res["torch"][0].view(torch.int32)))
        # the pool kernel alone, on the whole fine grid of the frame
        fine = tuple(f * d for d in dims)
        g = torch.Generator(device=dev).manual_seed(0)
        sig = torch.nn.functional.softplus(2 * torch.randn(fine, device=dev, generator=g))
        sig *= torch.rand(fine, device=dev, generator=g) >= 0.3
        lab = torch.randint(0, 19, fine, device=dev, generator=g, dtype=torch.uint8)
        call = lambda: _lib.ssc_pool(sig, lab, f, 0.2 / f, 19)
        call()
        ks = [timed(call, 20) for _ in range(RUNS)]
        out["pool_kernel"] = _stats(ks)
        out["pool_kernel"]["GB_per_s"] = round(5 * sig.numel() / (out["pool_kernel"]["median"] * 1e-3) / 1e9, 1)
        out["pool_share"] = round(out["pool_kernel"]["median"] / out["native"]["median"], 4)
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("ssc_supersample_bench: needs a ROCm device")
    _lib.load()
    net, _, dims = bench.c5_scene(torch.device(dev), "bf16", 0)
    out = {"runs": RUNS, "unit": "ms per frame", "coarse_dims": list(dims),
           "max_points": sscbench.MAX_POINTS, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        for f in (1, 2, 4):
            out[f"factor_{f}"] = _row(net, dims, f)
            torch.cuda.empty_cache()
    path = os.path.join(ROOT, "profiles", "ssc_supersample")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "bench.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
