#!/usr/bin/env python3
"""Diagnostic: the dense CRF of scenedino_amd/downstream_head/crf.py, the native route
(sd_dense_crf) against the same module's torch route (float64, exact sums), both on the GPU, on one
192 x 640 frame at the reference's constants (10 iterations):

  r1_c19   one result of 19 classes (19 columns: two 16-wide column tiles);
  r4_c19   the head's four results of 19 classes in one call (76 columns: five column tiles); the
           torch route takes the four as the columns of one inference too.

The scene is tests/_crf_oracle.py's generator at that size (bands of palette colours with noise,
15 % of the labels replaced).  HIP events around back-to-back calls after a warm-up call, RUNS runs
of each route, alternated in one process; every run is reported with the median and the spread
max - min.  The native route is timed over ITERS calls per run, the torch route over one.
``native_ms_per_iteration`` is (t(10 iterations) - t(1 iteration)) / 9 of the native medians: one
k_crf_sweep launch for all results.  ``faster_than`` is True where the torch median
exceeds native's by more than the two spreads together.  This is eager time on a shared host, not
kernel time.  Writes profiles/dense_crf/bench.json and prints it as one JSON line."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from scenedino_amd import _lib  # noqa: E402
from scenedino_amd.downstream_head import crf  # noqa: E402
from stego_train_bench import RUNS, timed  # noqa: E402
import _crf_oracle as O  # noqa: E402

dev = "cuda"
H_, W_, C_ = 192, 640, 19
ITERS = 5


def _stats(ts):
    return {"runs": [round(t, 4) for t in ts], "median": round(statistics.median(ts), 4),
            "spread": round(max(ts) - min(ts), 4)}


def _run(img, unaries, native, **params):
    was, crf._NATIVE = crf._NATIVE, native
    try:
        out = crf.crf_inference(img, unaries, **params)
    finally:
        crf._NATIVE = was
    assert crf.last_route == ("native" if native else "torch")
    return out


def _row(img, unaries):
    variants = (("native", lambda: _run(img, unaries, True), ITERS),
                ("torch", lambda: _run(img, unaries, False), 1))
    for _, f, _ in variants:
        f()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in variants}
    for _ in range(RUNS):
        for name, f, iters in variants:
            times[name].append(timed(f, iters))
    one = [timed(lambda: _run(img, unaries, True, iters=1), ITERS) for _ in range(RUNS)]
    out = {name: _stats(ts) for name, ts in times.items()}
    out["native_1_iteration"] = _stats(one)
    n, t = out["native"], out["torch"]
    out["native_ms_per_iteration"] = round((n["median"] - out["native_1_iteration"]["median"]) / 9, 4)
    out["faster_than"] = {"torch": bool(t["median"] - n["median"] > n["spread"] + t["spread"])}
    a, b = _run(img, unaries, True)[0], _run(img, unaries, False)[0]
    out["labels_differing_between_routes"] = int((a != b).sum())
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("crf_bench: needs a ROCm device")
    _lib.load()
    image, labels = O.make_fixture(H_, W_, C_)
    img = torch.from_numpy(image).to(dev)
    g = torch.Generator().manual_seed(0)
    maps = [torch.from_numpy(labels).reshape(-1)]
    for _ in range(3):  # three more label maps of the same scene: other pixels replaced
        m = maps[0].clone()
        flip = torch.rand(m.shape, generator=g) < 0.15
        m[flip] = torch.randint(0, C_, (int(flip.sum()),), generator=g)
        maps.append(m)
    unaries = [crf.unary_from_labels(m.to(dev), C_) for m in maps]
    out = {"iters": ITERS, "runs": RUNS, "unit": "ms per call", "shape": [H_, W_], "classes": C_,
           "crf_iterations": crf.MAX_ITER}
    out["r1_c19"] = _row(img, unaries[:1])
    out["r4_c19"] = _row(img, unaries)

    path = os.path.join(ROOT, "profiles", "dense_crf")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
