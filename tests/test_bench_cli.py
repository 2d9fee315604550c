"""bench.py's command line: --dump-outputs (the last timed step's arrays as .npy, sampled to a
fixed size, the same from run to run) and what a plain run leaves to --full.

CPU: the sampling / writing helpers.  GPU: one short plain run of the C2 benchmark in a
process of its own (that is what the test is about)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_sample_outputs_fixed_sample_and_dtypes():
    import bench
    n = bench.DUMP_MAX_ELEMS
    big = torch.arange(3 * n, dtype=torch.float32).reshape(3, n)
    arrays = {"big": big, "half": torch.ones(2, 3, dtype=torch.bfloat16),
              "mask": torch.tensor([True, False]), "f64": torch.ones(4, dtype=torch.float64),
              "none": None}
    state = torch.get_rng_state()
    a = bench.sample_outputs(arrays, "p_")
    assert torch.equal(torch.get_rng_state(), state)  # the global generator is not advanced
    b = bench.sample_outputs(arrays, "p_")
    assert sorted(a) == ["p_big", "p_f64", "p_half", "p_mask"]
    assert a["p_big"].shape == (n,) and a["p_big"].dtype == np.float32
    assert np.array_equal(a["p_big"], b["p_big"])  # the same elements in every call
    assert len(np.unique(a["p_big"])) > n // 2 and a["p_big"].max() > 2 * n  # spread over the array
    assert a["p_half"].shape == (2, 3) and a["p_half"].dtype == np.float32
    assert a["p_mask"].dtype == np.float32 and a["p_mask"].tolist() == [1.0, 0.0]
    assert a["p_f64"].dtype == np.float64


def test_named_tensors_and_dump(tmp_path):
    import bench
    t = [torch.zeros(1), (torch.ones(2), {"x": torch.full((3,), 2.0)})]
    named = bench.named_tensors(t, "m")
    assert list(named) == ["m_0", "m_1_0", "m_1_1_x"]
    d = tmp_path / "out" / "dir"
    bench.dump_outputs(str(d), bench.sample_outputs(named))
    assert sorted(os.listdir(d)) == ["m_0.npy", "m_1_0.npy", "m_1_1_x.npy"]
    assert np.load(d / "m_1_1_x.npy").tolist() == [2.0, 2.0, 2.0]
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(d), {"a": np.zeros(bench.DUMP_MAX_BYTES // 8 + 1, np.float64)})


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """A plain C2 run: --steps sets the timed steps, the line holds ms_per_step and none of
    the fields --full adds, and --dump-outputs writes both poses' maps (finite, float32,
    under 64 MB, depth and weights inside their ranges)."""
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "rays/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 192 * 640 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    for k in ("cpu_baseline", "end_to_end", "fp16_default", "no_gather"):
        assert k not in line
    files = sorted(os.listdir(d))
    total = 0
    for pose in ("identity", "offset"):
        for k in ("depth", "rgb", "dino_features", "weights", "alphas"):
            assert f"{pose}_{k}.npy" in files
    for f in files:
        a = np.load(d / f)
        total += a.nbytes
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
    assert total <= 64 * 10**6
    for pose in ("identity", "offset"):
        depth = np.load(d / f"{pose}_depth.npy")
        assert depth.shape == (1, 192 * 640)
        # depth = sum_k w_k z_k with w >= 0, sum w <= 1 and z <= z_far
        assert depth.min() >= 0.0 and depth.max() <= 80.0 + 1e-3 and depth.max() > 0.0
        w = np.load(d / f"{pose}_weights.npy")
        assert w.min() >= 0.0 and w.max() <= 1.0 and w.max() > 0.0
