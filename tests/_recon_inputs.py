"""Seeded inputs and configurations of the ReconstructionLoss tests; tests/golden/
make_golden_recon.py imports the same generators, so tests/golden/recon_loss.npz holds results
only.  Tensors are drawn in float32 (the GPU tests feed them as they are, the oracles upcast the
same values)."""
from __future__ import annotations

import copy

import torch

# the shipped first-stage loss (training/loss/scenedino.yaml)
SHIPPED = {"type": "reconstruction",
           "coarse": {"criterion": "l1+ssim", "dino_criterion": "cosine"},
           "invalid_policy": "weight_guided", "reconstruct_dino": True, "lambda_dino_coarse": 0.2,
           "temperature_dino": 5,
           "regularizations": [{"type": "edge_aware_smoothness", "lambda": 0.001},
                               {"type": "dino_edge_aware_smoothness", "lambda": 0.25}]}

# (n, pc, h, w, nv, K)
SHAPES = {"p16": (2, 2, 16, 16, 3, 8), "p8": (1, 3, 8, 8, 4, 8), "odd": (2, 1, 5, 7, 2, 8)}
# seeds whose top-2 view margin and policy margin are both >= 1e-5 on the f64 oracle
# (tests/test_recon_loss.py asserts it)
SEEDS = {"p16": 0, "p8": 1, "odd": 0}
LEAVES = ("rgb", "depth", "dino_features", "dino_features_downsampled")


def shipped(**over):
    c = copy.deepcopy(SHIPPED)
    for k, v in over.items():
        if v is None:
            c.pop(k, None)
        elif isinstance(v, dict) and isinstance(c.get(k), dict):
            c[k].update(v)
        else:
            c[k] = v
    return c


def make_data(shape, seed=0, C=64, gh=1, gw=1, artifacts=False, scales=1, fine=False,
              invalid_above=0.12):
    """The ``data`` dict the loss reads (plain float32 CPU tensors, no graph):
    rgb = rgb_gt + per-view noise of amplitude 0.1 (v + 1), weights = softmax(3 rand),
    invalid = rand > invalid_above (as 0 / 1 floats, the renderer's type), depth in [3, 43]."""
    n, pc, h, w, nv, K = shape
    g = torch.Generator().manual_seed(1234 + seed)

    def rand(*s):
        return torch.rand(*s, generator=g)

    gt = 0.2 + 0.45 * rand(n, pc, 1, 1, 3) + 0.3 * rand(n, pc, h, w, 3)
    data = {"rgb_gt": gt, "dino_gt": torch.randn(n, pc, gh, gw, C, generator=g)}
    if artifacts:
        data["dino_artifacts"] = 0.1 * torch.randn(n, pc, gh, gw, C, generator=g)
    amp = 0.1 * torch.arange(1, nv + 1, dtype=torch.float32).view(nv, 1)

    def part():
        return {"rgb": gt.unsqueeze(-2) + amp * (2 * rand(n, pc, h, w, nv, 3) - 1),
                "weights": torch.softmax(3 * rand(n, pc, h, w, K), dim=-1),
                "invalid": (rand(n, pc, h, w, K, nv) > invalid_above).float(),
                "depth": 3 + 40 * rand(n, pc, h, w),
                "dino_features": torch.randn(n, pc, h, w, 1, C, generator=g),
                "dino_features_downsampled": torch.randn(n, pc, gh, gw, 1, C, generator=g)}

    data["coarse"] = [part() for _ in range(scales)]
    if fine:
        data["fine"] = [part() for _ in range(scales)]
    return data


def convert(data, device="cpu", dtype=torch.float64, grad=True, dino_dtype=None):
    """A copy of ``data`` on device / dtype with the LEAVES of every part requiring grad.
    dino_dtype: the type of dino_features (values rounded to it first when it is bf16, on every
    device, so an oracle sees what the kernel reads)."""
    def conv(name, t):
        if name == "dino_features" and dino_dtype is not None:
            t = t.detach().to(dino_dtype)
            if device == "cpu":
                t = t.to(dtype)
            return t.to(device, copy=True)
        return t.detach().to(device=device, dtype=dtype, copy=True)

    out = {}
    for k, v in data.items():
        if k in ("coarse", "fine"):
            out[k] = []
            for p in v:
                q = {name: conv(name, t) for name, t in p.items()}
                if grad:
                    for name in LEAVES:
                        q[name].requires_grad_(True)
                out[k].append(q)
        else:
            out[k] = conv(k, v)
    return out


def leaves(data, part="coarse"):
    return [(f"{part}{i}.{name}", p[name]) for i, p in enumerate(data[part]) for name in LEAVES]


# name -> (config, shape key, make_data keywords)
CASES = {
    "shipped_p16": (shipped(), "p16", {}),
    "shipped_p8": (shipped(), "p8", {}),
    "shipped_odd": (shipped(), "odd", {}),
    "p8_grid_artifacts": (shipped(), "p8", {"gh": 2, "gw": 2, "artifacts": True}),
    "two_scales": (shipped(), "odd", {"scales": 2}),
    "l1": (shipped(coarse={"criterion": "l1"}), "odd", {}),
    "l2": (shipped(coarse={"criterion": "l2", "dino_criterion": "l2"}), "odd", {}),
    # 10 % invalid samples: strict masks about a third of the pixels
    "strict": (shipped(invalid_policy="strict"), "odd", {"invalid_above": 0.9}),
    "none": (shipped(invalid_policy="none"), "odd", {}),
    "median": (shipped(median_thresholding=True), "odd", {}),
    "fine": (shipped(fine={"criterion": "l2", "dino_criterion": "cosine", "lambda": 0.5},
                     lambda_dino_fine=0.3), "odd", {"fine": True}),
}


def case(name):
    cfg, key, kw = CASES[name]
    return copy.deepcopy(cfg), make_data(SHAPES[key], seed=SEEDS[key], **kw)


def projection(t):
    """A fixed pseudo-random direction of t's size (float64), to pin a whole tensor by one dot."""
    g = torch.Generator().manual_seed(t.numel())
    return torch.randn(t.numel(), generator=g, dtype=torch.float64)


def subset(t, limit=512):
    flat = t.reshape(-1)
    return flat[::max(1, -(-flat.numel() // limit))]
