"""Writes tests/golden/crop3d.npz: the reference's own ``BTSDownstreamWrapper.sample_3d_crop``
(scenedino/training/trainer_downstream.py:216-292) on the inputs of tests/_crop3d_inputs.py.

    SCENEDINO_REF=<reference checkout> python tests/golden/make_golden_crop3d.py

The trainer module does not import here (ignite), so the method is extracted with ``ast`` and
executed as it stands, on the CPU, as are ``gen_rays`` / ``unproj_map`` of common/util.py.
``Tensor.cuda`` is the identity meanwhile, and the method sees a ``torch`` whose ``randint`` /
``randn`` / ``rand`` serve the recorded draws (``randint(count)`` returns ``min(int(u * count),
count - 1)`` with the f32 product) and whose ``quantile`` / ``nonzero`` also record what they
return: the limits, the bin counts and the picked pixels.  The net is the analytic stand-in of
_crop3d_inputs.py, which records the positions it is handed.

Per case (arrays prefixed ``<case>_``): the inputs and draws, ``shift``, ``limits``, ``count``,
``pixel`` ((row, col), -1 for an empty bin), ``positions`` (n, kept bins, S, 3), and the two
returned arrays ``dino`` / ``occ``.  The seed of a case is the first one at which moving any
interpolated limit by one ulp changes no pixel's bin, no sample's sigma is within
SIGMA_MARGIN of the threshold and the case shows what it is meant to (``seeds``).
"""
from __future__ import annotations

import ast
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _crop3d_inputs as ci  # noqa: E402

REF = os.environ.get("SCENEDINO_REF", "")


def _functions(path, names, ns, cls=None):
    """Execute the named function definitions of a reference file (of class ``cls`` if given)
    in namespace ``ns``."""
    tree = ast.parse(open(path).read())
    body = tree.body
    if cls is not None:
        body = [n for n in body if isinstance(n, ast.ClassDef) and n.name == cls][0].body
    defs = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {d.name for d in defs} == set(names), (path, names)
    for d in defs:
        d.decorator_list = []
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns


class _Torch:
    """``torch`` as the method sees it: the recorded draws instead of the RNG, and a log."""

    def __init__(self, case):
        self.case, self.frame = case, 0
        n = case["pick"].shape[0]
        self.limits = []
        self.count = [[] for _ in range(n)]
        self.pixel = [[] for _ in range(n)]
        self._last = None

    def __getattr__(self, name):
        return getattr(torch, name)

    def quantile(self, *a, **k):
        out = torch.quantile(*a, **k)
        self.limits.append(out.clone())
        return out

    def nonzero(self, *a, **k):
        out = torch.nonzero(*a, **k)
        self._last = out
        self.count[self.frame].append(out.size(0))
        if out.size(0) == 0:
            self.pixel[self.frame].append([-1, -1])
        return out

    def randint(self, high, size):
        i = len(self.count[self.frame]) - 1  # the bin whose pixels were just listed
        u = np.float32(self.case["pick"][self.frame, i])
        r = min(int(u * np.float32(high)), high - 1)
        self.pixel[self.frame].append(self._last[r].tolist())
        return torch.tensor([r])

    def randn(self, k, s, three, device=None):
        return self.case["unit"][self.frame, :k].clone()

    def rand(self, k, s, one):
        out = self.case["rad"][self.frame, :k].clone()
        self.frame += 1
        return out


class _Net(ci.StandInNet):
    def forward(self, xyz, **kwargs):
        self.positions = xyz.clone()
        return super().forward(xyz, **kwargs)


def run_reference(case):
    util = types.SimpleNamespace(**{k: v for k, v in _functions(
        os.path.join(REF, "scenedino", "common", "util.py"), ["gen_rays", "unproj_map"],
        {"torch": torch}).items() if k in ("gen_rays", "unproj_map")})
    proxy = _Torch(case)
    fn = _functions(os.path.join(REF, "scenedino", "training", "trainer_downstream.py"),
                    ["sample_3d_crop"], {"torch": proxy, "util": util},
                    cls="BTSDownstreamWrapper")["sample_3d_crop"]
    net = _Net()
    me = types.SimpleNamespace(renderer=types.SimpleNamespace(net=net))
    saved = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # torch.range
            dino, occ = fn(me, case["poses"], case["projs"], case["depth"], z_far=ci.Z_FAR,
                           n_crops=ci.N_CROPS, n_samples=ci.N_SAMPLES, sample_radius=ci.RADIUS,
                           sigma_threshold=ci.THR)
    finally:
        torch.Tensor.cuda = saved
    n = case["pick"].shape[0]
    kept_bins = len([c for c in proxy.count[0] if c > 0])
    return {"limits": torch.stack(proxy.limits), "count": torch.tensor(proxy.count),
            "pixel": torch.tensor(proxy.pixel),
            "positions": net.positions.view(n, kept_bins, ci.S, 3), "dino": dino, "occ": occ}


def _oversampling_is(value):
    src = open(os.path.join(REF, "scenedino", "training", "trainer_downstream.py")).read()
    return f"oversampling = {value}" in src


def build_case(name):
    from scenedino_amd.training import crop3d
    _, _, _, plateau, edge = ci.CASES[name]
    for seed in range(64):
        case = ci.make_case(name, seed)
        if edge:
            shift = ci.shift_of(case["unit"], case["rad"])
            centre = crop3d.centres_torch(case["depth"], case["poses"], case["projs"], ci.Z_FAR,
                                          case["pick"], shift)[3]
            case = ci.shape_edge_case(case, centre, seed)
            if case is None:
                continue
        out = run_reference(case)
        if not ci.limits_are_robust(case["depth"][:, 0].numpy(), out["limits"].numpy()):
            continue
        count = out["count"]
        empty = (count == 0)
        if plateau and not (empty[0, -1] and not empty[0, :-1].any()):
            continue
        if not plateau and empty.any():
            continue
        sigma = ci.StandInNet.field(out["positions"])[0]
        if float((sigma - ci.THR).abs().min()) <= ci.SIGMA_MARGIN:
            continue
        n_occ = (sigma > ci.THR).sum(-1)
        if edge and not (int(n_occ[0, 0]) == ci.N_SAMPLES and int(n_occ[0, 1]) == ci.N_SAMPLES + 1):
            continue
        if out["dino"] is None:
            continue
        case["shift"] = ci.shift_of(case["unit"], case["rad"])
        return seed, case, out
    raise RuntimeError(f"{name}: no seed satisfies the fixture's conditions")


def main():
    if not os.path.isdir(os.path.join(REF, "scenedino")):
        raise SystemExit("set SCENEDINO_REF to a checkout of the reference")
    assert _oversampling_is(ci.OVERSAMPLING)
    arrays, seeds = {}, []
    for name in ci.CASES:
        seed, case, out = build_case(name)
        seeds.append(seed)
        for k, v in {**case, **out}.items():
            arrays[f"{name}_{k}"] = v.numpy()
        print(name, "seed", seed, "count", out["count"].tolist(), "returned", tuple(out["dino"].shape))
    arrays["seeds"] = np.asarray(seeds)
    path = os.path.join(HERE, "crop3d.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
